"""Images per second of the loader alone: JPEG decode (host threads) + upload +
``ld_preprocess_batch``, no model.

    python tools/bench_loader.py [--images 200] [--threads 2 8 16] \\
        [--out profiles/dataloader_latency.json]

Writes ``--images`` seeded 640 x 480 JPEGs into a temporary directory, loads
them through a train-mode ``DeviceDataLoader`` at ``img_scale=(1333, 800)``,
samples_per_gpu 2, once per thread count.  Timing: one warm-up epoch, then the
median of ``--repeats`` epochs, each ending in a device synchronise.  The
result is printed next to the recorded train step rates (README: 58.4 img/s
fp32, 188 img/s bf16); a loader below them limits training, and the stage that
limits it is the one whose own rate (decode only, measured in the same run) is
lowest.  Needs a GPU: there is no CPU figure.
"""
import argparse
import json
import os
import os.path as osp
import statistics
import sys
import tempfile
import time

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))

STEP_RATES = dict(fp32=58.4, bf16=188.0)  # README, img/s per GPU
PIPELINE = [
    dict(type='LoadImageFromFile'),
    dict(type='LoadAnnotations', with_bbox=True),
    dict(type='Resize', img_scale=(1333, 800), keep_ratio=True),
    dict(type='RandomFlip', flip_ratio=0.5),
    dict(type='Normalize', mean=[123.675, 116.28, 103.53],
         std=[58.395, 57.12, 57.375], to_rgb=True),
    dict(type='Pad', size_divisor=32),
    dict(type='DefaultFormatBundle'),
    dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels']),
]


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Loader-only throughput')
    p.add_argument('--images', type=int, default=200)
    p.add_argument('--threads', type=int, nargs='+', default=[2, 8, 16])
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--out', help='write the result as json')
    return p.parse_args(argv)


def write_images(root, n, seed=0):
    """n seeded 640 x 480 JPEGs and their middle-format annotation file."""
    import pickle

    import numpy as np
    from PIL import Image
    rng = np.random.RandomState(seed)
    infos = []
    for k in range(n):
        small = rng.randint(0, 256, size=(60, 80, 3))
        pix = np.kron(small, np.ones((8, 8, 1))).astype(np.uint8)
        pix = (pix.astype(np.int16) + rng.randint(-12, 13, pix.shape)).clip(
            0, 255).astype(np.uint8)
        name = f'{k:06d}.jpg'
        Image.fromarray(pix, 'RGB').save(osp.join(root, name), quality=90)
        infos.append(dict(filename=name, width=640, height=480, ann=dict(
            bboxes=np.array([[40, 50, 300, 400]], np.float32),
            labels=np.array([0], np.int64))))
    with open(osp.join(root, 'ann.pkl'), 'wb') as f:
        pickle.dump(infos, f)


def epoch_rate(loader, epoch, device_half=True):
    import torch
    t0 = time.perf_counter()
    n = 0
    if device_half:
        for data in loader(epoch):
            n += data['img'].shape[0]
        torch.cuda.synchronize()
    else:
        for host in loader.host_batches(epoch):
            n += len(host['images'])
    return n / (time.perf_counter() - t0)


def main(argv=None):
    args = parse_args(argv)
    import torch
    from ld_amd.dataloader import DeviceDataLoader
    from ld_amd.datasets import CustomDataset
    assert torch.cuda.is_available(), 'bench_loader needs the GPU'
    rows = []
    with tempfile.TemporaryDirectory() as root:
        write_images(root, args.images)
        ds = CustomDataset(ann_file=osp.join(root, 'ann.pkl'),
                           pipeline=PIPELINE, classes=('thing', ),
                           img_prefix=root, filter_empty_gt=False)
        for threads in args.threads:
            ld = DeviceDataLoader(ds, 2, 1, seed=0, device='cuda:0',
                                  num_threads=threads)
            epoch_rate(ld, 0)  # warm-up: code objects, pinned pools, threads
            full = [epoch_rate(ld, 1 + r) for r in range(args.repeats)]
            dec = [epoch_rate(ld, 1 + r, False) for r in range(args.repeats)]
            ld.close()
            row = dict(threads=threads,
                       images_per_s=statistics.median(full),
                       images_per_s_min=min(full), images_per_s_max=max(full),
                       decode_only_images_per_s=statistics.median(dec))
            row['sustains'] = {k: row['images_per_s'] >= v
                               for k, v in STEP_RATES.items()}
            rows.append(row)
            print(json.dumps(row), flush=True)
    result = dict(images=args.images, size='640x480',
                  img_scale=[1333, 800], samples_per_gpu=2,
                  repeats=args.repeats, step_rates_img_per_s=STEP_RATES,
                  host_cpus_used=os.environ.get('OMP_NUM_THREADS'),
                  device=torch.cuda.get_device_name(0), rows=rows)
    print(json.dumps(result))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
