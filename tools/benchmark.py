"""Inference speed in images per second: the reference's
tools/analysis_tools/benchmark.py loop.

    python tools/benchmark.py CONFIG CHECKPOINT [--log-interval 50] \\
        [--max-images 2000] [--out profiles/inference_fps.json]

One image per step over ``cfg.data.test``; the first 5 images warm up; every
``model(...)`` call is bracketed by device synchronisation and the pure
inference time is accumulated; stops after ``--max-images`` images (2000 in
the reference) or the end of the dataset.  The loader decodes ahead, so decode
is outside the timed region, as the reference's DataLoader workers are.
Not supported, refused by name: --fuse-conv-bn.
"""
import argparse
import json
import os.path as osp
import sys
import time

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))

REFUSED = ('--fuse-conv-bn', )
NUM_WARMUP = 5


def parse_args(argv=None):
    from ld_amd.cli import DictAction, add_refused, check_refused
    p = argparse.ArgumentParser(description='Benchmark a model')
    p.add_argument('config', help='test config file path')
    p.add_argument('checkpoint', help='checkpoint file')
    p.add_argument('--log-interval', type=int, default=50,
                   help='interval of logging')
    p.add_argument('--max-images', type=int, default=2000)
    p.add_argument('--out', help='write the result as json')
    p.add_argument('--cfg-options', nargs='+', action=DictAction,
                   help='override config settings, KEY=VALUE')
    p.add_argument('--device', default='cuda:0')
    add_refused(p, REFUSED)
    args = p.parse_args(argv)
    check_refused(p, args, REFUSED)
    return args


def measure(model, loader, log_interval=50, max_images=2000, log=print):
    """-> (fps, images timed)."""
    import torch
    dev = next(model.parameters()).device
    pure, timed, fps = 0.0, 0, float('nan')
    for i, data in enumerate(loader):
        torch.cuda.synchronize(dev)
        start = time.perf_counter()
        with torch.no_grad():
            model(return_loss=False, rescale=True, **data)
        torch.cuda.synchronize(dev)
        elapsed = time.perf_counter() - start
        if i >= NUM_WARMUP:
            pure += elapsed
            timed = i + 1 - NUM_WARMUP
            fps = timed / pure
            if (i + 1) % log_interval == 0:
                log(f'Done image [{i + 1:<3}/ {max_images}], fps: {fps:.1f} '
                    'img / s')
        if i + 1 == max_images:
            break
    log(f'Overall fps: {fps:.1f} img / s')
    return fps, timed


def main(argv=None):
    args = parse_args(argv)
    import torch
    from ld_amd import Config
    from ld_amd.cli import load_for_test, pop_test_samples_per_gpu
    from ld_amd.dataloader import build_dataloader
    from ld_amd.datasets import build_dataset
    cfg = Config.fromfile(args.config)
    if args.cfg_options is not None:
        cfg.merge_from_dict(args.cfg_options)
    pop_test_samples_per_gpu(cfg)
    dataset = build_dataset(cfg.data['test'])
    device = torch.device(args.device)
    loader = build_dataloader(dataset, 1, cfg.data.get('workers_per_gpu', 1),
                              dist=False, shuffle=False, device=device)
    model = load_for_test(cfg, args.checkpoint, device, dataset.CLASSES)
    fps, timed = measure(model, loader, args.log_interval, args.max_images)
    loader.close()
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(dict(config=osp.basename(args.config), fps=fps,
                           images_timed=timed, warmup_images=NUM_WARMUP,
                           device=torch.cuda.get_device_name(device)), f,
                      indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
