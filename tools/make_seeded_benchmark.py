"""Everything tools/benchmark.py needs for a run without a dataset or trained
weights: N seeded 640 x 480 JPEGs with a middle-format annotation file, a
config for the GFL R50 detector (``model_zoo.gfl_detector(50)``) testing them at
img_scale (1333, 800), and a checkpoint of its seeded synthetic weights.

    python tools/make_seeded_benchmark.py OUT_DIR [--images 120]
    python tools/benchmark.py OUT_DIR/gfl_r50_seeded.py OUT_DIR/gfl_r50_seeded.pth \\
        --out profiles/inference_fps.json

The detections of seeded weights mean nothing; the convolutions, the head and
``ld_get_bboxes`` do the work of a trained model of the same shape (score_thr
0.05 leaves few boxes for NMS, a trained model leaves more).
"""
import argparse
import os
import os.path as osp
import sys

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))

CONFIG = '''\
from ld_amd import model_zoo

model = model_zoo.gfl_detector(50)
norm = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375],
            to_rgb=True)
test_pipeline = [
    dict(type='LoadImageFromFile'),
    dict(type='MultiScaleFlipAug', img_scale=(1333, 800), flip=False,
         transforms=[dict(type='Resize', keep_ratio=True),
                     dict(type='RandomFlip'),
                     dict(type='Normalize', **norm),
                     dict(type='Pad', size_divisor=32),
                     dict(type='ImageToTensor', keys=['img']),
                     dict(type='Collect', keys=['img'])])]
data = dict(samples_per_gpu=1, workers_per_gpu=2,
            test=dict(type='CustomDataset', ann_file={ann!r},
                      img_prefix={root!r}, classes=('thing', ),
                      pipeline=test_pipeline))
'''


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Seeded inputs for benchmark.py')
    p.add_argument('out_dir')
    p.add_argument('--images', type=int, default=120)
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    import importlib.util
    from ld_amd import checkpoint, synthetic
    from ld_amd.registry import build_detector
    from ld_amd import model_zoo
    spec = importlib.util.spec_from_file_location(
        '_bench_loader', osp.join(osp.dirname(osp.abspath(__file__)),
                                  'bench_loader.py'))
    bl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bl)
    root = osp.abspath(args.out_dir)
    os.makedirs(root, exist_ok=True)
    bl.write_images(root, args.images)
    with open(osp.join(root, 'gfl_r50_seeded.py'), 'w') as f:
        f.write(CONFIG.format(ann=osp.join(root, 'ann.pkl'), root=root))
    det = build_detector(model_zoo.gfl_detector(50))
    det.load_state_dict(synthetic.seeded_state_dict(det.state_dict(), seed=1))
    checkpoint.save_checkpoint(det, osp.join(root, 'gfl_r50_seeded.pth'))
    print(root)


if __name__ == '__main__':
    main()
