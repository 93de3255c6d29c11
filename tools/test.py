"""Test (and evaluate) a detector from its config: the reference's
tools/test.py on one device.

    python tools/test.py CONFIG CHECKPOINT --eval mAP            # VOC
    python tools/test.py CONFIG CHECKPOINT --eval bbox           # COCO
    python tools/test.py CONFIG CHECKPOINT --out results.pkl \\
        [--format-only] [--show-dir DIR --show-score-thr 0.3] \\
        [--eval-options k=v ...] [--cfg-options k=v ...]

Builds ``cfg.data.test`` (``ld_amd.datasets``), a sequential
``DeviceDataLoader``, the config's detector with the checkpoint's weights, runs
``single_gpu_test`` and ``dataset.evaluate(results, **cfg.evaluation,
metric=...)``.  Not supported, refused by name: --launcher other than none,
--gpu-collect, --tmpdir, --show, --fuse-conv-bn.
"""
import argparse
import os.path as osp
import pickle
import sys

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))

REFUSED = ('--launcher', '--gpu-collect', '--tmpdir', '--show',
           '--fuse-conv-bn')


def parse_args(argv=None):
    from ld_amd.cli import DictAction, add_refused, check_refused
    p = argparse.ArgumentParser(description='Test (and eval) a model')
    p.add_argument('config', help='test config file path')
    p.add_argument('checkpoint', help='checkpoint file')
    p.add_argument('--out', help='output result file in pickle format')
    p.add_argument('--format-only', action='store_true',
                   help='format the results (dataset.format_results) without '
                   'evaluating them')
    p.add_argument('--eval', type=str, nargs='+',
                   help='evaluation metrics: bbox, proposal, proposal_fast '
                   'for COCO; mAP, recall for PASCAL VOC')
    p.add_argument('--show-dir',
                   help='directory where painted images will be saved')
    p.add_argument('--show-score-thr', type=float, default=0.3,
                   help='score threshold (default: 0.3)')
    p.add_argument('--cfg-options', nargs='+', action=DictAction,
                   help='override config settings, KEY=VALUE')
    p.add_argument('--eval-options', nargs='+', action=DictAction,
                   help='keyword arguments of dataset.evaluate / '
                   'format_results, KEY=VALUE')
    p.add_argument('--device', default='cuda:0')
    add_refused(p, REFUSED)
    args = p.parse_args(argv)
    check_refused(p, args, REFUSED)
    # tools/test.py:104-114 of the reference
    assert args.out or args.eval or args.format_only or args.show_dir, \
        ('Please specify at least one operation (save/eval/format/show the '
         'results / save the results) with the argument "--out", "--eval"'
         ', "--format-only" or "--show-dir"')
    if args.eval and args.format_only:
        raise ValueError('--eval and --format_only cannot be both specified')
    if args.out is not None and not args.out.endswith(('.pkl', '.pickle')):
        raise ValueError('The output file must be a pkl file.')
    return args


def main(argv=None):
    args = parse_args(argv)
    import torch
    from ld_amd import Config
    from ld_amd.apis import single_gpu_test
    from ld_amd.cli import load_for_test, pop_test_samples_per_gpu
    from ld_amd.dataloader import build_dataloader
    from ld_amd.datasets import build_dataset
    cfg = Config.fromfile(args.config)
    if args.cfg_options is not None:
        cfg.merge_from_dict(args.cfg_options)
    samples_per_gpu = pop_test_samples_per_gpu(cfg)
    dataset = build_dataset(cfg.data['test'])
    device = torch.device(args.device)
    loader = build_dataloader(
        dataset, samples_per_gpu, cfg.data.get('workers_per_gpu', 1),
        dist=False, shuffle=False, device=device)
    model = load_for_test(cfg, args.checkpoint, device, dataset.CLASSES)
    outputs = single_gpu_test(model, loader, args.show_dir,
                              args.show_score_thr)
    loader.close()
    if args.out:
        print(f'\nwriting results to {args.out}')
        with open(args.out, 'wb') as f:
            pickle.dump(outputs, f)
    kwargs = {} if args.eval_options is None else args.eval_options
    if args.format_only:
        dataset.format_results(outputs, **kwargs)
    if args.eval:
        eval_kwargs = dict(cfg.get('evaluation', {}) or {})
        for key in ('interval', 'tmpdir', 'start', 'gpu_collect', 'save_best',
                    'rule'):
            eval_kwargs.pop(key, None)
        eval_kwargs.update(dict(metric=args.eval, **kwargs))
        print(dataset.evaluate(outputs, **eval_kwargs))


if __name__ == '__main__':
    main()
