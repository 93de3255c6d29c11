"""Train a detector from its config: the reference's tools/train.py on one
device.

    python tools/train.py CONFIG [--work-dir DIR] [--resume-from CKPT] \\
        [--no-validate] [--seed N] [--deterministic] [--cfg-options k=v ...] \\
        [--virtual-gpus W]

Builds the config's detector, ``cfg.data.train`` (and ``cfg.data.val`` unless
--no-validate), a ``DeviceDataLoader`` seeded with --seed,
``SGDTrainer.from_config`` and ``EpochRunner``; dumps the resolved config into
the work dir; checkpoints carry ``CLASSES`` in their meta.  With a seed a run
is reproducible batch for batch (the loader's draws are a function of (seed,
epoch, batch)).  Not supported, refused by name: --launcher other than none.

``--virtual-gpus W`` is the reference's ``dist_train.sh CONFIG W`` on one
device: every optimizer step takes the W rank-local batches of a W-process
job (``SGDTrainer(virtual_ranks=W)``, ``build_dataloader(virtual_ranks=W)``)
and ``optimizer.lr`` stays as the config wrote it for that job.
"""
import argparse
import os
import os.path as osp
import sys

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))

REFUSED = ('--launcher', )


def parse_args(argv=None):
    from ld_amd.cli import DictAction, add_refused, check_refused
    p = argparse.ArgumentParser(description='Train a detector')
    p.add_argument('config', help='train config file path')
    p.add_argument('--work-dir', help='the dir to save logs and models')
    p.add_argument('--resume-from', help='the checkpoint file to resume from')
    p.add_argument('--no-validate', action='store_true',
                   help='do not evaluate the checkpoints during training')
    p.add_argument('--seed', type=int, default=None, help='random seed')
    p.add_argument('--deterministic', action='store_true',
                   help='deterministic options for the torch backend')
    p.add_argument('--cfg-options', nargs='+', action=DictAction,
                   help='override config settings, KEY=VALUE')
    p.add_argument('--device', default='cuda:0')
    p.add_argument('--virtual-gpus', type=int, default=1, metavar='W',
                   help='train as a W-process job would, on one device')
    add_refused(p, REFUSED)
    args = p.parse_args(argv)
    check_refused(p, args, REFUSED)
    return args


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import torch
    from ld_amd import Config, build_detector
    from ld_amd.cli import dump_config
    from ld_amd.dataloader import build_dataloader
    from ld_amd.datasets import build_dataset
    from ld_amd.runner import EpochRunner
    from ld_amd.train import SGDTrainer
    cfg = Config.fromfile(args.config)
    if args.cfg_options is not None:
        cfg.merge_from_dict(args.cfg_options)
    # tools/train.py:96-105: CLI > config > ./work_dirs/<config name>
    if args.work_dir is not None:
        work_dir = args.work_dir
    elif cfg.get('work_dir') is not None:
        work_dir = cfg.work_dir
    else:
        work_dir = osp.join('./work_dirs',
                            osp.splitext(osp.basename(args.config))[0])
    if args.resume_from is not None:
        cfg.merge_from_dict(dict(resume_from=args.resume_from))
    os.makedirs(work_dir, exist_ok=True)
    dump_config(cfg, osp.join(work_dir, osp.basename(args.config)))
    if args.seed is not None:  # apis/train.py set_random_seed
        import random
        random.seed(args.seed)
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
    if args.deterministic:
        torch.backends.cudnn.deterministic = True
        torch.backends.cudnn.benchmark = False
    device = torch.device(args.device)
    model = build_detector(dict(cfg.model), train_cfg=cfg.get('train_cfg'),
                           test_cfg=cfg.get('test_cfg')).to(device)
    model.train()
    dataset = build_dataset(cfg.data['train'])
    model.CLASSES = dataset.CLASSES  # saved into the checkpoints' meta
    workers = cfg.data.get('workers_per_gpu', 1)
    W = args.virtual_gpus
    loader = build_dataloader(dataset, cfg.data['samples_per_gpu'], workers,
                              dist=False, seed=args.seed, device=device,
                              virtual_ranks=W if W != 1 else None)
    val = None
    if not args.no_validate and cfg.data.get('val') is not None:
        vcfg = dict(cfg.data['val'])
        vspg = vcfg.pop('samples_per_gpu', 1)
        vset = build_dataset(vcfg, dict(test_mode=True))
        val = (build_dataloader(vset, vspg, workers, dist=False,
                                shuffle=False, device=device), vset,
               dict(cfg.get('evaluation', {}) or {}))
    trainer = SGDTrainer.from_config(model, cfg, virtual_ranks=W)
    runner = EpochRunner(trainer, cfg, work_dir, val=val)
    runner.run(loader)
    torch.cuda.synchronize(device)
    loader.close()
    if val is not None:
        val[0].close()
    print(f'trained {trainer.epoch} epochs, {trainer.iter} iterations; '
          f'checkpoints and train.log.json in {work_dir}')


if __name__ == '__main__':
    main()
