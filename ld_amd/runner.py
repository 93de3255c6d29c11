"""A thin epoch loop over a config's schedule: what mmcv 1.2's
``EpochBasedRunner`` with ``LrUpdaterHook``, ``OptimizerHook``,
``TextLoggerHook`` (json part) and ``CheckpointHook`` does around the train
step, restated for ``SGDTrainer`` / ``AutoStepper``.

    trainer = SGDTrainer.from_config(model, cfg)
    EpochRunner(trainer, cfg, work_dir).run(lambda epoch: batches_of(epoch))

``make_epoch_batches(epoch)`` returns the epoch's device batches (dicts of
``img``, ``img_metas``, ``gt_bboxes``, ``gt_labels``); a
``dataloader.DeviceDataLoader`` over a ``datasets`` dataset is one.  With
``SGDTrainer(virtual_ranks=W)`` the items are lists of W such batches
(``dataloader.VirtualRankLoader``): one log line per optimizer step, ``iter``
counted as the W-rank job counts it.  Config
keys read: ``runner.max_epochs`` (or the older ``total_epochs``),
``log_config.interval``, ``checkpoint_config.interval`` and ``resume_from``.

``val=(loader, dataset, eval_cfg)`` is mmdet's ``EvalHook``: after every
``eval_cfg['interval']`` (default 1) epochs ``apis.single_gpu_test`` runs over
the test-mode ``loader`` and ``dataset.evaluate(results, **eval_cfg)`` (without
``interval``) gives the metrics, appended to the log as one ``mode='val'``
line (``epoch``, ``iter``, ``lr`` and the metrics).  Without ``val`` nothing
changes.

Every ``log_config.interval`` iterations one JSON line goes to
``work_dir/train.log.json``: ``mode, epoch, iter`` (1-based within the epoch,
as mmcv writes them), ``lr``, the iteration's ``log_vars`` and, with gradient
clipping, ``grad_norm``.  These are the values of that iteration (mmcv's
LogBuffer averages over the interval, which would read every iteration back):
the host waits for the device only at log points and checkpoints.  Every
``checkpoint_config.interval`` epochs ``epoch_{k}.pth`` is written through
``checkpoint.save_checkpoint`` with mmcv's meta (``epoch=k, iter``).
"""
import json
import os

from . import checkpoint as CK

__all__ = ['EpochRunner']


def _get(cfg, key, default=None):
    if cfg is None:
        return default
    try:
        v = cfg.get(key, default)
    except AttributeError:
        v = getattr(cfg, key, default)
    return default if v is None else v


class EpochRunner:

    def __init__(self, trainer_or_stepper, cfg, work_dir, val=None):
        self.stepper = trainer_or_stepper
        self.trainer = getattr(trainer_or_stepper, 'trainer', trainer_or_stepper)
        self.cfg = cfg
        self.work_dir = str(work_dir)
        runner = _get(cfg, 'runner', {})
        self.max_epochs = _get(runner, 'max_epochs', _get(cfg, 'total_epochs'))
        self.log_interval = int(_get(_get(cfg, 'log_config', {}), 'interval', 50))
        self.ckpt_interval = int(_get(_get(cfg, 'checkpoint_config', {}),
                                      'interval', 1))
        self.resume_from = _get(cfg, 'resume_from')
        self.log_path = os.path.join(self.work_dir, 'train.log.json')
        os.makedirs(self.work_dir, exist_ok=True)
        self.val = val
        self.val_records = []
        if val is not None:
            self.val_interval = int(_get(val[2], 'interval', 1))

    def validate(self, epoch_done):
        """One evaluation pass -> the ``mode='val'`` record it logged."""
        from .apis import single_gpu_test
        loader, dataset, eval_cfg = self.val
        kw = {k: v for k, v in dict(eval_cfg or {}).items() if k != 'interval'}
        model = self.trainer.model
        was_training = model.training
        results = single_gpu_test(model, loader)
        model.train(was_training)
        metrics = dataset.evaluate(results, **kw)
        rec = dict(mode='val', epoch=epoch_done, iter=len(loader),
                   lr=float(self.trainer.lr))
        rec.update({k: (v if isinstance(v, str) else float(v))
                    for k, v in metrics.items()})
        with open(self.log_path, 'a') as f:
            f.write(json.dumps(rec) + '\n')
        self.val_records.append(rec)
        return rec

    def _log(self, epoch, inner, out):
        rec = dict(mode='train', epoch=epoch + 1, iter=inner + 1,
                   lr=float(self.trainer.lr))
        rec.update({k: float(v) for k, v in dict(out['log_vars']).items()})
        if 'grad_norm' in out:
            rec['grad_norm'] = float(out['grad_norm'])
        with open(self.log_path, 'a') as f:
            f.write(json.dumps(rec) + '\n')
        return rec

    def save(self, epoch_done):
        path = os.path.join(self.work_dir, f'epoch_{epoch_done}.pth')
        CK.save_checkpoint(self.trainer.model, path, optimizer=self.trainer,
                           meta=dict(epoch=epoch_done, iter=self.trainer.iter))
        return path

    def _stream(self, make_epoch_batches, start, stop):
        """(epoch, inner, batch) over the epochs, pulled lazily: the runner
        holds at most the current batch and the next one."""
        for epoch in range(start, stop):
            for inner, data in enumerate(make_epoch_batches(epoch)):
                yield epoch, inner, data

    def _end_epoch(self, epoch):
        if (epoch + 1) % self.ckpt_interval == 0:
            self.save(epoch + 1)
        if self.val is not None and (epoch + 1) % self.val_interval == 0:
            self.validate(epoch + 1)

    def run(self, make_epoch_batches, max_epochs=None):
        """Train from ``trainer.epoch`` (after ``resume_from``, if set) to
        ``max_epochs``; returns the list of log records written.

        ``make_epoch_batches(epoch)`` may return any iterable (a generator
        included): it is consumed one batch ahead of the step, the look-ahead
        being the step's ``next_data``.  The look-ahead crosses epoch
        boundaries, so ``make_epoch_batches(e + 1)`` is called while epoch
        ``e``'s last step is prepared (before its checkpoint); an
        ``AutoStepper('pipelined')`` thus gets every batch once, in order, as
        the previous call's ``next_data``."""
        if max_epochs is None:
            max_epochs = self.max_epochs
        if max_epochs is None:
            raise ValueError('EpochRunner: no runner.max_epochs / total_epochs '
                             'in the config and none given')
        lw = getattr(make_epoch_batches, 'virtual_ranks', None)
        tw = getattr(self.trainer, 'virtual_ranks', 1)
        if lw is not None and lw != tw:
            raise ValueError(f'EpochRunner: a loader of {lw} virtual ranks '
                             f'with a trainer of {tw}')
        if self.resume_from:
            CK.resume(self.trainer, self.resume_from)
        pipelined = getattr(self.stepper, 'mode', None) == 'pipelined'
        max_epochs = int(max_epochs)
        epoch = int(self.trainer.epoch)
        records = []
        if epoch < max_epochs:
            stream = self._stream(make_epoch_batches, epoch, max_epochs)
            self.trainer.begin_epoch(epoch)
            cur = next(stream, None)
            while True:
                if cur is None or cur[0] != epoch:  # epoch ``epoch`` is done
                    self._end_epoch(epoch)
                    epoch += 1
                    if epoch >= max_epochs:
                        break
                    self.trainer.begin_epoch(epoch)
                    continue
                _, inner, data = cur
                nxt = next(stream, None)
                # the pipelined step loads next_data for a following call: at
                # the very end there is none, so it is handed its own batch
                nd = nxt[2] if nxt is not None else (data if pipelined else None)
                out = self.stepper.step(data, next_data=nd)
                if (inner + 1) % self.log_interval == 0:
                    records.append(self._log(epoch, inner, out))
                cur = nxt
        self.trainer.epoch = max_epochs
        return records
