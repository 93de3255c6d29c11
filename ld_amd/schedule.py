"""The ``lr_config`` of a config: mmcv 1.2's ``StepLrUpdaterHook`` (the only
policy configs/ld, configs/ldv2 and configs/gfl use: ``_base_/schedules/
schedule_1x.py``), restated for ``SGDTrainer``.

    lr_config = dict(policy='step', warmup='linear', warmup_iters=500,
                     warmup_ratio=0.001, step=[8, 11])

Keys: ``step`` (int or list of milestones), ``gamma`` (0.1), ``min_lr``,
``by_epoch`` (True), ``warmup`` (None, 'constant', 'linear', 'exp'),
``warmup_iters``, ``warmup_ratio`` (0.1).  Anything else raises.

The hook's order is kept exactly: ``before_train_epoch`` sets the regular lr
(by_epoch only), ``before_train_iter`` sets the warmup lr while
``iter < warmup_iters``, the regular lr at ``iter == warmup_iters`` and nothing
after that (by_epoch); with ``by_epoch=False`` every iteration sets one or the
other.  The base lr of a group is its ``initial_lr``.
"""

__all__ = ['StepLrSchedule', 'build_lr_schedule']

_KEYS = {'policy', 'step', 'gamma', 'min_lr', 'by_epoch', 'warmup',
         'warmup_iters', 'warmup_ratio'}


class StepLrSchedule:
    """Stateful like the mmcv hook: ``before_run(base_lrs)`` once, then
    ``before_train_epoch(epoch)`` / ``before_train_iter(epoch, it)`` return the
    new lr of every group, or None when the hook would leave the lr alone."""

    def __init__(self, step, gamma=0.1, min_lr=None, by_epoch=True,
                 warmup=None, warmup_iters=0, warmup_ratio=0.1):
        if isinstance(step, (list, tuple)):
            step = [int(s) for s in step]
            if any(s <= 0 for s in step):
                raise ValueError(f'lr_config.step: milestones must be > 0, got {step}')
        elif isinstance(step, int):
            if step <= 0:
                raise ValueError(f'lr_config.step must be > 0, got {step}')
        else:
            raise TypeError('lr_config.step must be an int or a list of ints')
        if warmup is not None:
            if warmup not in ('constant', 'linear', 'exp'):
                raise ValueError(f'"{warmup}" is not a supported type for warming '
                                 'up, valid types are "constant", "linear" and "exp"')
            if int(warmup_iters) <= 0:
                raise ValueError('"warmup_iters" must be a positive integer')
            if not 0 < float(warmup_ratio) <= 1.0:
                raise ValueError('"warmup_ratio" must be in range (0,1]')
        self.step, self.gamma, self.min_lr = step, float(gamma), min_lr
        self.by_epoch, self.warmup = bool(by_epoch), warmup
        self.warmup_iters = int(warmup_iters) if warmup is not None else 0
        self.warmup_ratio = float(warmup_ratio)
        self.base_lr = None
        self.regular_lr = None

    # -- the hook's arithmetic ----------------------------------------------
    def get_lr(self, progress, base_lr):
        if isinstance(self.step, int):
            exp = progress // self.step
        else:
            exp = len(self.step)
            for i, s in enumerate(self.step):
                if progress < s:
                    exp = i
                    break
        lr = base_lr * self.gamma**exp
        if self.min_lr is not None:
            lr = max(lr, self.min_lr)
        return lr

    def get_regular_lr(self, epoch, it):
        progress = epoch if self.by_epoch else it
        return [self.get_lr(progress, b) for b in self.base_lr]

    def get_warmup_lr(self, it):
        if self.warmup == 'constant':
            return [lr * self.warmup_ratio for lr in self.regular_lr]
        if self.warmup == 'linear':
            k = (1 - it / self.warmup_iters) * (1 - self.warmup_ratio)
            return [lr * (1 - k) for lr in self.regular_lr]
        k = self.warmup_ratio**(1 - it / self.warmup_iters)  # 'exp'
        return [lr * k for lr in self.regular_lr]

    # -- the hook's call points ------------------------------------------------
    def before_run(self, base_lrs):
        self.base_lr = [float(b) for b in base_lrs]
        self.regular_lr = None

    def before_train_epoch(self, epoch, it=0):
        if not self.by_epoch:
            return None
        self.regular_lr = self.get_regular_lr(epoch, it)
        return list(self.regular_lr)

    def before_train_iter(self, epoch, it):
        if not self.by_epoch:
            self.regular_lr = self.get_regular_lr(epoch, it)
            if self.warmup is None or it >= self.warmup_iters:
                return list(self.regular_lr)
            return self.get_warmup_lr(it)
        if self.regular_lr is None:  # no epoch began under this schedule yet
            self.before_train_epoch(epoch, it)
        if self.warmup is None or it > self.warmup_iters:
            return None
        if it == self.warmup_iters:
            return list(self.regular_lr)
        return self.get_warmup_lr(it)

    def lr_at(self, base_lr, epoch, it):
        """The lr one group with ``base_lr`` trains with at (epoch, iter) when
        every epoch began with ``before_train_epoch``: a pure function."""
        regular = self.get_lr(epoch if self.by_epoch else it, base_lr)
        if self.warmup is None or it >= self.warmup_iters:
            return regular
        saved = self.regular_lr
        self.regular_lr = [regular]
        try:
            return self.get_warmup_lr(it)[0]
        finally:
            self.regular_lr = saved


def build_lr_schedule(lr_config):
    """``cfg.lr_config`` -> StepLrSchedule (None for None).  Only
    ``policy='step'``; other policies and unknown keys raise."""
    if lr_config is None:
        return None
    cfg = dict(lr_config)
    policy = cfg.pop('policy', None)
    if policy is None:
        raise ValueError('lr_config needs a policy')
    if str(policy).lower() != 'step':
        raise NotImplementedError(
            f"lr_config.policy={policy!r}: only 'step' (StepLrUpdaterHook) is "
            'supported')
    unknown = sorted(set(cfg) - _KEYS)
    if unknown:
        raise NotImplementedError(f'lr_config key {unknown[0]!r} is not supported '
                                  f'(supported: {sorted(_KEYS)})')
    if 'step' not in cfg:
        raise ValueError("lr_config.step is required for policy='step'")
    return StepLrSchedule(**cfg)
