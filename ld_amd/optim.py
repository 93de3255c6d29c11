"""The ``optimizer`` / ``optimizer_config`` of a config: mmcv 1.2's
``DefaultOptimizerConstructor`` (paramwise_cfg) and ``OptimizerHook``
(grad_clip), restated for the flat-arena ``SGDTrainer``.

    optimizer = dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001,
                     paramwise_cfg=dict(bias_lr_mult=2.0, bias_decay_mult=0.0))
    optimizer_config = dict(grad_clip=dict(max_norm=35, norm_type=2))

mmcv builds one parameter group per parameter.  Here every parameter gets an
``(lr_mult, decay_mult)`` pair by the constructor's rules; the distinct pairs
are the *classes* (2-4 on the LD configs), and the optimizer launch reads its
(lr, weight decay) from a per-class table with one uint8 class id per 64-float
chunk of the arena (csrc/optim.hip).  Rules, in mmcv's order:

  * ``custom_keys`` first: keys sorted alphabetically, then by decreasing
    length; the first key that is a substring of ``f'{prefix}.{name}'`` sets
    ``lr_mult`` / ``decay_mult`` and no other rule applies;
  * otherwise ``name == 'bias'`` of a module that is not a norm:
    ``lr * bias_lr_mult``; a norm module: ``wd * norm_decay_mult``; a depthwise
    conv (``groups == in_channels``): ``wd * dwconv_decay_mult``; any other
    bias: ``wd * bias_decay_mult``.
Frozen parameters get a group with the defaults, as in mmcv.  Anything this
restatement does not cover raises ``NotImplementedError`` naming the key.
"""
import torch
import torch.nn as nn

__all__ = ['ParamClasses', 'build_optimizer', 'parse_grad_clip',
           'PARAMWISE_KEYS']

PARAMWISE_KEYS = ('custom_keys', 'bias_lr_mult', 'bias_decay_mult',
                  'norm_decay_mult', 'dwconv_decay_mult')
_SGD_KEYS = {'type', 'lr', 'momentum', 'weight_decay', 'paramwise_cfg',
             'nesterov', 'dampening'}
CHUNK = 64  # floats per class id: GradArena's parameter alignment


def _norm_types():
    from . import cnn
    from torch.nn.modules.batchnorm import _BatchNorm
    from torch.nn.modules.instancenorm import _InstanceNorm
    return (cnn.BatchNorm2d, cnn.GroupNorm, _BatchNorm, _InstanceNorm,
            nn.GroupNorm, nn.LayerNorm)


def _conv_types():
    from . import cnn
    return (cnn.Conv2d, cnn.GroupedConv2d, nn.Conv2d)


class ParamClasses:
    """Per-parameter multipliers of a model and the classes they fall into.

    ``mults[i]``: (lr_mult, decay_mult) of ``params[i]`` (``model.parameters()``
    order, frozen ones included); ``classes``: the distinct pairs, (1, 1) first
    when any parameter has it; ``class_of[i]``: index into ``classes``."""

    def __init__(self, params, names, mults):
        self.params, self.names = list(params), list(names)
        self.mults = [(float(a), float(b)) for a, b in mults]
        order = sorted(set(self.mults), key=lambda m: (m != (1.0, 1.0),
                                                       self.mults.index(m)))
        from .lib import LD_SGD_MAX_CLASSES
        if len(order) > LD_SGD_MAX_CLASSES:
            raise NotImplementedError(
                f'{len(order)} distinct (lr_mult, decay_mult) classes; the '
                f'optimizer table holds {LD_SGD_MAX_CLASSES}')
        self.classes = order
        index = {m: k for k, m in enumerate(order)}
        self.class_of = [index[m] for m in self.mults]

    def __len__(self):
        return len(self.classes)

    def chunk_ids(self, arena):
        """uint8 class id per 64-float chunk of ``arena`` (train.GradArena),
        on the arena's device."""
        if arena.numel % CHUNK or any(o % CHUNK for o in arena.offsets):
            raise ValueError('the class table needs every arena parameter on a '
                             f'{CHUNK}-float boundary (GradArena align % 64 == 0)')
        cls_of = {id(p): c for p, c in zip(self.params, self.class_of)}
        ids = torch.zeros(arena.numel // CHUNK, dtype=torch.uint8)
        for p, o in zip(arena.order, arena.offsets):
            n = (p.numel() + CHUNK - 1) // CHUNK
            ids[o // CHUNK:o // CHUNK + n] = cls_of[id(p)]
        return ids.to(arena.flat_param.device)

    def table(self, lr_of_class, wd_of_class):
        """Flat [lr_0, wd_0, lr_1, wd_1, ...] for the device table."""
        out = []
        for lr, wd in zip(lr_of_class, wd_of_class):
            out += [float(lr), float(wd)]
        return out


def classify(model, paramwise_cfg):
    """(names, [(lr_mult, decay_mult)]) per ``model.parameters()`` entry, by
    DefaultOptimizerConstructor.add_params' rules."""
    from . import cnn
    cfg = dict(paramwise_cfg or {})
    for k in cfg:
        if k not in PARAMWISE_KEYS:
            raise NotImplementedError(
                f'optimizer.paramwise_cfg key {k!r} is not supported '
                f'(supported: {", ".join(PARAMWISE_KEYS)})')
    custom = dict(cfg.get('custom_keys', {}) or {})
    for key, v in custom.items():
        bad = sorted(set(v) - {'lr_mult', 'decay_mult'})
        if bad:
            raise NotImplementedError(
                f'paramwise_cfg.custom_keys[{key!r}] key {bad[0]!r} is not '
                'supported (lr_mult, decay_mult)')
    sorted_keys = sorted(sorted(custom.keys()), key=len, reverse=True)
    bias_lr = float(cfg.get('bias_lr_mult', 1.0))
    bias_decay = float(cfg.get('bias_decay_mult', 1.0))
    norm_decay = float(cfg.get('norm_decay_mult', 1.0))
    dw_decay = float(cfg.get('dwconv_decay_mult', 1.0))
    norms, convs = _norm_types(), _conv_types()
    seen, names, mults = set(), [], []
    for prefix, module in model.named_modules():
        if cfg and isinstance(module, cnn._DeformConvPack) and \
                any(p.requires_grad for p in module.parameters()):
            # mmcv's dcn rules (no bias_lr_mult / bias_decay_mult under a DCN,
            # dcn_offset_lr_mult) touch trainable parameters only; a frozen
            # DCN's parameters get the defaults like any frozen parameter
            raise NotImplementedError(
                f'paramwise_cfg on a trainable deformable conv ({prefix}: '
                'mmcv\'s dcn_offset rules) is not supported')
        is_norm = isinstance(module, norms)
        is_dw = isinstance(module, convs) and \
            getattr(module, 'groups', 1) == module.in_channels
        for name, p in module.named_parameters(recurse=False):
            if id(p) in seen:
                continue
            seen.add(id(p))
            names.append(f'{prefix}.{name}' if prefix else name)
            lr_m, dec_m = 1.0, 1.0
            if not p.requires_grad:
                mults.append((lr_m, dec_m))
                continue
            full = f'{prefix}.{name}'
            for key in sorted_keys:
                if key in full:
                    lr_m = float(custom[key].get('lr_mult', 1.0))
                    dec_m = float(custom[key].get('decay_mult', 1.0))
                    break
            else:
                if name == 'bias' and not is_norm:
                    lr_m = bias_lr
                if is_norm:
                    dec_m = norm_decay
                elif is_dw:
                    dec_m = dw_decay
                elif name == 'bias':
                    dec_m = bias_decay
            mults.append((lr_m, dec_m))
    allp = list(model.parameters())
    if len(allp) != len(mults):
        raise RuntimeError('parameter walk does not match model.parameters()')
    return names, mults


def parse_grad_clip(optimizer_config):
    """``optimizer_config.grad_clip`` -> None or dict(max_norm, norm_type=2)."""
    oc = dict(optimizer_config or {})
    unknown = sorted(set(oc) - {'grad_clip', 'type'})
    if unknown:
        raise NotImplementedError(f'optimizer_config key {unknown[0]!r} is not '
                                  'supported (grad_clip)')
    if oc.get('type', 'OptimizerHook') != 'OptimizerHook':
        raise NotImplementedError(f"optimizer_config.type={oc['type']!r}: only "
                                  'OptimizerHook (fp32) is supported')
    gc = oc.get('grad_clip')
    if gc is None:
        return None
    gc = dict(gc)
    unknown = sorted(set(gc) - {'max_norm', 'norm_type'})
    if unknown:
        raise NotImplementedError(f'grad_clip key {unknown[0]!r} is not supported')
    if 'max_norm' not in gc:
        raise ValueError('grad_clip needs max_norm')
    norm_type = float(gc.get('norm_type', 2))
    if norm_type != 2.0:
        raise NotImplementedError(f'grad_clip norm_type={gc.get("norm_type")!r}: '
                                  'only the L2 norm (norm_type=2) is supported')
    return dict(max_norm=float(gc['max_norm']), norm_type=2)


def build_optimizer(model, optimizer_cfg, optimizer_config=None):
    """mmcv.runner.build_optimizer for SGD: a dict with ``lr``, ``momentum``,
    ``weight_decay``, ``param_classes`` (a ParamClasses, or None without
    ``paramwise_cfg``) and ``grad_clip`` (None or dict(max_norm, norm_type)) --
    the keyword arguments of ``SGDTrainer``."""
    cfg = dict(optimizer_cfg)
    typ = cfg.get('type', 'SGD')
    if typ != 'SGD':
        raise NotImplementedError(f'optimizer type {typ!r}: only SGD is supported')
    unknown = sorted(set(cfg) - _SGD_KEYS)
    if unknown:
        raise NotImplementedError(f'optimizer key {unknown[0]!r} is not supported')
    if cfg.get('nesterov', False):
        raise NotImplementedError('optimizer key \'nesterov\' is not supported')
    if cfg.get('dampening', 0) != 0:
        raise NotImplementedError('optimizer key \'dampening\' is not supported')
    if 'lr' not in cfg:
        raise ValueError('optimizer.lr is required')
    pw = cfg.get('paramwise_cfg')
    classes = None
    if pw is not None:
        names, mults = classify(model, pw)
        classes = ParamClasses(model.parameters(), names, mults)
    return dict(lr=float(cfg['lr']), momentum=float(cfg.get('momentum', 0.0)),
                weight_decay=float(cfg.get('weight_decay', 0.0)),
                param_classes=classes,
                grad_clip=parse_grad_clip(optimizer_config))
