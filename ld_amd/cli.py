"""What tools/train.py, tools/test.py and tools/benchmark.py share: mmcv's
``DictAction`` (``--cfg-options a.b=1 c=[1,2]``) and the options of the
reference's tools that are refused by name."""
import argparse
import ast

__all__ = ["DictAction", "add_refused", "check_refused", "load_for_test",
           "dump_config", "pop_test_samples_per_gpu"]


class DictAction(argparse.Action):
    """``KEY=VALUE`` pairs -> a dict; values are Python literals when they
    parse (ints, floats, bools, None, lists, tuples) and strings otherwise;
    ``a,b`` without brackets is a list, as in mmcv."""

    @staticmethod
    def _value(text):
        low = text.strip()
        if low.lower() in ('true', 'false'):
            return low.lower() == 'true'
        if low.lower() in ('none', 'null'):
            return None
        try:
            return ast.literal_eval(low)
        except (ValueError, SyntaxError):
            pass
        if ',' in low and not low.startswith(('[', '(')):
            return [DictAction._value(v) for v in low.split(',')]
        return low

    def __call__(self, parser, namespace, values, option_string=None):
        options = dict(getattr(namespace, self.dest, None) or {})
        for kv in values:
            if '=' not in kv:
                parser.error(f'{option_string}: expected KEY=VALUE, got {kv!r}')
            key, val = kv.split('=', maxsplit=1)
            options[key] = self._value(val)
        setattr(namespace, self.dest, options)


# option -> (argparse keywords, why it is refused)
REFUSED = {
    '--launcher': (dict(default='none'),
                   'one process drives one device; start ranks with torchrun '
                   'and ld_amd.train instead'),
    '--gpu-collect': (dict(action='store_true'), 'no multi-process test loop'),
    '--tmpdir': (dict(), 'no multi-process test loop'),
    '--show': (dict(action='store_true'),
               'no interactive window; use --show-dir'),
    '--fuse-conv-bn': (dict(action='store_true'),
                       'the conv kernels already fold frozen BatchNorm'),
}


def add_refused(parser, names):
    for n in names:
        kw, why = REFUSED[n]
        parser.add_argument(n, help=f'not supported: {why}', **kw)


def check_refused(parser, args, names):
    for n in names:
        kw, why = REFUSED[n]
        v = getattr(args, n.lstrip('-').replace('-', '_'))
        if v != kw.get('default', False if 'action' in kw else None):
            parser.error(f'{n} is not supported: {why}')


def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(_plain(x) for x in v)
    return v


def dump_config(cfg, path):
    """The resolved config as a Python file of ``key = literal`` lines (what
    ``cfg.dump`` leaves in a work dir); it loads back through
    ``Config.fromfile``."""
    import pprint
    with open(path, 'w') as f:
        for k, v in dict(cfg._cfg_dict).items():
            f.write(f'{k} = {pprint.pformat(_plain(v), width=79)}\n')


def pop_test_samples_per_gpu(cfg):
    """tools/test.py:137-153: ``test_mode`` on, ``samples_per_gpu`` popped
    from the test block(s) (default 1)."""
    test = cfg.data['test']
    blocks = test if isinstance(test, list) else [test]
    spg = 1
    for b in blocks:
        b['test_mode'] = True
        spg = max(spg, b.pop('samples_per_gpu', 1))
    return spg


def load_for_test(cfg, checkpoint, device, classes=None):
    """tools/test.py:171-185: the config's detector without train_cfg, the
    checkpoint's weights, ``CLASSES`` from its meta or ``classes``."""
    from .checkpoint import load_checkpoint
    from .registry import build_detector
    mcfg = dict(cfg.model)
    mcfg['pretrained'] = None
    mcfg['train_cfg'] = None
    model = build_detector(mcfg, test_cfg=cfg.get('test_cfg'))
    ckpt = load_checkpoint(model, checkpoint, map_location='cpu')
    meta = ckpt.get('meta', {}) or {}
    model.CLASSES = meta['CLASSES'] if 'CLASSES' in meta else classes
    model.cfg = cfg
    return model.to(device).eval()
