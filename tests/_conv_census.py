"""Census of the conv launches a real step makes.

``Recorder`` wraps the conv entry points ON THE LOADED LIBRARY OBJECT (the
ctypes attributes ld_amd.layers looks up at every call) and the Python calls
that lead to them (layers.conv_forward_raw / _conv_backward).  The wrappers call
through unchanged and record the entry point, the ld_conv_t descriptor, the
epilogue flags and how the operands arrived (fp32 or a C8 image, accumulating
or not); leaving the ``with`` block restores the originals.

A *unit* is one Python-level call (its kind, descriptor and operand kinds);
the entry points it reached are its *signatures*.  Replaying a unit with
seeded operands must reach the same signatures (test_gpu_conv_census.py).
"""
import ctypes as C

import torch

CONV_ENTRIES = (
    'ld_conv_forward', 'ld_conv_forward_smallc', 'ld_conv_bf16_forward',
    'ld_conv_bf16_forward_c8', 'ld_conv_dgrad', 'ld_conv_dgrad_acc',
    'ld_conv_bf16_dgrad', 'ld_conv_bf16_dgrad_acc', 'ld_conv_bf16_dgrad_c8',
    'ld_conv_bf16_dgrad_c8_acc', 'ld_conv_wgrad', 'ld_conv_bf16_wgrad',
    'ld_conv_bf16_wgrad_c8', 'ld_conv_wgrad_partial')
OTHER_ENTRIES = ('ld_bottleneck_c8_forward', 'ld_gconv_forward',
                 'ld_deform_im2col')


def desc_tuple(d):
    """ld_conv_t -> (N, Cin, Cout, k, stride, pad, levels)."""
    assert d.KH == d.KW
    return (d.N, d.Cin, d.Cout, d.KH, d.stride, d.pad,
            tuple((d.lv[l].Hin, d.lv[l].Win) for l in range(d.num_levels)))


def _obj(a):
    return getattr(a, '_obj', a)


def _ep_flags(ep):
    return tuple(int(bool(getattr(ep, f))) for f in (
        'bias', 'scale', 'shift', 'residual', 'residual_c8', 'y_c8', 'y_raw',
        'y_raw_c8')) + (int(ep.relu), )


def _kind(t):
    from ld_amd import layers as Y
    if t is None:
        return 'none'
    if isinstance(t, Y.C8Act):
        return 'c8'
    if Y._unwritten(t):
        return 'unwritten'
    return 'cached' if Y._c8_cached(t) is not None else 'f32'


class Recorder:

    def __init__(self):
        self.units = {}  # unit key -> {'sigs': set, 'count': int, 'tags': set}
        self.other = {}  # composite-launch signature -> count / tags
        self.tag = ''
        self._stack = []

    # ------------------------------------------------------------ wrappers --
    def _lib_wrapper(self, name, fn):
        rec = self

        def call(*args):
            rc = fn(*args)
            if name in CONV_ENTRIES:
                d = desc_tuple(_obj(args[0]))
                extra = ()
                if name.startswith('ld_conv_forward') or '_forward' in name:
                    extra = _ep_flags(_obj(args[3]))
                elif name in ('ld_conv_wgrad', 'ld_conv_bf16_wgrad',
                              'ld_conv_bf16_wgrad_c8'):
                    extra = (int(args[4]), )  # accumulate
                elif name == 'ld_conv_wgrad_partial':
                    extra = (int(args[1]), )  # family
                sig = (name, d, extra)
                if rec._stack:
                    rec._stack[-1][1].add(sig)
                else:
                    rec._note_other(('orphan', ) + sig)
            elif name == 'ld_bottleneck_c8_forward':
                b = _obj(args[0])
                rec._note_other((name, b.N, b.H, b.W, b.Cin, b.mid))
            elif name == 'ld_gconv_forward':
                # x, img, y, N, cin, cout, groups, k, stride, pad, h, w, scale,
                # shift, relu, stream
                rec._note_other((name, ) + tuple(int(v) for v in args[3:12]) +
                                (int(bool(args[12])), int(args[14])))
            elif name == 'ld_deform_im2col':
                # x, off, N, cin, h, w, kh, kw, stride, pad, dilation, col, st
                rec._note_other((name, ) + tuple(int(v) for v in args[2:11]))
            return rc
        call.__wrapped__ = fn
        return call

    def _note_other(self, key):
        e = self.other.setdefault(key, dict(count=0, tags=set()))
        e['count'] += 1
        e['tags'].add(self.tag)

    def _unit(self, key, run):
        from ld_amd import layers as Y
        sigs = set()
        self._stack.append((key, sigs))
        try:
            return run()
        finally:
            self._stack.pop()
            full = key + (Y.get_precision(), )
            e = self.units.setdefault(full, dict(sigs=set(), count=0,
                                                 tags=set()))
            e['sigs'] |= sigs
            e['count'] += 1
            e['tags'].add(self.tag)

    def _fwd_wrapper(self, fn):
        rec = self

        def conv_forward_raw(x3, w, stride, pad, levels, bias=None, scale=None,
                             shift=None, residual=None, relu=False,
                             emit_c8=False, c8_only=False, y_raw=None,
                             y_raw_c8=None):
            from ld_amd import layers as Y
            N, cin, _ = x3.shape
            cout, _, kh, _ = w.shape
            d, _ = Y.conv_desc(N, cin, cout, kh, kh, stride, pad, levels)
            key = ('fwd', desc_tuple(d), _kind(x3), bias is not None,
                   scale is not None, _kind(residual), bool(relu),
                   bool(emit_c8), bool(c8_only), y_raw is not None,
                   y_raw_c8 is not None)
            return rec._unit(key, lambda: fn(
                x3, w, stride, pad, levels, bias=bias, scale=scale,
                shift=shift, residual=residual, relu=relu, emit_c8=emit_c8,
                c8_only=c8_only, y_raw=y_raw, y_raw_c8=y_raw_c8))
        return conv_forward_raw

    def _bwd_wrapper(self, fn):
        rec = self

        def _conv_backward(x3, x8, w, dy, meta, params, need_x, need_w,
                           need_b, addend=None):
            from ld_amd import layers as Y
            xs = x8 if x8 is not None else x3
            N, cin, _ = xs.shape
            cout, _, kh, _ = w.shape
            stride, pad, levels, has_bias = meta
            d, _ = Y.conv_desc(N, cin, cout, kh, kh, stride, pad, levels)
            sink = Y._sink(params[0]) is not None
            key = ('bwd', desc_tuple(d), 'c8' if x8 is not None else _kind(x3),
                   _kind(dy), bool(need_x), bool(need_w), addend is not None,
                   sink, sink and Y._DEFER_ON[0])
            return rec._unit(key, lambda: fn(x3, x8, w, dy, meta, params,
                                              need_x, need_w, need_b,
                                              addend=addend))
        return _conv_backward

    def __enter__(self):
        from ld_amd import layers as Y
        from ld_amd import lib as L
        lib = L.get_lib()
        self._saved_lib = {}
        for name in CONV_ENTRIES + OTHER_ENTRIES:
            fn = getattr(lib, name)
            self._saved_lib[name] = fn
            setattr(lib, name, self._lib_wrapper(name, fn))
        self._saved_py = (Y.conv_forward_raw, Y._conv_backward)
        Y.conv_forward_raw = self._fwd_wrapper(Y.conv_forward_raw)
        Y._conv_backward = self._bwd_wrapper(Y._conv_backward)
        return self

    def __exit__(self, *exc):
        from ld_amd import layers as Y
        from ld_amd import lib as L
        lib = L.get_lib()
        for name, fn in self._saved_lib.items():
            setattr(lib, name, fn)
        Y.conv_forward_raw, Y._conv_backward = self._saved_py
        return False

    def signatures(self):
        return {s for e in self.units.values() for s in e['sigs']}


# ----------------------------------------------------------- the configs --
def _batch(dev, pad, img_shape):
    from ld_amd import synthetic
    b = synthetic.synthetic_batch(2, img_shape, pad, 7, 1234)
    return dict(img=b['img'].to(dev), img_metas=b['img_metas'],
                gt_bboxes=[x.to(dev) for x in b['gt_bboxes']],
                gt_labels=[x.to(dev) for x in b['gt_labels']])


CONFIGS = ('c1_r18', 'c2_r50_fp32', 'c3_r50_bf16', 'c4_r101_dcn_fwd',
           'c5_ldv2_x101', 'infer_r50')


def run_config(name, rec, dev):
    """One forward and backward (config 4: forward only) of a BASELINE
    config at its per-GPU size, recorded into ``rec``."""
    from ld_amd import layers as Y
    from ld_amd import model_zoo
    from ld_amd.train import SGDTrainer
    big = ((800, 1344), (800, 1333))
    pad, shape = ((800, 800), (800, 800)) if name == 'c1_r18' else big
    cfg = {
        'c1_r18': lambda: model_zoo.ld_detector(18, 101, with_vlr_kd=False),
        'c2_r50_fp32': lambda: model_zoo.ld_detector(50, 101),
        'c3_r50_bf16': lambda: model_zoo.ld_detector(50, 101),
        'c4_r101_dcn_fwd': model_zoo.ld_r101_dcn_detector,
        'c5_ldv2_x101': lambda: model_zoo.ldv2_x101_detector(50),
        'infer_r50': lambda: model_zoo.ld_detector(50, 101),
    }[name]()
    Y.set_precision('bf16' if name == 'c3_r50_bf16' else 'fp32')
    try:
        det = model_zoo.build_seeded(cfg, dev)
        data = _batch(dev, pad, shape)
        rec.tag = name
        with rec:
            if name == 'c4_r101_dcn_fwd':
                det(**data)
            elif name == 'infer_r50':
                det.eval()
                with torch.no_grad():
                    det.simple_test(data['img'], data['img_metas'])
            else:
                SGDTrainer(det, lr=0.0025).step(data)
            Y.wgrad_join(dev)
            Y.flush_deferred(dev)
        torch.cuda.synchronize()
    finally:
        Y.set_precision('fp32')
        Y.drop_deferred()
    del det
    torch.cuda.empty_cache()
