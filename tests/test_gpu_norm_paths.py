"""Every dispatch path of the norm and glue kernels (csrc/nn.hip) against the
float64 references of tests/_norm_ref64.py: full comparisons at the smallest
shapes that reach each branch, every bound 16 u S, the image bound or
equality.

Inside an entry point the kernel choice is host logic; the predicates:
  ld_bn_act_forward      bn_act_fwd_kernel<true> iff P % 4 == 0 and x, y, res
                         16-byte aligned
  ld_bn_act_backward     bn_act_bwd_kernel<true> iff P % 4 == 0 and every
                         operand aligned; splits = nsplit(N, C, P, 0)
  ld_bn_act_backward_c8  P % 4 == 0, C % 8 == 0, N ceil(P / 256) <= 256 slots
  ld_bn_act_backward_c8in  V = 4 iff P % 4 == 0, else 2 (P % 2 == 0)
  ld_gn_forward          gn_apply4_kernel iff P % 4 == 0 and x, y aligned;
                         stats: one slice per 1024 cells (A > 1024), 16-byte
                         loads on the aligned body of a slice
  ld_gn_backward         gn_bwd_reduce_row_kernel + gn_bwd_apply_kernel<4> iff
                         P % 4 == 0 and dy, x, y, dx aligned; else the sliced
                         reduce + fold and gn_bwd_apply_kernel<1>
  ld_gn_*_c8*            C % 8 == 0 (the wrapper: C % 32), P % 4 == 0;
                         one_group iff (C / G) % 8 == 0
  ld_bias_grad_partial   16-byte loads iff P % 4 == 0 and dy aligned
  ld_maxpool3x3s2        vector form iff W % 4 == 0, W >= 8, x 16-byte aligned
Each case asserts the entry points it reached (CASES below) and its predicate.

Each case prints one line under -s: path, shape, entry points and the worst
|got - ref| / (u S) per output.  Worst ratio per entry point over all cases,
MI355X (the bar is 16; a forward entry counts the forward outputs, a backward
entry the gradients):
  ld_bn_act_forward         2.72    ld_gn_forward             3.30
  ld_bn_act_forward_c8      2.49    ld_gn_forward_c8          3.08
  ld_bn_act_backward        3.04    ld_gn_backward            4.48
  ld_bn_act_backward_c8     2.65    ld_gn_backward_c8         3.59
  ld_bn_act_backward_c8in   2.68    ld_gn_backward_c8_lean    3.59
  ld_bias_grad              0.16    ld_bias_grad_partial      0.16
  ld_upsample_add_forward   1.00    ld_upsample_add_backward  1.73
  ld_upsample_add_backward_acc 1.73
  ld_scale_levels_forward   1.00    ld_scale_levels_backward  1.00
  ld_maxpool3x3s2, ld_pack_levels(_c8), ld_unpack_levels(_c8): exact; every
  image written beside an fp32 output: exact.
"dx (literal)" in a GroupNorm line is a figure, not a check: the dx error over
the S that holds |m1|, |m2| instead of the magnitudes of the group means'
terms.  It reaches 283.8 on these kernels (65.5 on the case the host test
restates in fp32), which is why the helper does not use that S.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _norm_ref64 as R

pytestmark = pytest.mark.gpu

FAMILIES = ('ld_bn_act_', 'ld_gn_', 'ld_bias_grad', 'ld_maxpool3x3s2',
            'ld_upsample_add_', 'ld_pack_levels', 'ld_unpack_levels',
            'ld_scale_levels_')
EXTRA = ('ld_bn_bwd_finalize_batch', 'ld_bn_prepare', 'ld_conv_to_c8')

# test -> the entry points its cases must reach (asserted case by case)
CASES = {
    'gn_fp32': ('ld_gn_forward', 'ld_gn_backward',
                'ld_gn_forward_workspace_bytes',
                'ld_gn_backward_workspace_bytes'),
    'gn_bf16': ('ld_gn_forward_c8', 'ld_gn_backward_c8_lean',
                'ld_gn_backward_c8'),
    'gn_image_only': ('ld_gn_forward_c8', 'ld_gn_backward_c8_lean'),
    'bn_fp32': ('ld_bn_act_forward', 'ld_bn_act_backward',
                'ld_bn_act_backward_workspace_bytes',
                'ld_bn_act_backward_nsplit'),
    'bn_bf16': ('ld_bn_act_forward_c8', 'ld_bn_act_backward_c8',
                'ld_bn_act_backward'),
    'bn_c8in': ('ld_bn_act_backward_c8in', ),
    'bias': ('ld_bias_grad', 'ld_bias_grad_partial', 'ld_bias_grad_nsplit'),
    'maxpool': ('ld_maxpool3x3s2', ),
    'upsample': ('ld_upsample_add_forward', 'ld_upsample_add_backward_acc',
                 'ld_upsample_add_backward'),
    'pack_fp32': ('ld_pack_levels', 'ld_unpack_levels'),
    'pack_bf16': ('ld_pack_levels_c8', 'ld_unpack_levels_c8'),
    'scale': ('ld_scale_levels_forward', 'ld_scale_levels_backward',
              'ld_scale_levels_backward_workspace_bytes'),
}
UNREACHED = {}  # export -> why no checked case reaches it

WORST_SEEN = {}  # entry point -> worst ratio of the cases that reached it


def _dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def _exports():
    from ld_amd import lib as L
    return sorted(n for n in L.SIGNATURES if n.startswith(FAMILIES))


class Recorder:
    """Wraps the norm / glue entries on the loaded library object (the ctypes
    attributes ld_amd.layers looks up at every call) and notes which were
    called; leaving the block restores them."""

    def __init__(self):
        self.names = []

    def __enter__(self):
        from ld_amd import lib as L
        self.lib = L.get_lib()
        self.saved = {}
        for name in _exports() + list(EXTRA):
            fn = getattr(self.lib, name)
            self.saved[name] = fn
            setattr(self.lib, name, self._wrap(name, fn))
        return self

    def _wrap(self, name, fn):
        def call(*args):
            self.names.append(name)
            return fn(*args)
        call.__wrapped__ = fn
        return call

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)
        return False

    def expect(self, test, *names, absent=()):
        for n in names:
            assert n in CASES[test], (test, n)
            assert n in self.names, f'{test}: {n} not reached: {self.names}'
        for n in absent:
            assert n not in self.names, f'{test}: {n} reached'
        return names


_FORWARD_KEYS = ('y', 'mean', 'rstd', 'stats')


def _report(path, shape, entries, worst):
    """One line per case; a forward entry keeps the worst ratio of the forward
    outputs, a backward entry that of the gradients, any other entry all."""
    fwd = {k for k in worst if k.split()[0].rstrip('0123456789') in _FORWARD_KEYS}
    for e in entries:
        if e.endswith(('_bytes', '_nsplit')):
            continue  # host arithmetic, no kernel
        keys = fwd if 'forward' in e else set(worst) - fwd \
            if 'backward' in e else set(worst)
        keys = [k for k in keys if not k.endswith('(literal)')]
        WORST_SEEN[e] = max([WORST_SEEN.get(e, 0.0)] + [worst[k] for k in keys])
    print(f'\n{path} {shape} {"+".join(entries)} ' +
          ' '.join(f'{k}={v:.2f}' for k, v in worst.items()))


def _d(a, grad=False):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(
        _dev()).requires_grad_(grad)


def _offset_view(a, grad=False):
    """a on the device at an address 4 bytes off a 16-byte boundary."""
    a = np.asarray(a, dtype=np.float32)
    store = torch.empty(a.size + 1, dtype=torch.float32, device=_dev())
    v = store[1:].view(a.shape)
    v.copy_(torch.from_numpy(np.array(a)))
    v = v.detach().requires_grad_(grad)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _img(buf, shape):
    return R.c8_to_ncp(buf.float().cpu().numpy(), shape)


@pytest.fixture
def bf16_mode():
    from ld_amd import layers as Y
    Y.set_precision('bf16')
    try:
        yield Y
    finally:
        Y._GN_LEAN[0] = True
        Y.set_precision('fp32')


# --------------------------------------------------------------- GroupNorm --
@functools.lru_cache(maxsize=4)  # neighbouring cases share a reference
def _gn_ref(case):
    name, N, C, G, relu, variant = case
    d = R.gn_inputs(*case)
    f = R.gn_forward(d['x'], d['gamma'], d['beta'], G, R.EPS, d['levels'], relu)
    if relu:
        assert R.undecided(f['pre'], f['S']) == 0
    bw = R.gn_backward(d['dy'], d['x'], f['pre'] > 0 if relu else None,
                       d['gamma'], G, d['levels'], f)
    return d, f, bw


def _check_gn_stats(stats, f, worst):
    worst['mean'] = R.check(stats[0], f['mean'], f['S_mean'], 'mean')
    worst['rstd'] = R.check(stats[1], f['rstd'], f['rstd'], 'rstd',
                            bar=f['bar_rstd'])


@pytest.mark.parametrize('case', R.gn_fp32_cases(), ids=str)
def test_gn_fp32(case):
    from ld_amd import layers as Y
    name, N, C, G, relu, variant = case
    d, f, bw = _gn_ref(case)
    levels, P = d['levels'], R.PYRAMID_P[name]
    xd = _offset_view(d['x'], True) if variant == 'offset' else _d(d['x'], True)
    gd, bd, go = _d(d['gamma'], True), _d(d['beta'], True), _d(d['dy'])
    with Recorder() as rec:
        y = Y.gn_act(xd, gd, bd, G, R.EPS, levels, relu)
        y.backward(go)
        y2, img, stats = Y._gn_forward(xd.detach(), gd.detach(), bd.detach(), G,
                                       R.EPS, levels, relu)
    torch.cuda.synchronize()
    entries = rec.expect('gn_fp32', *CASES['gn_fp32'],
                         absent=('ld_gn_forward_c8', 'ld_gn_backward_c8',
                                 'ld_gn_backward_c8_lean'))
    vec = P % 4 == 0 and xd.data_ptr() % 16 == 0
    assert vec == (name in ('A', 'A8v', 'C', 'E') and variant != 'offset')
    assert img is None and torch.equal(y2, y)
    worst = {}
    worst['y'] = R.check(y, f['y'], f['S'], 'y')
    _check_gn_stats(stats, f, worst)
    worst['dx'] = R.check(xd.grad, *bw['dx'], 'dx')
    # a figure, not a check: the same error over S with |m1|, |m2| in place of
    # the magnitudes of the group means' terms (see _norm_ref64's docstring)
    err = np.abs(R.f64(xd.grad) - bw['dx'][0])
    worst['dx (literal)'] = float(np.where(
        err > 0, err / np.maximum(R.U * bw['dx_literal_S'], 1e-300), 0.0).max())
    worst['dgamma'] = R.check(gd.grad, *bw['dgamma'], 'dgamma')
    worst['dbeta'] = R.check(bd.grad, *bw['dbeta'], 'dbeta')
    _report(f'gn fp32 {"vector" if vec else "scalar"} {variant}'.strip(),
            (name, N, C, G, relu), entries[:2], worst)


@pytest.mark.parametrize('form', ['lean', 'c8'])
@pytest.mark.parametrize('case', R.GN_BF16_CASES, ids=str)
def test_gn_bf16(case, form, bf16_mode):
    Y = bf16_mode
    name, N, C, G, relu = case
    d, f, bw = _gn_ref(case + ('', ))
    levels, P = d['levels'], R.PYRAMID_P[name]
    assert C % 32 == 0 and P % 4 == 0
    Y._GN_LEAN[0] = form == 'lean'
    xd, gd, bd = _d(d['x'], True), _d(d['gamma'], True), _d(d['beta'], True)
    go = _d(d['dy'])
    seen = {}
    xd.register_hook(lambda g: seen.setdefault('dx', g))
    with Recorder() as rec:
        y = Y.gn_act(xd, gd, bd, G, R.EPS, levels, relu)
        y.backward(go)
        y2, img, stats = Y._gn_forward(xd.detach(), gd.detach(), bd.detach(), G,
                                       R.EPS, levels, relu)
    torch.cuda.synchronize()
    back = 'ld_gn_backward_c8_lean' if form == 'lean' else 'ld_gn_backward_c8'
    entries = rec.expect('gn_bf16', 'ld_gn_forward_c8', back,
                         absent=('ld_gn_forward', 'ld_gn_backward'))
    dx_img = Y._c8_cached(seen['dx'])
    assert img is not None and dx_img is not None and torch.equal(y2, y)
    worst = {}
    worst['y'] = R.check(y, f['y'], f['S'], 'y')
    worst['y image'] = R.check_image_of(_img(img, (N, C, P)), y, 'y image')
    _check_gn_stats(stats, f, worst)
    worst['dx'] = R.check(xd.grad, *bw['dx'], 'dx')
    worst['dx image'] = R.check_image_of(_img(dx_img, (N, C, P)), seen['dx'],
                                         'dx image')
    worst['dgamma'] = R.check(gd.grad, *bw['dgamma'], 'dgamma')
    worst['dbeta'] = R.check(bd.grad, *bw['dbeta'], 'dbeta')
    one_group = (C // G) % 8 == 0
    _report(f'gn bf16 {form} {"one_group" if one_group else "per-channel"}',
            case, entries, worst)


def test_gn_bf16_image_only_through_conv_gn_act(bf16_mode, monkeypatch):
    """conv_gn_act(c8_only=True) followed by a second layer: the first layer's
    output and both layers' dx exist only as C8 images.  The GroupNorm operands
    (the conv results, the incoming gradients) are taken where the wrapper
    hands them to the norm, and each norm launch is checked on its own."""
    Y = bf16_mode
    dev = _dev()
    levels, P, N, C, G = R.PYRAMIDS['A'], 380, 2, 64, 32
    orig_f, orig_b = Y._gn_forward, Y._gn_backward
    for attempt in range(4):  # settle by reseeding: the conv results are not ours
        calls = dict(fwd=[], bwd=[])

        def fwd(x3, gamma, beta, groups, eps, lv, relu, image_only=False):
            out = orig_f(x3, gamma, beta, groups, eps, lv, relu,
                         image_only=image_only)
            calls['fwd'].append((x3, gamma, beta, image_only, out))
            return out

        def bwd(dy, x3, y, gamma, beta, stats, groups, lv, relu, params, need_g,
                need_b, dx_c8_only=False, need_lean=False):
            out = orig_b(dy, x3, y, gamma, beta, stats, groups, lv, relu, params,
                         need_g, need_b, dx_c8_only=dx_c8_only,
                         need_lean=need_lean)
            calls['bwd'].append((dy, x3, gamma, dx_c8_only, out))
            return out

        monkeypatch.setattr(Y, '_gn_forward', fwd)
        monkeypatch.setattr(Y, '_gn_backward', bwd)
        rng = R._rng('conv_gn', attempt)
        t = [_d(R._randn(rng, N, C, P), True)]
        for _ in range(2):
            t += [_d(R._randn(rng, C, C, 3, 3) * np.float32(0.05), True),
                  _d(R._randn(rng, C), True), _d(R._randn(rng, C), True)]
        go = _d(R._randn(rng, N, C, P))
        with Recorder() as rec:
            h, lv = Y.conv_gn_act(t[0], t[1], t[2], t[3], G, R.EPS, 1, 1, levels,
                                  c8_only=True)
            assert Y._unwritten(h)
            y, _ = Y.conv_gn_act(h, t[4], t[5], t[6], G, R.EPS, 1, 1, lv)
            y.backward(go)
            with torch.no_grad():  # the frozen form: a C8Act comes back
                frozen, _ = Y.conv_gn_act(t[0].detach(), t[1].detach(),
                                          t[2].detach(), t[3].detach(), G, R.EPS,
                                          1, 1, levels, c8_only=True)
        torch.cuda.synchronize()
        assert isinstance(frozen, Y.C8Act)
        assert len(calls['fwd']) == 3 and len(calls['bwd']) == 2
        refs = []
        for x3, gamma, beta, image_only, out in calls['fwd']:
            f = R.gn_forward(x3, gamma, beta, G, R.EPS, levels, True)
            refs.append((f, R.undecided(f['pre'], f['S'])))
        if all(u == 0 for _, u in refs):
            break
    assert [u for _, u in refs] == [0, 0, 0]
    entries = rec.expect('gn_image_only', *CASES['gn_image_only'],
                         absent=('ld_gn_forward', 'ld_gn_backward',
                                 'ld_gn_backward_c8'))
    worst = {}
    for i, ((x3, gamma, beta, image_only, out), (f, _)) in enumerate(
            zip(calls['fwd'], refs)):
        yv, img, stats = out
        assert image_only == (i != 1) and (yv is None) == image_only
        if yv is None:
            worst[f'y{i} image alone'] = R.check_image_alone(
                _img(img, (N, C, P)), f['y'], f['S'], f'y{i} image')
        else:
            worst[f'y{i}'] = R.check(yv, f['y'], f['S'], f'y{i}')
            R.check_image_of(_img(img, (N, C, P)), yv, f'y{i} image')
        w = {}
        _check_gn_stats(stats, f, w)
        worst[f'stats{i}'] = max(w.values())
    # backward launches arrive last layer first; forward refs 1, 0 match them
    for i, (dy, x3, gamma, dx_c8_only, out) in enumerate(calls['bwd']):
        f = refs[1 - i][0]
        bw = R.gn_backward(dy, x3, f['pre'] > 0, gamma, G, levels, f)
        dx, dgamma, dbeta = out
        assert dx_c8_only and isinstance(dx, Y.C8Act)
        worst[f'dx{1 - i} image alone'] = R.check_image_alone(
            _img(dx.buf, (N, C, P)), *bw['dx'], f'dx{1 - i} image')
        worst[f'dgamma{1 - i}'] = R.check(dgamma, *bw['dgamma'], 'dgamma')
        worst[f'dbeta{1 - i}'] = R.check(dbeta, *bw['dbeta'], 'dbeta')
    _report('gn bf16 image-only', ('A', N, C, G, f'seed {attempt}'), entries,
            worst)


# ----------------------------------------------------------------- eval-BN --
@functools.lru_cache(maxsize=4)  # neighbouring cases share a reference
def _bn_ref(N, C, P, relu, with_res, tag=''):
    d = R.bn_inputs(N, C, P, relu, with_res, tag)
    f = R.bn_forward(d['x'], d['gamma'], d['beta'], d['mean'], d['var'], R.EPS,
                     d['res'], relu)
    if relu:
        assert R.undecided(f['pre'], f['S']) == 0
    bw = R.bn_backward(d['dy'], d['x'], f['pre'] > 0 if relu else None,
                       d['gamma'], d['mean'], d['var'], R.EPS)
    return d, f, bw


BN_SPLITS = {(3, 8, 1500): 2, (2, 20, 4100): 3}


def _bn_run(Y, d, relu, x_grad=True, p_grad=True, res_view=False, hook=None):
    xd = _d(d['x'], x_grad)
    gd, bd = _d(d['gamma'], p_grad), _d(d['beta'], p_grad)
    rd = None
    if d['res'] is not None:
        rd = _offset_view(d['res'], True) if res_view else _d(d['res'], True)
    if hook is not None:
        xd.register_hook(hook)
    y = Y.bn_act(xd, gd, bd, _d(d['mean']), _d(d['var']), R.EPS, rd, relu)
    y.backward(_d(d['dy']))
    torch.cuda.synchronize()
    return y, xd, gd, bd, rd


def _bn_checks(y, xd, gd, bd, rd, f, bw):
    worst = {'y': R.check(y, f['y'], f['S'], 'y')}
    if xd.grad is not None:
        worst['dx'] = R.check(xd.grad, *bw['dx'], 'dx')
    if rd is not None:
        worst['dres'] = R.check_exact(rd.grad, bw['dres'][0], 'dres')
    if gd.grad is not None:
        worst['dgamma'] = R.check(gd.grad, *bw['dgamma'], 'dgamma')
        worst['dbeta'] = R.check(bd.grad, *bw['dbeta'], 'dbeta')
    return worst


@pytest.mark.parametrize('shape', R.BN_SHAPES, ids=str)
@pytest.mark.parametrize('relu,with_res', R.BN_FLAGS)
def test_bn_fp32(shape, relu, with_res):
    from ld_amd import layers as Y
    from ld_amd import lib as L
    N, C, P = shape
    d, f, bw = _bn_ref(N, C, P, relu, with_res)
    with Recorder() as rec:
        out = _bn_run(Y, d, relu)
        ns = L.get_lib().ld_bn_act_backward_nsplit(N, C, P, 0)
    entries = rec.expect('bn_fp32', *CASES['bn_fp32'],
                         absent=('ld_bn_act_forward_c8', 'ld_bn_act_backward_c8'))
    assert ns == BN_SPLITS.get(shape, 1)
    worst = _bn_checks(*out, f, bw)
    _report(f'bn fp32 {"vector" if P % 4 == 0 else "scalar"} splits {ns}',
            shape + (relu, with_res), entries[:2], worst)


@pytest.mark.parametrize('shape', [(1, 24, 1028), (2, 40, 253), (3, 8, 1500)],
                         ids=str)
@pytest.mark.parametrize('mode', ['frozen', 'no_dx', 'res_view'])
def test_bn_fp32_operand_forms(shape, mode):
    """frozen: no parameter gradient is requested (partial == NULL, x aliases
    dy); no_dx: dx is null, only the parameter gradients come out; res_view:
    the residual is a misaligned view (scalar forward kernel)."""
    from ld_amd import layers as Y
    N, C, P = shape
    d, f, bw = _bn_ref(N, C, P, True, True)
    with Recorder() as rec:
        out = _bn_run(Y, d, True, x_grad=mode != 'no_dx', p_grad=mode != 'frozen',
                      res_view=mode == 'res_view')
    entries = rec.expect('bn_fp32', 'ld_bn_act_forward', 'ld_bn_act_backward')
    y, xd, gd, bd, rd = out
    assert (xd.grad is None) == (mode == 'no_dx')
    assert (gd.grad is None) == (mode == 'frozen')
    worst = _bn_checks(*out, f, bw)
    _report(f'bn fp32 {mode}', shape, entries, worst)


@pytest.mark.parametrize('shape', R.BN_BF16_SHAPES, ids=str)
def test_bn_bf16(shape, bf16_mode):
    Y = bf16_mode
    from ld_amd import lib as L
    N, C, P = shape
    d, f, bw = _bn_ref(N, C, P, True, True)
    seen = {}
    with Recorder() as rec:
        out = _bn_run(Y, d, True, hook=lambda g: seen.setdefault('dx', g))
        y, xd, gd, bd, rd = out
        y2 = Y._bn_act_forward(xd.detach(), gd.detach(), bd.detach(),
                               _d(d['mean']), _d(d['var']), R.EPS, rd.detach(),
                               True)[0]
    slots = L.get_lib().ld_bn_act_backward_nsplit(N, C, P, 1)
    assert slots == {252: 2, 1028: 5, 32772: 258}[P]
    covered = slots <= 256
    assert Y._bn_c8_covers(N, P) == covered
    if covered:
        entries = rec.expect('bn_bf16', 'ld_bn_act_forward_c8',
                             'ld_bn_act_backward_c8',
                             absent=('ld_bn_act_backward', ))
    else:  # the plain kernel; the image comes from a conversion of its own
        entries = rec.expect('bn_bf16', 'ld_bn_act_forward_c8',
                             'ld_bn_act_backward',
                             absent=('ld_bn_act_backward_c8', ))
    worst = _bn_checks(*out, f, bw)
    img = Y._c8_cached(y2)
    assert img is not None and torch.equal(y2, y)
    worst['y image'] = R.check_image_of(_img(img, shape), y, 'y image')
    dx_img = Y._c8_cached(seen['dx'])
    assert (dx_img is not None) == covered
    if not covered:
        dx_img = Y.to_c8(seen['dx'])
    worst['dx image'] = R.check_image_of(_img(dx_img, shape), seen['dx'],
                                         'dx image')
    _report(f'bn bf16 slots {slots}', shape, entries, worst)


@pytest.mark.parametrize('P', R.BN_C8IN_P)
@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('with_dres', [True, False])
def test_bn_backward_c8in(P, relu, with_dres):
    """ld_bn_act_backward_c8in through the ABI: y and x arrive as bf16 C8
    images built with to_c8; dgamma is held to what the ROUNDED x gives."""
    from ld_amd import layers as Y
    from ld_amd import lib as L
    N, C = 2, 32
    dev = _dev()
    d, f, _ = _bn_ref(N, C, P, relu, False, 'c8in')
    x_r = R.bf16_rne(d['x'])
    bw = R.bn_backward(d['dy'], x_r, f['pre'] > 0 if relu else None, d['gamma'],
                       d['mean'], d['var'], R.EPS)
    lib = L.get_lib()
    assert lib.ld_bn_act_backward_nsplit(N, C, P, 2) == {560: 6, 54: 2, 130: 4}[P]
    x_img = Y.to_c8(_d(d['x']))
    y_img = Y.to_c8(_d(R.f32(f['y']))) if relu else None
    R.check_exact(_img(x_img, (N, C, P)), x_r, 'x image')
    scale, _, rstd = Y._bn_prepare(_d(d['gamma']), _d(d['beta']), _d(d['mean']),
                                   _d(d['var']), R.EPS)
    mean, dy = _d(d['mean']), _d(d['dy'])
    ws = torch.empty(lib.ld_bn_act_backward_workspace_bytes(N, C, P),
                     dtype=torch.uint8, device=dev)
    worst = {}
    for dx_fp32 in (True, False):
        dx = torch.full((N, C, P), float('nan'), device=dev) if dx_fp32 else None
        dres = torch.full((N, C, P), float('nan'), device=dev) \
            if with_dres else None
        dx8 = torch.zeros(N * C * P, dtype=torch.bfloat16, device=dev)
        dgamma, dbeta = (torch.full((C, ), float('nan'), device=dev)
                         for _ in range(2))
        with Recorder() as rec:
            L.check(rec.lib.ld_bn_act_backward_c8in(
                L.ptr(dy), L.ptr(y_img), L.ptr(x_img), L.ptr(scale), L.ptr(mean),
                L.ptr(rstd), N, C, P, 1 if relu else 0, L.ptr(dx), L.ptr(dx8),
                L.ptr(dres), L.ptr(dgamma), L.ptr(dbeta), 0, L.ptr(ws),
                ws.numel(), L.stream_ptr(dev)), 'ld_bn_act_backward_c8in')
        torch.cuda.synchronize()
        entries = rec.expect('bn_c8in', 'ld_bn_act_backward_c8in')
        if dx_fp32:
            worst['dx'] = R.check(dx, *bw['dx'], 'dx')
            worst['dx image'] = R.check_image_of(_img(dx8, (N, C, P)), dx,
                                                 'dx image')
        else:
            worst['dx image alone'] = R.check_image_alone(
                _img(dx8, (N, C, P)), *bw['dx'], 'dx image alone')
        if with_dres:
            R.check_exact(dres, bw['dres'][0], 'dres')
        worst['dgamma'] = max(worst.get('dgamma', 0.0),
                              R.check(dgamma, *bw['dgamma'], 'dgamma'))
        worst['dbeta'] = max(worst.get('dbeta', 0.0),
                             R.check(dbeta, *bw['dbeta'], 'dbeta'))
    _report(f'bn c8in V={4 if P % 4 == 0 else 2}', (N, C, P, relu, with_dres),
            entries, worst)


# -------------------------------------------------------------------- glue --
@pytest.mark.parametrize('shape', R.BIAS_SHAPES, ids=str)
def test_bias_grad(shape):
    from ld_amd import layers as Y
    from ld_amd import lib as L
    N, C, P = shape
    dev = _dev()
    rng = R._rng('bias', shape)
    dy_h, db0_h = R._randn(rng, N, C, P), R._randn(rng, C)
    ref, S = R.bias_grad(dy_h)
    dy = _d(dy_h)
    st = L.stream_ptr(dev)
    worst = {}
    with Recorder() as rec:
        lib = rec.lib
        db = torch.full((C, ), float('nan'), device=dev)
        L.check(lib.ld_bias_grad(L.ptr(dy), N, C, P, L.ptr(db), 0, st),
                'ld_bias_grad')
        acc = _d(db0_h)
        L.check(lib.ld_bias_grad(L.ptr(dy), N, C, P, L.ptr(acc), 1, st),
                'ld_bias_grad')
        ns = lib.ld_bias_grad_nsplit(N, C, P)
        part = torch.empty(C * ns * 16, dtype=torch.uint8, device=dev)
        L.check(lib.ld_bias_grad_partial(L.ptr(dy), N, C, P, L.ptr(part),
                                         part.numel(), st),
                'ld_bias_grad_partial')
        fin = torch.full((C, ), float('nan'), device=dev)
        job = L.BnFinJobT()
        job.partial, job.dgamma, job.dbeta = part.data_ptr(), None, fin.data_ptr()
        job.C, job.nsplit, job.accumulate = C, ns, 0
        tab, bmap, nb = Y._job_table([job], [(C + 15) // 16], dev)
        L.check(lib.ld_bn_bwd_finalize_batch(L.ptr(tab), L.ptr(bmap), nb, st),
                'ld_bn_bwd_finalize_batch')
    torch.cuda.synchronize()
    entries = rec.expect('bias', *CASES['bias'])
    assert 'ld_bn_bwd_finalize_batch' in rec.names
    assert ns == {253: 1, 1500: 2, 4100: 3}[P]
    worst['db'] = R.check(db, ref, S, 'db')
    worst['db accumulated'] = R.check(acc, ref + R.f64(db0_h),
                                      S + np.abs(R.f64(db0_h)), 'db accumulated')
    worst['db partial+finalise'] = R.check(fin, ref, S, 'db partial')
    _report(f'bias grad {"vector" if P % 4 == 0 else "scalar"} splits {ns}',
            shape, entries, worst)


POOL_CASES = [(s, 'vector', '') for s in R.POOL_VEC] + \
    [(s, 'scalar', '') for s in R.POOL_SCALAR] + \
    [((5, 7, 12), 'scalar', 'view'), ((5, 7, 12), 'vector', 'negative')]


@pytest.mark.parametrize('shape,form,variant', POOL_CASES, ids=str)
def test_maxpool(shape, form, variant):
    from ld_amd import layers as Y
    rows, H, W = shape
    x = R._randn(R._rng('pool', shape, variant), 1, rows, H, W)
    if variant == 'negative':
        x = -np.abs(x) - np.float32(0.5)
    xd = _offset_view(x) if variant == 'view' else _d(x)
    vec = W % 4 == 0 and W >= 8 and xd.data_ptr() % 16 == 0
    assert vec == (form == 'vector')
    with Recorder() as rec:
        y = Y.maxpool3x3s2(xd)
    torch.cuda.synchronize()
    entries = rec.expect('maxpool', 'ld_maxpool3x3s2')
    ref = R.maxpool3x3s2(x)
    if variant == 'negative':
        assert (ref < 0).all()
    R.check_exact(y, ref, 'maxpool')
    _report(f'maxpool {form} {variant}'.strip(), shape, entries, {'y': 0.0})


@pytest.mark.parametrize('fine,coarse', R.UPSAMPLE, ids=str)
def test_upsample_add(fine, coarse):
    from ld_amd import layers as Y
    from ld_amd import lib as L
    dev = _dev()
    N, C = 2, 3
    rng = R._rng('up', fine, coarse)
    a, b = R._randn(rng, N, C, *fine), R._randn(rng, N, C, *coarse)
    go, add = R._randn(rng, N, C, *fine), R._randn(rng, N, C, *coarse)
    ad, bd, god, addd = _d(a, True), _d(b, True), _d(go), _d(add)
    st = L.stream_ptr(dev)
    with Recorder() as rec:
        y = Y.upsample_add(ad, bd)
        y.backward(god)
        acc = torch.full((N, C) + coarse, float('nan'), device=dev)
        L.check(rec.lib.ld_upsample_add_backward_acc(
            L.ptr(god), N * C, fine[0], fine[1], coarse[0], coarse[1],
            L.ptr(addd), L.ptr(acc), st), 'ld_upsample_add_backward_acc')
        plain = torch.full((N, C) + coarse, float('nan'), device=dev)
        L.check(rec.lib.ld_upsample_add_backward(
            L.ptr(god), N * C, fine[0], fine[1], coarse[0], coarse[1],
            L.ptr(plain), st), 'ld_upsample_add_backward')
    torch.cuda.synchronize()
    entries = rec.expect('upsample', *CASES['upsample'])
    worst = {'y': R.check(y, *R.upsample_add(a, b), 'y')}
    dfine, dc, S = R.upsample_add_backward(go, coarse)
    worst['d fine'] = R.check_exact(ad.grad, dfine, 'd fine')
    worst['d coarse'] = R.check(bd.grad, dc, S, 'd coarse')
    worst['d coarse abi'] = R.check(plain, dc, S, 'd coarse (abi)')
    _, dca, Sa = R.upsample_add_backward(go, coarse, add)
    worst['d coarse + addend'] = R.check(acc, dca, Sa, 'd coarse + addend')
    _report('upsample_add', (fine, coarse), entries, worst)


def _pack_case(Y, name, N, C, rec_test, images):
    levels = R.PYRAMIDS[name]
    P = R.PYRAMID_P[name]
    rng = R._rng('pack', name, C)
    feats_h = [R._randn(rng, N, C, h, w) for h, w in levels]
    dx3_h = R._randn(rng, N, C, P)
    feats = [_d(f, True) for f in feats_h]
    seen = {}
    for i, t in enumerate(feats):
        t.register_hook(lambda g, i=i: seen.setdefault(i, g))
    with Recorder() as rec:
        x3, lv = Y.pack_levels(feats)
        x3.backward(_d(dx3_h))
        # split: views forward; separate gradients come back through one pack
        leaf = _d(dx3_h, True)
        views = Y.split_levels(leaf, lv)
        gs = [_d(f) for f in feats_h]
        torch.autograd.backward(views, gs)
    torch.cuda.synchronize()
    assert lv == levels
    entries = rec.expect(rec_test, *CASES[rec_test])
    R.check_exact(x3, R.pack_levels(feats_h), 'pack')
    for got, want in zip(feats, R.unpack_levels(dx3_h, levels)):
        R.check_exact(got.grad, want, 'unpack')
    for got, want in zip(views, R.unpack_levels(dx3_h, levels)):
        R.check_exact(got, want, 'split')
    R.check_exact(leaf.grad, R.pack_levels(feats_h), 'split backward')
    if images:
        img = Y._c8_cached(x3)
        assert img is not None
        R.check_image_of(_img(img, (N, C, P)), x3, 'pack image')
        for i, (h, w) in enumerate(levels):
            gi = Y._c8_cached(seen[i])
            assert gi is not None
            R.check_image_of(_img(gi, (N, C, h * w)),
                             seen[i].reshape(N, C, h * w), 'unpack image')
    # round trip: unpack(pack(feats)) gives the maps back
    again = [_d(f, True) for f in feats_h]
    x3b, _ = Y.pack_levels(again)
    x3b.backward(x3b.detach().clone())
    torch.cuda.synchronize()
    for got, want in zip(again, feats_h):
        R.check_exact(got.grad, want, 'round trip')
    _report(f'pack/unpack {"bf16" if images else "fp32"}', (name, N, C), entries,
            {'copies': 0.0})


@pytest.mark.parametrize('name', ['A', 'A8'])
def test_pack_unpack_fp32(name):
    from ld_amd import layers as Y
    _pack_case(Y, name, 2, 5, 'pack_fp32', False)


@pytest.mark.parametrize('name', ['A', 'A8v'])
def test_pack_unpack_bf16(name, bf16_mode):
    _pack_case(bf16_mode, name, 2, 32, 'pack_bf16', True)


@pytest.mark.parametrize('name,N,C', [('A8', 2, 68), ('C', 2, 8)])
def test_scale_levels(name, N, C):
    from ld_amd import layers as Y
    from ld_amd import lib as L
    dev = _dev()
    levels, P = R.PYRAMIDS[name], R.PYRAMID_P[name]
    rng = R._rng('scale', name)
    x, dy = R._randn(rng, N, C, P), R._randn(rng, N, C, P)
    s, d0 = R._randn(rng, len(levels)), R._randn(rng, len(levels))
    xd, sd, god = _d(x, True), _d(s, True), _d(dy)
    with Recorder() as rec:
        y = Y.scale_levels(xd, sd, levels)
        y.backward(god)
        lib = rec.lib
        lv = Y.levels_desc(levels)
        ws = torch.empty(lib.ld_scale_levels_backward_workspace_bytes(
            ctypes.byref(lv)), dtype=torch.uint8, device=dev)
        dx2 = torch.full((N, C, P), float('nan'), device=dev)
        acc = _d(d0)
        L.check(lib.ld_scale_levels_backward(
            ctypes.byref(lv), L.ptr(god), L.ptr(xd.detach()), L.ptr(sd.detach()),
            N * C, L.ptr(dx2), L.ptr(acc), 1, L.ptr(ws), ws.numel(),
            L.stream_ptr(dev)), 'ld_scale_levels_backward')
    torch.cuda.synchronize()
    entries = rec.expect('scale', *CASES['scale'])
    worst = {'y': R.check(y, *R.scale_levels(x, s, levels), 'y')}
    (dx, S_dx), (ds, S_ds) = R.scale_levels_backward(dy, x, s, levels)
    worst['dx'] = R.check(xd.grad, dx, S_dx, 'dx')
    worst['dx abi'] = R.check(dx2, dx, S_dx, 'dx (abi)')
    worst['dscale'] = R.check(sd.grad, ds, S_ds, 'dscale')
    _, (dsa, Sa) = R.scale_levels_backward(dy, x, s, levels, d0)
    worst['dscale accumulated'] = R.check(acc, dsa, Sa, 'dscale accumulated')
    _report('scale_levels', (name, N, C), entries, worst)


# ----------------------------------------------------------------- closing --
def test_every_export_has_a_checked_case():
    declared = {n for names in CASES.values() for n in names}
    exports = set(_exports())
    assert not declared - exports, sorted(declared - exports)
    assert not set(UNREACHED) & declared
    missing = exports - declared - set(UNREACHED)
    assert not missing, f'no checked case reaches {sorted(missing)}'
    print('\nworst |got - ref| / (u S) per entry point:')
    for name in sorted(WORST_SEEN):
        print(f'  {name:34s} {WORST_SEEN[name]:.2f}')
