"""tests/_norm_ref64.py on the CPU: the references agree with torch float64
autograd, a correct fp32 kernel stays inside the bars, planted kernel defects
break them, and ``settle`` leaves no undecidable ReLU cell in any case of the
matrix."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _norm_ref64 as R

REL = 1e-12
E32 = R.eps32(R.EPS)


def _t(a, grad=False):
    return torch.from_numpy(np.asarray(a, dtype=np.float64).copy()
                            ).requires_grad_(grad)


def _agree(ref, t, what):
    t = t.detach().numpy()
    scale = max(float(np.abs(t).max()), 1e-300)
    err = float(np.abs(np.asarray(ref).reshape(t.shape) - t).max())
    assert err <= REL * scale, (what, err / scale)


def _gn_fp32_keys():
    return sorted({c[:4] for c in R.gn_fp32_cases()})


# ------------------------------------------------ 1. reference correctness --
@pytest.mark.parametrize('shape', R.BN_SHAPES, ids=str)
@pytest.mark.parametrize('relu,with_res', R.BN_FLAGS)
def test_bn_reference_agrees_with_autograd(shape, relu, with_res):
    N, C, P = shape
    d = R.bn_inputs(N, C, P, relu, with_res)
    x, g, b = (_t(d[k], True) for k in ('x', 'gamma', 'beta'))
    res = _t(d['res'], True) if with_res else None
    y = F.batch_norm(x, _t(d['mean']), _t(d['var']), g, b, False, 0.0, E32)
    if with_res:
        y = y + res
    if relu:
        y = F.relu(y)
    y.backward(_t(d['dy']))
    f = R.bn_forward(d['x'], d['gamma'], d['beta'], d['mean'], d['var'], R.EPS,
                     d['res'], relu)
    bw = R.bn_backward(d['dy'], d['x'], f['pre'] > 0 if relu else None,
                       d['gamma'], d['mean'], d['var'], R.EPS)
    _agree(f['y'], y, 'y')
    _agree(bw['dx'][0], x.grad, 'dx')
    _agree(bw['dgamma'][0], g.grad, 'dgamma')
    _agree(bw['dbeta'][0], b.grad, 'dbeta')
    if with_res:
        _agree(bw['dres'][0], res.grad, 'dres')


@pytest.mark.parametrize('key', _gn_fp32_keys(), ids=str)
@pytest.mark.parametrize('relu', [True, False])
def test_gn_reference_agrees_with_autograd(key, relu):
    name, N, C, G = key
    d = R.gn_inputs(name, N, C, G, relu)
    levels = d['levels']
    x, g, b = (_t(d[k], True) for k in ('x', 'gamma', 'beta'))
    outs, off = [], R.offsets(levels)
    for l, (h, w) in enumerate(levels):
        xl = x[:, :, off[l]:off[l + 1]].reshape(N, C, h, w)
        o = F.group_norm(xl, G, g, b, E32)
        outs.append((F.relu(o) if relu else o).flatten(2))
    y = torch.cat(outs, 2)
    y.backward(_t(d['dy']))
    f = R.gn_forward(d['x'], d['gamma'], d['beta'], G, R.EPS, levels, relu)
    bw = R.gn_backward(d['dy'], d['x'], f['pre'] > 0 if relu else None,
                       d['gamma'], G, levels, f)
    _agree(f['y'], y, 'y')
    _agree(bw['dx'][0], x.grad, 'dx')
    _agree(bw['dgamma'][0], g.grad, 'dgamma')
    _agree(bw['dbeta'][0], b.grad, 'dbeta')
    # the statistics, against their definition
    xt = x.detach()
    for l in range(len(levels)):
        xl = xt[:, :, off[l]:off[l + 1]].reshape(N, G, -1)
        _agree(f['mean'][:, :, l], xl.mean(2), 'mean')
        _agree(f['rstd'][:, :, l],
               1 / torch.sqrt(xl.var(2, unbiased=False) + E32), 'rstd')


@pytest.mark.parametrize('shape', R.POOL_VEC + R.POOL_SCALAR, ids=str)
def test_maxpool_reference_agrees_with_torch(shape):
    x = R._randn(R._rng('pool', shape), *shape)
    ref = F.max_pool2d(torch.from_numpy(x)[None], 3, 2, 1)[0].numpy()
    R.check_exact(R.maxpool3x3s2(x), ref, 'maxpool')


@pytest.mark.parametrize('fine,coarse', R.UPSAMPLE, ids=str)
def test_upsample_reference_agrees_with_autograd(fine, coarse):
    rng = R._rng('up', fine, coarse)
    a, b = R._randn(rng, 2, 3, *fine), R._randn(rng, 2, 3, *coarse)
    go, add = R._randn(rng, 2, 3, *fine), R._randn(rng, 2, 3, *coarse)
    at, bt = _t(a, True), _t(b, True)
    y = at + F.interpolate(bt, size=fine, mode='nearest')
    y.backward(_t(go))
    _agree(R.upsample_add(a, b)[0], y, 'fwd')
    dfine, dc, _ = R.upsample_add_backward(go, coarse)
    _agree(dfine, at.grad, 'd fine')
    _agree(dc, bt.grad, 'd coarse')
    _agree(R.upsample_add_backward(go, coarse, add)[1],
           bt.grad + _t(add), 'd coarse + addend')


def test_scale_bias_pack_references_agree_with_autograd():
    levels = R.PYRAMIDS['A8']
    rng = R._rng('scale')
    x, dy = R._randn(rng, 2, 68, 381), R._randn(rng, 2, 68, 381)
    s, d0 = R._randn(rng, 8), R._randn(rng, 8)
    xt, st = _t(x, True), _t(s, True)
    sc = torch.cat([st[i].expand(h * w) for i, (h, w) in enumerate(levels)])
    y = xt * sc
    y.backward(_t(dy))
    _agree(R.scale_levels(x, s, levels)[0], y, 'scale fwd')
    (dx, _), (ds, _) = R.scale_levels_backward(dy, x, s, levels)
    _agree(dx, xt.grad, 'scale dx')
    _agree(ds, st.grad, 'dscale')
    _agree(R.scale_levels_backward(dy, x, s, levels, d0)[1][0],
           st.grad + _t(d0), 'dscale accumulated')
    _agree(R.bias_grad(dy)[0], _t(dy).sum((0, 2)), 'bias grad')
    feats = R.unpack_levels(x, levels)
    assert [f.shape[2:] for f in feats] == [tuple(l) for l in levels]
    R.check_exact(R.pack_levels(feats), x, 'pack(unpack)')
    R.check_exact(R.pack_levels(feats),
                  torch.cat([torch.from_numpy(f).flatten(2) for f in feats],
                            2).numpy(), 'pack vs cat')


def test_bf16_rounding_is_nearest_even():
    x = np.concatenate([R._randn(R._rng('bf16'), 4096) * 3,
                        np.array([1.00390625, 1.01171875, -1.00390625, 0.0,
                                  3.0e-39], dtype=np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    R.check_exact(R.bf16_rne(x), want, 'rne')
    assert (R.bf16_rne(x) != R.bf16_rtz(x)).any()
    img = np.arange(2 * 16 * 5, dtype=np.float32).reshape(2, 16, 5)
    flat = img.reshape(2, 2, 8, 5).transpose(0, 1, 3, 2).ravel()
    R.check_exact(R.c8_to_ncp(flat, (2, 16, 5)), img, 'C8 layout')


# ---------------------------------------------- 2. a correct kernel passes --
def _f(a):
    return np.asarray(a, dtype=np.float32)


def _gn_kernel_fp32(d, G, levels, relu):
    """The device's sequence of fp32 operations for GroupNorm forward and dx
    (statistics in fp64, stored as fp32; sums in fp64)."""
    x, ga, be, dy = (_f(d[k]) for k in ('x', 'gamma', 'beta', 'dy'))
    n, c, p = x.shape
    cpg, off, L = c // G, R.offsets(levels), len(levels)
    mean, rstd = np.empty((n, G, L), np.float32), np.empty((n, G, L), np.float32)
    for l in range(L):
        xl = x[:, :, off[l]:off[l + 1]].astype(np.float64).reshape(n, G, -1)
        m = xl.sum(2) / xl.shape[2]
        var = np.maximum((xl * xl).sum(2) / xl.shape[2] - m * m, 0)
        mean[:, :, l], rstd[:, :, l] = m, 1 / np.sqrt(var + np.float64(_f(R.EPS)))
    mu = _f(R._per_level(mean, levels, x.shape))
    rs = _f(R._per_level(rstd, levels, x.shape))
    xh = (x - mu) * rs
    y = xh * ga[None, :, None] + be[None, :, None]
    dz = np.where(y > 0, dy, np.float32(0)) if relu else dy
    if relu:
        y = np.maximum(y, np.float32(0))
    t = (dz * xh).astype(np.float64)
    g64 = ga.astype(np.float64)[None, :, None]
    m1, m2 = np.empty((n, G, L), np.float32), np.empty((n, G, L), np.float32)
    for l in range(L):
        sl = slice(off[l], off[l + 1])
        cnt = cpg * (off[l + 1] - off[l])
        m1[:, :, l] = (g64 * dz)[:, :, sl].reshape(n, G, -1).sum(2) / cnt
        m2[:, :, l] = (g64 * t)[:, :, sl].reshape(n, G, -1).sum(2) / cnt
    f1 = _f(R._per_level(m1, levels, x.shape))
    f2 = _f(R._per_level(m2, levels, x.shape))
    dx = rs * (ga[None, :, None] * dz - f1 - xh * f2)
    return dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=_f(t.sum((0, 2))),
                dbeta=_f(dz.astype(np.float64).sum((0, 2))))


@pytest.mark.parametrize('case', [('A', 2, 64, 32, True, ''),
                                  ('A8', 2, 48, 12, True, ''),
                                  ('C', 2, 32, 32, False, ''),
                                  ('A', 2, 64, 32, True, 'shift256')], ids=str)
def test_fp32_groupnorm_arithmetic_passes(case):
    name, N, C, G, relu, variant = case
    d = R.gn_inputs(*case)
    levels = d['levels']
    k = _gn_kernel_fp32(d, G, levels, relu)
    f = R.gn_forward(d['x'], d['gamma'], d['beta'], G, R.EPS, levels, relu)
    bw = R.gn_backward(d['dy'], d['x'], f['pre'] > 0 if relu else None,
                       d['gamma'], G, levels, f)
    R.check(k['y'], f['y'], f['S'], 'y')
    R.check(k['mean'], f['mean'], f['S_mean'], 'mean')
    R.check(k['rstd'], f['rstd'], f['rstd'], 'rstd', bar=f['bar_rstd'])
    for key in ('dx', 'dgamma', 'dbeta'):
        R.check(k[key], *bw[key], key)
    # and the reference itself, rounded to fp32 and to an image
    R.check(_f(f['y']), f['y'], f['S'], 'rounded y')
    R.check_image_alone(R.bf16_rne(_f(f['y'])), f['y'], f['S'], 'image of y')
    R.check_image_of(R.bf16_rne(k['y']), k['y'], 'image beside y')


@pytest.mark.parametrize('shape', R.BN_SHAPES, ids=str)
@pytest.mark.parametrize('relu,with_res', R.BN_FLAGS)
def test_fp32_bn_arithmetic_passes(shape, relu, with_res):
    d = R.bn_inputs(*shape, relu, with_res)
    x, ga, be, mu, var, dy = (_f(d[k]) for k in ('x', 'gamma', 'beta', 'mean',
                                                 'var', 'dy'))
    rstd = np.float32(1) / np.sqrt(var + _f(R.EPS))
    s = ga * rstd
    sh = be - mu * s
    y = x * s[None, :, None] + sh[None, :, None]
    if with_res:
        y = y + _f(d['res'])
    dz = np.where(y > 0, dy, np.float32(0)) if relu else dy
    if relu:
        y = np.maximum(y, np.float32(0))
    dx = dz * s[None, :, None]
    t = dz * ((x - mu[None, :, None]) * rstd[None, :, None])
    f = R.bn_forward(x, ga, be, mu, var, R.EPS, d['res'], relu)
    bw = R.bn_backward(dy, x, f['pre'] > 0 if relu else None, ga, mu, var, R.EPS)
    R.check(y, f['y'], f['S'], 'y')
    R.check(dx, *bw['dx'], 'dx')
    R.check_exact(dz, _f(bw['dres'][0]), 'dres')
    R.check(_f(t.astype(np.float64).sum((0, 2))), *bw['dgamma'], 'dgamma')
    R.check(_f(dz.astype(np.float64).sum((0, 2))), *bw['dbeta'], 'dbeta')
    # the C8-input form: dgamma from the rounded x, judged against the same
    xr = R.bf16_rne(x)
    tr = dz * ((xr - mu[None, :, None]) * rstd[None, :, None])
    br = R.bn_backward(dy, xr, f['pre'] > 0 if relu else None, ga, mu, var, R.EPS)
    R.check(_f(tr.astype(np.float64).sum((0, 2))), *br['dgamma'], 'dgamma c8in')


# ------------------------------------------------------ 3. planted defects --
def _breaks(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


def test_defect_previous_levels_statistics_after_a_boundary():
    d = R.gn_inputs('A', 2, 64, 32, False)
    levels = d['levels']
    f = R.gn_forward(d['x'], d['gamma'], d['beta'], 32, R.EPS, levels)
    y = f['y'].copy()
    R.check(_f(y), f['y'], f['S'], 'correct')
    x = R.f64(d['x'])
    mu = R._per_level(f['mean'], levels, x.shape)
    rs = R._per_level(f['rstd'], levels, x.shape)
    for o in R.offsets(levels)[1:-1]:  # first cell of levels 1..: wrong table
        y[:, :, o] = ((x[:, :, o] - mu[:, :, o - 1]) * rs[:, :, o - 1] *
                      R.f64(d['gamma'])[None, :] + R.f64(d['beta'])[None, :])
    _breaks(R.check, _f(y), f['y'], f['S'], 'wrong level table')


def test_defect_last_stats_slice_missing():
    d = R.gn_inputs('C', 2, 64, 32, False)
    levels = d['levels']
    assert levels[0][0] * levels[0][1] == 2050
    f = R.gn_forward(d['x'], d['gamma'], d['beta'], 32, R.EPS, levels)
    cells = [h * w for h, w in levels]
    whole = R.gn_stats(d['x'], 32, R.EPS, levels, cells=cells)  # one-pass, all
    R.check(_f(whole['mean']), f['mean'], f['S_mean'], 'mean')
    R.check(_f(whole['rstd']), f['rstd'], f['rstd'], 'rstd', bar=f['bar_rstd'])
    cells[0] = 2048  # the third slice (2 cells) never summed
    bad = R.gn_stats(d['x'], 32, R.EPS, levels, cells=cells)
    _breaks(R.check, _f(bad['mean']), f['mean'], f['S_mean'], 'mean')
    _breaks(R.check, _f(bad['rstd']), f['rstd'], f['rstd'], 'rstd',
            bar=f['bar_rstd'])
    yb = R.gn_forward(d['x'], d['gamma'], d['beta'], 32, R.EPS, levels,
                      stats=bad)['y']
    _breaks(R.check, _f(yb), f['y'], f['S'], 'y')


def test_defect_float4_group_missing_from_dgamma():
    d = R.gn_inputs('E', 1, 16, 4, False)  # the longest sum: 32776 terms
    levels = d['levels']
    f = R.gn_forward(d['x'], d['gamma'], d['beta'], 4, R.EPS, levels)
    good = R.gn_backward(d['dy'], d['x'], None, d['gamma'], 4, levels, f)
    R.check(_f(good['dgamma'][0]), *good['dgamma'], 'dgamma')
    bad = R.gn_backward(d['dy'], d['x'], None, d['gamma'], 4, levels, f,
                        drop=(0, 5, 1024))
    _breaks(R.check, _f(bad['dgamma'][0]), *good['dgamma'], 'dgamma')
    # the same sum feeds the group mean m2 every dx of the group uses: the dx
    # bar (the magnitudes of the means' terms, not |m1|, |m2|) stays sharp
    R.check(_f(good['dx'][0]), *good['dx'], 'dx')
    _breaks(R.check, _f(bad['dx'][0]), *good['dx'], 'dx')


def test_defect_split_slot_dropped_in_finalise():
    N, C, P = 3, 8, 1500  # two splits; slice 0 ends inside image 1
    d = R.bn_inputs(N, C, P, False, False)
    good = R.bn_backward(d['dy'], d['x'], None, d['gamma'], d['mean'], d['var'],
                         R.EPS)
    per = ((N * P + 1) // 2 + 3) // 4 * 4  # float4-aligned slices
    dy0 = R.f64(d['dy']).transpose(1, 0, 2).reshape(C, N * P).copy()
    dy0[:, per:] = 0.0  # slot 1 never added
    dy0 = dy0.reshape(C, N, P).transpose(1, 0, 2)
    bad = R.bn_backward(dy0, d['x'], None, d['gamma'], d['mean'], d['var'], R.EPS)
    for key in ('dgamma', 'dbeta'):
        R.check(_f(good[key][0]), *good[key], key)
        _breaks(R.check, _f(bad[key][0]), *good[key], key)
    db, S = R.bias_grad(d['dy'])
    _breaks(R.check, _f(R.bias_grad(dy0)[0]), db, S, 'bias grad')


def test_defect_image_rounded_toward_zero():
    d = R.bn_inputs(2, 40, 252, True, True)
    f = R.bn_forward(d['x'], d['gamma'], d['beta'], d['mean'], d['var'], R.EPS,
                     d['res'], True)
    y = _f(f['y'])
    R.check_image_of(R.bf16_rne(y), y, 'rne')
    R.check_image_alone(R.bf16_rne(y), f['y'], f['S'], 'rne alone')
    _breaks(R.check_image_of, R.bf16_rtz(y), y, 'rtz')
    _breaks(R.check_image_alone, R.bf16_rtz(y), f['y'], f['S'], 'rtz alone')


def test_defect_maxpool_zero_padding_on_negative_map():
    x = -np.abs(R._randn(R._rng('poolneg'), 5, 7, 12)) - np.float32(0.5)
    ref = R.maxpool3x3s2(x)
    assert (ref < 0).all()
    _breaks(R.check_exact, R.maxpool3x3s2(x, pad_value=0.0), ref, 'zero padding')


def test_defect_nearest_index_off_by_one():
    fine, coarse = (13, 21), (7, 11)  # 2c - 1
    rng = R._rng('up', fine, coarse)
    a, b = R._randn(rng, 2, 3, *fine), R._randn(rng, 2, 3, *coarse)
    ref, S = R.upsample_add(a, b)
    R.check(_f(ref), ref, S, 'correct')
    _breaks(R.check, _f(R.upsample_add(a, b, shift=1)[0]), ref, S, 'index + 1')
    # rounding instead of flooring the source coordinate
    hi = np.clip(np.rint(np.arange(13) * 7 / 13).astype(int), 0, 6)
    wi = np.clip(np.rint(np.arange(21) * 11 / 21).astype(int), 0, 10)
    wrong = R.f64(a) + R.f64(b)[..., hi[:, None], wi[None, :]]
    _breaks(R.check, _f(wrong), ref, S, 'rounded index')


def test_defect_addend_not_added():
    fine, coarse = (13, 21), (7, 11)
    rng = R._rng('upadd')
    go, add = R._randn(rng, 2, 3, *fine), R._randn(rng, 2, 3, *coarse)
    _, ref, S = R.upsample_add_backward(go, coarse, add)
    R.check(_f(ref), ref, S, 'correct')
    _breaks(R.check, _f(R.upsample_add_backward(go, coarse)[1]), ref, S,
            'no addend')


# ----------------------------------------------------- 4. input conditions --
def _few(rounds):
    assert rounds <= 4, rounds


@pytest.mark.parametrize('case', [c for c in R.gn_fp32_cases() if c[4]] +
                         [c + ('', ) for c in R.GN_BF16_CASES if c[4]], ids=str)
def test_settle_leaves_no_undecidable_gn_cell(case):
    name, N, C, G, relu, variant = case
    d = R.gn_inputs(*case)
    _few(d['rounds'])
    f = R.gn_forward(d['x'], d['gamma'], d['beta'], G, R.EPS, d['levels'])
    assert R.undecided(f['pre'], f['S']) == 0


BN_SETTLE = [s + (True, wr, '') for s in R.BN_SHAPES + R.BN_BF16_SHAPES
             for wr in (True, False)] + \
    [(2, 32, p, True, False, 'c8in') for p in R.BN_C8IN_P]


@pytest.mark.parametrize('args', BN_SETTLE, ids=str)
def test_settle_leaves_no_undecidable_bn_cell(args):
    d = R.bn_inputs(*args)
    _few(d['rounds'])
    f = R.bn_forward(d['x'], d['gamma'], d['beta'], d['mean'], d['var'], R.EPS,
                     d['res'])
    assert R.undecided(f['pre'], f['S']) == 0


def test_settle_moves_only_offending_cells_and_is_deterministic():
    rng = R._rng('settle')
    x = R._randn(rng, 2, 8, 64)
    x[0, 0, :4] = 0.0  # exactly on the threshold of y = x
    ev = lambda v: (v.astype(np.float64), np.abs(v.astype(np.float64)) + 1e-3)
    a, ra = R.settle(x, ev, seed=3)
    b, rb = R.settle(x, ev, seed=3)
    assert ra == rb >= 1 and np.array_equal(a, b)
    moved = a != x
    assert moved[0, 0, :4].all() and moved.sum() < 16
    assert R.undecided(*ev(a)) == 0


# ------------------------------------- why two bars differ from a first guess --
def test_dx_bar_needs_the_magnitudes_of_the_group_means_terms():
    """With |m1|, |m2| in S a correct fp32 kernel breaks the bar: a group mean
    cancels to ~1 / sqrt(count) of its terms while its fp32 error stays
    relative to the terms."""
    case = ('A', 2, 64, 32, True, '')
    d = R.gn_inputs(*case)
    k = _gn_kernel_fp32(d, 32, d['levels'], True)
    f = R.gn_forward(d['x'], d['gamma'], d['beta'], 32, R.EPS, d['levels'], True)
    bw = R.gn_backward(d['dy'], d['x'], f['pre'] > 0, d['gamma'], 32, d['levels'],
                       f)
    R.check(k['dx'], *bw['dx'], 'dx')
    assert (bw['dx_literal_S'] <= bw['dx'][1] * (1 + 1e-12)).all()
    _breaks(R.check, k['dx'], bw['dx'][0], bw['dx_literal_S'], 'dx, |m1| |m2|')


def test_image_bar_is_half_an_ulp_of_the_reference():
    """2^-9 |ref| is half a bf16 ulp only at the top of a binade: the correctly
    rounded image of the reference itself exceeds it; hu(ref) holds and never
    exceeds 2^-8 |ref|."""
    ref = R.f64(R._randn(R._rng('image bar'), 4096))
    img = R.bf16_rne(ref)
    hu = R.half_ulp_bf16(ref)
    assert (np.abs(img - ref) <= hu).all()
    assert (hu <= 2.0 ** -8 * np.abs(ref)).all()
    assert (hu > 2.0 ** -9 * np.abs(ref) * (1 - 1e-12)).all()
    assert (np.abs(img - ref) > 2.0 ** -9 * np.abs(ref)).any()
    R.check_image_alone(img, ref, np.abs(ref), 'rne of the reference')
