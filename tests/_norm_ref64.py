"""Float64 restatements of the norm and glue operations of csrc/nn.hip, each
with a per-element error bar, plus the case matrix the host and the GPU test
share (host arithmetic only: numpy float64, no autograd, no device).

Layout: activations are (N, C, P) with the levels' (H, W) images concatenated
along P, as ld_amd.layers holds them.  Every reference takes the fp32 operands
the kernel consumes (for a C8-input form: the RNE-rounded bf16 values) and
returns, beside each value,

  S = the sum of the absolute values of the terms of its expression at the
      finest granularity (|x s| + |mean s| + |beta| + |res| for the BN
      forward, sum |dz xhat| for a reduction, ...).

Bars (one constant, the conv helper's argument, tests/_conv_ref64.py):

  fp32 result            |got - ref| <= 16 u S,  u = 2^-24
  GN rstd                relative 16 u + 2^-52 (q/n) / (var + eps): the device
                         forms q/n - m^2 in fp64, the second term is the
                         cancellation of that subtraction (offset-mean case)
  image beside fp32      image == RNE_bf16(that output), exactly
  image alone            |img - ref| <= hu(ref) + 16 u S, hu = half the bf16
                         spacing at ref, 2^(floor(log2 |ref|) - 8): between
                         2^-9 |ref| and 2^-8 |ref|.  (2^-9 |ref| alone is half
                         an ulp only at the top of a binade: the correctly
                         rounded image of the reference itself misses it on
                         one cell in seven.)
  copies, max, d(fine)   equality

fp32 roundings per path (each is at most u times the term it touches, so their
sum is a multiple of u S; all fit under 16):
  BN forward    scale = gamma * (1 / sqrt(var + eps)): 4 (add, sqrt, divide,
                multiply), carried by |x s| and |mean s|; shift = beta - mean s:
                2; x s + shift: 2 (1 when contracted); + res: 1.        <= 9
  BN dx         scale 4, dz * s 1.                                      <= 5
  BN dgamma     rstd 3; per term x - mean, * rstd, * dz: 3 (the sum itself is
                fp64 on the device), the final fp32 store 1.            <= 7
  BN dbeta / bias gradient / dscale  fp64 sums of fp32 terms (dscale: one
                fp32 product per term), one final rounding.             <= 2
  GN forward    mean and rstd stored as fp32: 1 each; x - mean, * rstd: 2; the
                fma with gamma, beta: 1.                                <= 5
  GN dx         rstd (m1 + xhat m2 - gamma dz) with the group means m1 =
                mean(gamma dz), m2 = mean(gamma dz xhat).  The means are sums
                themselves, so at the finest granularity their terms count:
                S = rstd (|gamma dz| + M1 + (|x| + |mu|) rstd M2) with M1, M2
                the means of |gamma dz| and |gamma dz| (|x| + |mu|) rstd.  (With
                |m1|, |m2| in their place a correct kernel fails: the fp32
                error of a group mean is relative to its terms, not to the
                mean, which cancels to 1 / sqrt(count) of them -- the host
                test's fp32 restatement of the device's operations reached
                65 u S that way.)  Roundings: mean, rstd 2; xhat 2; per term
                of m2 3 more; m1, m2 stored as fp32 2; gamma dz, the two
                subtractions, xhat m2, * rstd 5.                        <= 14
  GN dgamma     as BN dgamma with the fp32 mean / rstd.                 <= 6
  upsample-add  forward 1; d(coarse): at most 9 fine cells per coarse cell
                (+ the addend) summed in fp32.                          <= 9
  scale         one product.                                            1
Every reduction here has fewer than 2^20 terms, so a dropped term of average
size S / K exceeds 16 u S = S / 2^20: the bar is sharp (test_norm_ref64_host.py
plants such defects and requires them to break it).

ReLU mask.  The reference takes the mask from its own float64 y.  A cell with
|y_ref| <= 16 u S_y cannot be decided (a correct kernel may land on either
side), so a case may hold none: ``settle`` moves such cells of x by a fixed
step and re-evaluates until none are left, and the tests assert the count is
zero on the reference alone.
"""
import functools

import numpy as np

U = 2.0 ** -24
BAR = 16.0

# ------------------------------------------------------------- the matrix --
# Offsets are in cells.  A8 / A8v: the fourth level is (1, 3) so that P is 381
# (odd: scalar kernels) / 384 (P % 4 == 0: vector kernels) with LD_MAX_LEVELS
# = 8 levels, and one thread's four cells span three or more levels.
_A3 = ((13, 21), (7, 11), (4, 6))
PYRAMIDS = {
    # P % 4 == 0; boundaries at 273, 350, 374 fall inside a thread's 4 cells
    'A': _A3 + ((2, 3), ),
    'A8': _A3 + ((1, 3), (1, 1), (1, 1), (1, 1), (1, 1)),
    'A8v': _A3 + ((1, 3), (1, 1), (1, 1), (1, 1), (1, 4)),
    'B': ((12, 20), (6, 10), (3, 5), (2, 3), (1, 2)),
    # level 0 has 2050 cells: three stats slices, the last of 2 cells
    'C': ((41, 50), (21, 25), (11, 13), (2, 1)),
    # scalar path; the sliced reduce has 5 empty slices that must write zeros
    'Codd': ((41, 50), (21, 25), (11, 13), (1, 1)),
    # slice length 1025: slices start off 16-byte boundaries
    'E': ((241, 136), ),
}
PYRAMID_P = dict(A=380, A8=381, A8v=384, B=323, C=2720, Codd=2719, E=32776)

GN_CG = ((64, 32), (64, 16), (48, 12), (64, 4), (32, 32))
# E runs with C = 16, N = 1: the same channels per group (2, 4, 16, 1)
GN_CG_E = ((16, 8), (16, 4), (16, 1), (16, 16))


def gn_fp32_cases():
    """(pyramid, N, C, G, relu, variant); variant '' | 'offset' | 'shift256'."""
    out = []
    for name in ('A', 'A8', 'A8v', 'B', 'C', 'Codd', 'E'):
        for c, g in (GN_CG_E if name == 'E' else GN_CG):
            for relu in (True, False):
                out.append((name, 1 if name == 'E' else 2, c, g, relu, ''))
    out.append(('A', 2, 64, 32, True, 'offset'))
    out.append(('A', 2, 64, 32, True, 'shift256'))
    return out


# bf16 mode: (64, 32) and (32, 32) reload the table per channel (!one_group),
# (256, 32) and (64, 4) share it (one_group: 8 / 16 channels per group)
GN_BF16_CASES = (
    ('A', 2, 64, 32, True), ('A', 2, 64, 32, False), ('A', 2, 256, 32, True),
    ('A', 2, 64, 4, True), ('A', 2, 32, 32, True),
    ('A8v', 2, 64, 32, True), ('A8v', 2, 64, 4, True),
    ('C', 2, 64, 32, True), ('C', 2, 64, 4, True),
    ('E', 1, 32, 32, True), ('E', 1, 32, 4, True),
)

BN_SHAPES = ((2, 40, 252), (2, 40, 253), (1, 24, 1028), (3, 8, 1500),
             (2, 20, 4100))
BN_FLAGS = ((True, True), (True, False), (False, False))  # (relu, residual)
BN_BF16_SHAPES = ((2, 64, 252), (1, 32, 1028), (2, 32, 32772))
BN_C8IN_P = (560, 54, 130)
BIAS_SHAPES = ((2, 68, 253), (3, 8, 1500), (2, 80, 4100))
POOL_VEC = ((6, 9, 8), (5, 7, 12), (3, 11, 20))
POOL_SCALAR = ((4, 9, 10), )
UPSAMPLE = (((14, 22), (7, 11)), ((13, 21), (7, 11)), ((7, 11), (7, 11)),
            ((2, 3), (1, 2)), ((1, 1), (1, 1)))
EPS = 1e-5


# ---------------------------------------------------------------- plumbing --
def f32(t):
    """t (numpy or a torch tensor on any device) as a float32 numpy array."""
    if t is None:
        return None
    if hasattr(t, 'detach'):
        t = t.detach().to('cpu').float().numpy()
    return np.ascontiguousarray(t, dtype=np.float32)


def f64(t):
    return None if t is None else f32(t).astype(np.float64)


def eps32(eps):
    """eps as the library receives it: a C float."""
    return float(np.float32(eps))


def offsets(levels):
    off = [0]
    for h, w in levels:
        off.append(off[-1] + h * w)
    return off


def bf16_rne(a):
    """fp32 values rounded to bf16, round to nearest even (as fp32)."""
    b = f32(a).view(np.uint32).astype(np.uint64)
    b = (b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000
    return b.astype(np.uint32).view(np.float32)


def bf16_rtz(a):
    """fp32 values truncated to bf16: the wrong rounding."""
    return (f32(a).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def c8_to_ncp(img, shape):
    """A C8 image (N, C/8, P, 8), flat, as an (N, C, P) array."""
    n, c, p = shape
    return np.ascontiguousarray(
        np.asarray(img).reshape(n, c // 8, p, 8).transpose(0, 1, 3, 2)
    ).reshape(n, c, p)


# -------------------------------------------------------------------- bars --
def bound(S):
    return BAR * U * np.asarray(S, dtype=np.float64)


def _fail(what, bad, got, ref, err, bar, ratio):
    i = np.unravel_index(int(np.flatnonzero(bad.ravel())[0]), bad.shape)
    raise AssertionError(
        f'{what}: {int(bad.sum())}/{bad.size} elements outside the bar; first '
        f'at {tuple(int(v) for v in i)}: got {got[i]:.9g} ref {ref[i]:.9g} '
        f'|err| {err[i]:.3g} > bar {bar[i]:.3g}; worst err/(uS) '
        f'{float(ratio.max()):.1f}')


def check(got, ref, S, what='', bar=None):
    """Assert |got - ref| <= bar (default 16 u S) on every element.  Returns
    the largest |got - ref| / (u S) (0 where the error is 0)."""
    got = f64(got).reshape(np.shape(ref))
    ref = np.asarray(ref, dtype=np.float64)
    S = np.broadcast_to(np.asarray(S, dtype=np.float64), ref.shape)
    bar = bound(S) if bar is None else np.broadcast_to(bar, ref.shape)
    err = np.abs(got - ref)
    ratio = np.where(err > 0, err / np.maximum(U * S, 1e-300), 0.0)
    bad = ~(err <= bar)
    if bad.any():
        _fail(what, bad, got, ref, err, bar, ratio)
    return float(ratio.max()) if ratio.size else 0.0


def check_exact(got, ref, what=''):
    got, ref = f32(got), f32(ref).reshape(np.shape(got))
    bad = got.view(np.uint32) != ref.view(np.uint32)
    # +0 / -0 are the same value
    bad &= ~((got == 0) & (ref == 0))
    if bad.any():
        i = np.unravel_index(int(np.flatnonzero(bad.ravel())[0]), bad.shape)
        raise AssertionError(
            f'{what}: {int(bad.sum())}/{bad.size} elements differ; first at '
            f'{tuple(int(v) for v in i)}: got {got[i]!r} expected {ref[i]!r}')
    return 0.0


def check_image_of(img, out, what=''):
    """A bf16 image written beside an fp32 output is its RNE conversion."""
    return check_exact(img, bf16_rne(out), what)


def half_ulp_bf16(ref):
    """Half the spacing of bf16 (8 significand bits) at each value of ref."""
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    _, e = np.frexp(ref)  # ref = m 2^e, m in [0.5, 1)
    return np.where(ref > 0, np.ldexp(1.0, e - 9), 0.0)


def check_image_alone(img, ref, S, what=''):
    """An image that is the only output: half a bf16 ulp of the reference on
    top of the fp32 bar.  Returns the worst (|err| - half ulp) / (u S)."""
    ref = np.asarray(ref, dtype=np.float64)
    img = f64(img).reshape(ref.shape)
    S = np.broadcast_to(np.asarray(S, dtype=np.float64), ref.shape)
    err = np.abs(img - ref)
    hu = half_ulp_bf16(ref)
    bar = hu + bound(S)
    ratio = np.maximum(err - hu, 0) / np.maximum(U * S, 1e-300)
    bad = ~(err <= bar)
    if bad.any():
        _fail(what, bad, img, ref, err, bar, ratio)
    return float(ratio.max()) if ratio.size else 0.0


def undecided(pre, S):
    """How many cells of a pre-activation cannot have their ReLU mask decided."""
    return int((np.abs(pre) <= bound(S)).sum())


SETTLE_STEP = 2.0 ** -8
SETTLE_ROUNDS = 8


def settle(x, evaluate, seed=0, step=SETTLE_STEP, max_rounds=SETTLE_ROUNDS):
    """x (fp32) with every cell whose ReLU mask ``evaluate(x) -> (pre, S)``
    cannot decide moved by ``step`` per round, in a direction drawn once per
    cell from ``seed``; stops when none is left.  Returns (x, rounds); raises
    when ``max_rounds`` do not suffice."""
    x = f32(x).copy()
    sign = np.where(np.random.default_rng(seed).integers(0, 2, x.shape) > 0,
                    np.float32(1), np.float32(-1))
    for rounds in range(max_rounds + 1):
        pre, S = evaluate(x)
        off = np.abs(pre) <= bound(S)
        if not off.any():
            return x, rounds
        x[off] = (x[off] + sign[off] * np.float32(step)).astype(np.float32)
    raise AssertionError(f'settle: {int(off.sum())} undecidable cells left '
                         f'after {max_rounds} rounds')


# ----------------------------------------------------------------- eval-BN --
def bn_coeffs(gamma, var, eps):
    rstd = 1.0 / np.sqrt(f64(var) + eps32(eps))
    return f64(gamma) * rstd, rstd


def bn_forward(x, gamma, beta, mean, var, eps, res=None, relu=False):
    """y = relu?(BN_eval(x) + res).  Returns dict(y, pre, S)."""
    x = f64(x)
    s, _ = bn_coeffs(gamma, var, eps)
    s, m, b = s[None, :, None], f64(mean)[None, :, None], f64(beta)[None, :, None]
    pre = x * s - m * s + b
    S = np.abs(x * s) + np.abs(m * s) + np.abs(b)
    if res is not None:
        pre = pre + f64(res)
        S = S + np.abs(f64(res))
    return dict(y=np.maximum(pre, 0.0) if relu else pre, pre=pre, S=S)


def bn_backward(dy, x, mask, gamma, mean, var, eps):
    """Backward of the above.  ``mask``: y > 0 (None without ReLU); ``x``: the
    BN input as the kernel reads it (the bf16-rounded values for the C8-input
    form).  Returns dict of (value, S) for dx, dres, dgamma, dbeta."""
    dz = f64(dy) if mask is None else f64(dy) * mask
    s, rstd = bn_coeffs(gamma, var, eps)
    dx = dz * s[None, :, None]
    out = dict(dx=(dx, np.abs(dx)), dres=(dz, np.abs(dz)),
               dbeta=(dz.sum((0, 2)), np.abs(dz).sum((0, 2))))
    if x is not None:
        x, m, r = f64(x), f64(mean)[None, :, None], rstd[None, :, None]
        out['dgamma'] = ((dz * (x - m) * r).sum((0, 2)),
                         (np.abs(dz) * (np.abs(x) + np.abs(m)) * r).sum((0, 2)))
    return out


# --------------------------------------------------------------- GroupNorm --
def _per_level(stat, levels, shape):
    """(N, G, L) statistics -> (N, C, P) (each group's value on its channels
    and its level's cells)."""
    n, c, p = shape
    g = stat.shape[1]
    out = np.empty((n, g, c // g, p))
    off = offsets(levels)
    for l in range(len(levels)):
        out[:, :, :, off[l]:off[l + 1]] = stat[:, :, l][:, :, None, None]
    return out.reshape(n, c, p)


def gn_stats(x, groups, eps, levels, cells=None):
    """mean, rstd per (n, group, level) and their bars.  ``cells`` (a planted
    defect): per level, how many leading cells the sums cover (the divisor
    stays the full count, as on the device)."""
    x = f64(x)
    n, c, _ = x.shape
    cpg = c // groups
    off = offsets(levels)
    L = len(levels)
    mean, rstd = np.empty((n, groups, L)), np.empty((n, groups, L))
    s_mean, rel_rstd = np.empty((n, groups, L)), np.empty((n, groups, L))
    e = eps32(eps)
    for l in range(L):
        a = off[l + 1] - off[l]
        xl = x[:, :, off[l]:off[l + 1]].reshape(n, groups, cpg, a)
        cnt = cpg * a
        if cells is not None:
            xl = xl[:, :, :, :cells[l]]
        m = xl.sum((2, 3)) / cnt
        if cells is None:
            var = ((xl - m[:, :, None, None]) ** 2).sum((2, 3)) / cnt
        else:
            var = np.maximum((xl ** 2).sum((2, 3)) / cnt - m * m, 0.0)
        q = (xl ** 2).sum((2, 3)) / cnt
        mean[:, :, l], rstd[:, :, l] = m, 1.0 / np.sqrt(var + e)
        s_mean[:, :, l] = np.abs(xl).sum((2, 3)) / cnt
        rel_rstd[:, :, l] = BAR * U + 2.0 ** -52 * q / (var + e)
    return dict(mean=mean, rstd=rstd, S_mean=s_mean, bar_rstd=rel_rstd * rstd)


def gn_forward(x, gamma, beta, groups, eps, levels, relu=False, stats=None):
    """GroupNorm (+ ReLU) per (n, group, level).  Returns dict(y, pre, S, mean,
    rstd, S_mean, bar_rstd)."""
    x = f64(x)
    st = gn_stats(x, groups, eps, levels) if stats is None else stats
    mu = _per_level(st['mean'], levels, x.shape)
    rs = _per_level(st['rstd'], levels, x.shape)
    ga, be = f64(gamma)[None, :, None], f64(beta)[None, :, None]
    pre = (x - mu) * rs * ga + be
    S = (np.abs(x) + np.abs(mu)) * rs * np.abs(ga) + np.abs(be)
    out = dict(st)
    out.update(y=np.maximum(pre, 0.0) if relu else pre, pre=pre, S=S)
    return out


def gn_backward(dy, x, mask, gamma, groups, levels, stats, drop=None):
    """Backward of the above from the reference's own statistics.  ``drop``
    (a planted defect): (n, c, first cell) of four consecutive cells left out
    of that channel's dgamma sum.  Returns dict of (value, S) for dx, dgamma,
    dbeta."""
    x = f64(x)
    n, c, p = x.shape
    cpg = c // groups
    dz = f64(dy) if mask is None else f64(dy) * mask
    mu = _per_level(stats['mean'], levels, x.shape)
    rs = _per_level(stats['rstd'], levels, x.shape)
    ga = f64(gamma)[None, :, None]
    xh = (x - mu) * rs
    off = offsets(levels)
    L = len(levels)
    t = dz * xh
    S_t = np.abs(dz) * (np.abs(x) + np.abs(mu)) * rs
    if drop is not None:
        t = t.copy()
        t[drop[0], drop[1], drop[2]:drop[2] + 4] = 0.0
    # the group means m1, m2 and the means M1, M2 of their terms' magnitudes
    m1, m2, M1, M2 = (np.empty((n, groups, L)) for _ in range(4))
    for l in range(L):
        sl = slice(off[l], off[l + 1])
        cnt = cpg * (off[l + 1] - off[l])
        for dst, src in ((m1, ga * dz), (m2, ga * t), (M1, np.abs(ga * dz)),
                         (M2, np.abs(ga) * S_t)):
            dst[:, :, l] = src[:, :, sl].reshape(n, groups, -1).sum(2) / cnt
    m1, m2, M1, M2 = (_per_level(m, levels, x.shape) for m in (m1, m2, M1, M2))
    dx = rs * (ga * dz - m1 - xh * m2)
    S_dx = rs * (np.abs(ga * dz) + M1 + (np.abs(x) + np.abs(mu)) * rs * M2)
    S_lit = rs * (np.abs(ga * dz) + np.abs(m1) +
                  (np.abs(x) + np.abs(mu)) * rs * np.abs(m2))
    return dict(dx=(dx, S_dx), dgamma=(t.sum((0, 2)), S_t.sum((0, 2))),
                dbeta=(dz.sum((0, 2)), np.abs(dz).sum((0, 2))),
                dx_literal_S=S_lit)  # reported, never a bar


# -------------------------------------------------------------------- glue --
def bias_grad(dy):
    dy = f64(dy)
    return dy.sum((0, 2)), np.abs(dy).sum((0, 2))


def maxpool3x3s2(x, pad_value=-np.inf):
    """MaxPool2d(3, 2, 1) of (..., H, W); exact (fp32 in, fp32 out)."""
    x = f32(x)
    h, w = x.shape[-2:]
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    xp = np.full(x.shape[:-2] + (h + 2, w + 2), pad_value, dtype=np.float32)
    xp[..., 1:h + 1, 1:w + 1] = x
    out = np.full(x.shape[:-2] + (ho, wo), -np.inf, dtype=np.float32)
    for kh in range(3):
        for kw in range(3):
            out = np.maximum(out, xp[..., kh:kh + 2 * ho:2, kw:kw + 2 * wo:2])
    return out


def nearest_index(out_size, in_size, shift=0):
    """Source index of each destination cell, F.interpolate(mode='nearest'):
    min(floor(dst * in / out), in - 1).  ``shift``: a planted defect."""
    d = np.arange(out_size)
    return np.clip(d * in_size // out_size + shift, 0, in_size - 1)


def upsample_add(fine, coarse, shift=0):
    """fine + nearest_up(coarse) on (..., H, W) maps: (value, S)."""
    fine, coarse = f64(fine), f64(coarse)
    hi = nearest_index(fine.shape[-2], coarse.shape[-2], shift)
    wi = nearest_index(fine.shape[-1], coarse.shape[-1], shift)
    up = coarse[..., hi[:, None], wi[None, :]]
    return fine + up, np.abs(fine) + np.abs(up)


def upsample_add_backward(dout, coarse_hw, addend=None):
    """d(fine) (= dout, exact) and d(coarse) (+ addend) with its S."""
    dout = f64(dout)
    hc, wc = coarse_hw
    hi = nearest_index(dout.shape[-2], hc)
    wi = nearest_index(dout.shape[-1], wc)
    lead = dout.shape[:-2]
    dc, S = np.zeros(lead + (hc, wc)), np.zeros(lead + (hc, wc))
    flat = (hi[:, None] * wc + wi[None, :]).ravel()
    d2 = dout.reshape(-1, dout.shape[-2] * dout.shape[-1])
    for dst, src in ((dc, d2), (S, np.abs(d2))):
        v = dst.reshape(-1, hc * wc)
        for r in range(v.shape[0]):
            v[r] = np.bincount(flat, weights=src[r], minlength=hc * wc)
    if addend is not None:
        dc, S = dc + f64(addend), S + np.abs(f64(addend))
    return dout, dc, S


def pack_levels(feats):
    """Per-level (N, C, H, W) maps -> (N, C, P): a copy."""
    return np.concatenate(
        [f32(f).reshape(f.shape[0], f.shape[1], -1) for f in feats], axis=2)


def unpack_levels(x3, levels):
    x3 = f32(x3)
    off = offsets(levels)
    return [x3[:, :, off[l]:off[l + 1]].reshape(x3.shape[0], x3.shape[1], h, w)
            for l, (h, w) in enumerate(levels)]


def scale_levels(x, scales, levels):
    """y = x * scales[level]: (value, S)."""
    x = f64(x)
    s = np.repeat(f64(scales), [h * w for h, w in levels])[None, None, :]
    return x * s, np.abs(x * s)


def scale_levels_backward(dy, x, scales, levels, dscale0=None):
    """dx, dscale (+ dscale0 when accumulating), each with S."""
    dy, x = f64(dy), f64(x)
    dx, S_dx = scale_levels(dy, scales, levels)
    off = offsets(levels)
    t = dy * x
    ds = np.array([t[:, :, off[l]:off[l + 1]].sum() for l in range(len(levels))])
    S = np.array([np.abs(t[:, :, off[l]:off[l + 1]]).sum()
                  for l in range(len(levels))])
    if dscale0 is not None:
        ds, S = ds + f64(dscale0), S + np.abs(f64(dscale0))
    return (dx, S_dx), (ds, S)


# ------------------------------------------------------------ case inputs --
def _rng(*key):
    return np.random.default_rng(_stable_seed(key))


def _stable_seed(key):
    s = 0
    for ch in repr(key):
        s = (s * 131 + ord(ch)) % (2 ** 32)
    return s


def _randn(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def gn_inputs(name, N, C, G, relu, variant=''):
    """Seeded operands of a GroupNorm case: dict(x, gamma, beta, dy, levels,
    rounds).  x is settled (ReLU cases); gamma from randn, so both signs.
    The arrays are shared between tests: do not write to them."""
    levels = PYRAMIDS[name]
    P = PYRAMID_P[name]
    rng = _rng('gn', name, N, C, G, variant)
    x = _randn(rng, N, C, P) * np.float32(2) + np.float32(0.5)
    if variant == 'shift256':
        x = _randn(rng, N, C, P) + np.float32(256)
    gamma, beta = _randn(rng, C), _randn(rng, C)
    dy = _randn(rng, N, C, P)
    rounds = 0
    if relu:
        def ev(xx):
            r = gn_forward(xx, gamma, beta, G, EPS, levels)
            return r['pre'], r['S']
        x, rounds = settle(x, ev, seed=_stable_seed(('gn', name, C, G)))
    for a in (x, gamma, beta, dy):
        a.setflags(write=False)
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, levels=levels,
                rounds=rounds)


@functools.lru_cache(maxsize=None)
def bn_inputs(N, C, P, relu, with_res, tag=''):
    """Seeded operands of an eval-BN case: dict(x, res, gamma, beta, mean,
    var, dy, rounds); x settled for ReLU cases."""
    rng = _rng('bn', N, C, P, with_res, tag)
    x = _randn(rng, N, C, P)
    res = _randn(rng, N, C, P) if with_res else None
    gamma, beta, mean = _randn(rng, C), _randn(rng, C), _randn(rng, C)
    var = (rng.random(C) + 0.5).astype(np.float32)
    dy = _randn(rng, N, C, P)
    rounds = 0
    if relu:
        def ev(xx):
            r = bn_forward(xx, gamma, beta, mean, var, EPS, res)
            return r['pre'], r['S']
        x, rounds = settle(x, ev, seed=_stable_seed(('bn', N, C, P)))
    for a in (x, res, gamma, beta, mean, var, dy):
        if a is not None:
            a.setflags(write=False)
    return dict(x=x, res=res, gamma=gamma, beta=beta, mean=mean, var=var,
                dy=dy, rounds=rounds)
