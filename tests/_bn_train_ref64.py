"""Float64 restatements of training-mode BatchNorm2d (+ residual) (+ ReLU) as
csrc/nn.hip's ld_bn_train_forward / ld_bn_train_backward compute it, each with
a per-element error bar, an fp32 restatement of the device's own operations
(for planting defects on the host), and the seeded cases the host and the GPU
test share.  Host arithmetic only: numpy, no autograd, no device.

Conventions are those of tests/_norm_ref64.py (imported, not restated): the
layout is (N, C, P) with M = N * P values per channel; every reference takes
the fp32 operands the kernel consumes and returns, beside each value,

  S = the sum of the absolute values of the terms of its expression at the
      finest granularity,

and the bar is |got - ref| <= 16 u S, u = 2^-24, for every fp32 result.

  y        x s - mean s + beta (+ res), s = gamma rstd:
           S = |x s| + |mean s| + |beta| (+ |res|)
  mean     sum x / M:  S = sum |x| / M
  rstd     relative 16 u + 2^-52 (q/M) / (var + eps), q = sum x^2: the device
           forms q/M - mean^2 in fp64, the second term is the cancellation of
           that subtraction (the GN statistics' bar)
  running_mean   (1 - m) r + m mean:  S = (1 - m) |r| + m sum |x| / M
  running_var    (1 - m) r + m var M/(M-1), var = q/M - mean^2:
                 S = (1 - m) |r| + m M/(M-1) (q/M + (sum |x| / M)^2)
  dbeta    sum dz:  S = sum |dz|
  dgamma   sum dz xhat, xhat = (x - mean) rstd:
           S = sum |dz| (|x| + |mean|) rstd
  dx       s (dz - mean(dz) - xhat mean(dz xhat)).  The means are sums
           themselves, so their terms count (the GN-dx entry):
           S = |s| (|dz| + mean|dz| + (|x| + |mean|) rstd
                                      mean(|dz| (|x| + |mean|) rstd))
  dres     = dz, exact

fp32 roundings per path (each at most u times a term of S; the sums themselves
are fp64 on the device):
  y        mean stored as fp32 1 (on |mean s|); rstd stored 1, gamma * rstd 1
           (on |x s| and |mean s|); mean * s, beta - that: 2; x * s, + shift:
           2 (1 when contracted); + res: 1.                            <= 8
           The cancellation term of rstd rides on |x s| + |mean s| <= S; the
           cases keep it below u (asserted on the reference: rstd_cancel).
  mean     the fp32 store.                                             1
  running_mean / running_var   formed in fp64 from the fp64 mean / variance
           and the fp32 buffer, one fp32 store per update (k updates: k; the
           fp64 cancellation of var is 2^-52 q/M, far below u S).      <= 3
  dbeta    fp64 sum of fp32 terms, one store (+ 1 when accumulating).  <= 2
  dgamma   mean 1, rstd 1; per term x - mean, * rstd, * dz: 3; the store 1
           (+ 1 when accumulating).                                    <= 7
  dx       s: 2; mean, rstd in xhat: 2; x - mean, * rstd: 2; per term of
           sum dz xhat 1 more (dz * xhat) and its mean stored as fp32 1;
           mean(dz) stored 1; dz - k1, xhat * k2, the second subtraction,
           * s: 4.                                                     <= 14
Every reduction here has fewer than 2^20 terms, so one dropped term of average
size S / M exceeds 16 u S = S / 2^20: the bar is sharp
(test_bn_train_host.py plants such defects and requires them to break it).

ReLU mask: from the reference's own float64 y; ``settle`` moves the cells of x
whose mask cannot be decided (|pre| <= 16 u S) and the tests assert on the
reference alone that none remain.
"""
import functools

import numpy as np

from _norm_ref64 import (BAR, U, _randn, _rng, _stable_seed, bound, eps32, f32,
                         f64, settle)

EPS = 1e-5
MOMENTUM = 0.1

# (N, C, P): M = 2 (unbiased factor 2) | odd P, scalar path, C below a wave |
# P % 4 == 0, vector path | several slices, a ragged last one | a long single
# image, nine slices
SHAPES = ((1, 3, 2), (2, 5, 253), (2, 40, 1028), (3, 8, 2050), (1, 16, 32776))
FLAGS = ((False, False), (False, True), (True, False), (True, True))
CONST_VALUE = 2.0 ** -6  # the constant channel of the 'const' cases


def _cs(a):
    """(C,) -> broadcastable against (N, C, P)."""
    return np.asarray(a, dtype=np.float64)[None, :, None]


def bn_train_stats(x, eps):
    """The batch statistics in float64 (two-pass variance) and their bars."""
    x = f64(x)
    M = x.shape[0] * x.shape[2]
    mean = x.sum((0, 2)) / M
    var = ((x - _cs(mean)) ** 2).sum((0, 2)) / M
    q = (x * x).sum((0, 2)) / M
    a = np.abs(x).sum((0, 2)) / M
    rstd = 1.0 / np.sqrt(var + eps32(eps))
    cancel = 2.0 ** -52 * q / (var + eps32(eps))
    return dict(M=M, mean=mean, var=var, q=q, S_mean=a, rstd=rstd,
                rstd_cancel=cancel, bar_rstd=(BAR * U + cancel) * rstd)


def bn_train_forward(x, gamma, beta, eps, res=None, relu=False, stats=None):
    """y = relu?(BN_batch(x) + res).  Returns the statistics dict plus y, pre,
    S, scale, shift (and their S)."""
    x = f64(x)
    st = dict(bn_train_stats(x, eps) if stats is None else stats)
    s = f64(gamma) * st['rstd']
    m, b = st['mean'], f64(beta)
    pre = x * _cs(s) - _cs(m * s) + _cs(b)
    S = np.abs(x * _cs(s)) + _cs(np.abs(m * s)) + _cs(np.abs(b))
    if res is not None:
        pre = pre + f64(res)
        S = S + np.abs(f64(res))
    st.update(y=np.maximum(pre, 0.0) if relu else pre, pre=pre, S=S, scale=s,
              S_scale=np.abs(s), shift=b - m * s,
              S_shift=np.abs(b) + np.abs(m * s))
    return st


def bn_train_running(x, running_mean, running_var, num_batches_tracked,
                     momentum, S_mean=None, S_var=None):
    """One update of the running statistics as torch.nn.BatchNorm2d does it
    (unbiased variance).  ``running_*`` are float64 values (the reference's own
    chain over several updates), ``S_*`` the bars' S so far (default: the
    magnitude of the buffers).  Returns dict(mean=(v, S), var=(v, S), count)."""
    x = f64(x)
    st = bn_train_stats(x, EPS)  # (its rstd is not used here)
    M, m = st['M'], float(momentum)
    rm = np.asarray(running_mean, dtype=np.float64)
    rv = np.asarray(running_var, dtype=np.float64)
    S_mean = np.abs(rm) if S_mean is None else S_mean
    S_var = np.abs(rv) if S_var is None else S_var
    unb = M / (M - 1.0)
    return dict(
        mean=((1 - m) * rm + m * st['mean'], (1 - m) * S_mean + m * st['S_mean']),
        var=((1 - m) * rv + m * st['var'] * unb,
             (1 - m) * S_var + m * unb * (st['q'] + st['S_mean'] ** 2)),
        count=int(num_batches_tracked) + 1)


def bn_train_backward(dy, x, mask, gamma, eps):
    """Backward of bn_train_forward.  ``mask``: y > 0 (None without ReLU).
    Returns dict of (value, S) for dx, dres, dgamma, dbeta."""
    x = f64(x)
    dz = f64(dy) if mask is None else f64(dy) * mask
    st = bn_train_stats(x, eps)
    M = st['M']
    m, r = _cs(st['mean']), _cs(st['rstd'])
    s = _cs(f64(gamma) * st['rstd'])
    xh = (x - m) * r
    ax = (np.abs(x) + np.abs(m)) * r
    t, S_t = dz * xh, np.abs(dz) * ax
    dbeta, dgamma = dz.sum((0, 2)), t.sum((0, 2))
    dx = s * (dz - _cs(dbeta) / M - xh * _cs(dgamma) / M)
    S_dx = np.abs(s) * (np.abs(dz) + _cs(np.abs(dz).sum((0, 2))) / M +
                        ax * _cs(S_t.sum((0, 2))) / M)
    return dict(dx=(dx, S_dx), dres=(dz, np.abs(dz)),
                dgamma=(dgamma, S_t.sum((0, 2))),
                dbeta=(dbeta, np.abs(dz).sum((0, 2))))


# ----------------------------------------------- the device's operations --
DEFECTS = ('running_var_biased', 'norm_var_unbiased', 'dx_m_minus_1',
           'dx_no_xhat_term', 'stats_drop_one', 'dgamma_drop_one')


def device_emulation(x, gamma, beta, eps, momentum, running_mean, running_var,
                     dy, res=None, relu=False, defect=None):
    """The kernels' arithmetic restated with numpy: fp64 sums of fp32 terms,
    every other operation rounded to fp32 where the device rounds.  ``defect``
    plants one of DEFECTS.  Returns dict(y, mean, rstd, running_mean,
    running_var, dx, dres, dgamma, dbeta) as fp32 arrays."""
    assert defect is None or defect in DEFECTS
    F = np.float32
    x = f32(x)
    xd = x.astype(np.float64)
    M = x.shape[0] * x.shape[2]
    s, q = xd.sum((0, 2)), (xd * xd).sum((0, 2))
    if defect == 'stats_drop_one':
        s, q = s - xd[0, :, 0], q - xd[0, :, 0] ** 2
    m = s / M
    var = np.maximum(q / M - m * m, 0.0)
    unb = var * (M / (M - 1.0))
    nvar = unb if defect == 'norm_var_unbiased' else var
    mu = m.astype(F)
    r = (1.0 / np.sqrt(nvar + float(F(eps)))).astype(F)
    sc = f32(gamma) * r
    sh = f32(beta) - mu * sc
    y = x * sc[None, :, None] + sh[None, :, None]
    if res is not None:
        y = y + f32(res)
    if relu:
        y = np.maximum(y, F(0))
    mom = float(momentum)
    rvar = var if defect == 'running_var_biased' else unb
    rm = ((1 - mom) * f64(running_mean) + mom * m).astype(F)
    rv = ((1 - mom) * f64(running_var) + mom * rvar).astype(F)
    dz = f32(dy) * (y > 0) if relu else f32(dy)
    dz = dz.astype(F)
    xh = (x - mu[None, :, None]) * r[None, :, None]
    t = dz * xh
    assert y.dtype == F and xh.dtype == F and t.dtype == F
    s1 = dz.astype(np.float64).sum((0, 2))
    s2 = t.astype(np.float64).sum((0, 2))
    if defect == 'dgamma_drop_one':
        s2 = s2 - t[0, :, 0].astype(np.float64)
    Md = M - 1.0 if defect == 'dx_m_minus_1' else float(M)
    k1 = (s1 / Md).astype(F)[None, :, None]
    k2 = (s2 / Md).astype(F)[None, :, None]
    inner = dz - k1
    if defect != 'dx_no_xhat_term':
        inner = inner - xh * k2
    dx = sc[None, :, None] * inner
    assert dx.dtype == F
    return dict(y=y, mean=mu, rstd=r, running_mean=rm, running_var=rv, dx=dx,
                dres=dz, dgamma=s2.astype(F), dbeta=s1.astype(F))


# ------------------------------------------------------------ case inputs --
@functools.lru_cache(maxsize=None)
def bn_train_inputs(N, C, P, relu, with_res, tag=''):
    """Seeded operands of a case: dict(x, res, gamma, beta, running_mean,
    running_var, dy, rounds); x settled for ReLU cases.  ``tag``: '' |
    'offset' (x = 256 + noise: cancellation in q/M - mean^2) | 'const'
    (channel 0 is the constant CONST_VALUE: var = 0, rstd = 1/sqrt(eps)).
    The arrays are shared between tests: do not write to them."""
    rng = _rng('bn_train', N, C, P, with_res, tag)
    x = _randn(rng, N, C, P) * np.float32(1.5) + np.float32(0.25)
    if tag == 'offset':
        x = _randn(rng, N, C, P) + np.float32(256)
    if tag == 'const':
        x[:, 0, :] = np.float32(CONST_VALUE)
    res = _randn(rng, N, C, P) if with_res else None
    gamma, beta = _randn(rng, C), _randn(rng, C)
    running_mean = _randn(rng, C)
    running_var = (rng.random(C) + 0.5).astype(np.float32)
    dy = _randn(rng, N, C, P)
    rounds = 0
    if relu:
        def ev(xx):
            r = bn_train_forward(xx, gamma, beta, EPS, res)
            return r['pre'], r['S']
        x, rounds = settle(x, ev, seed=_stable_seed(('bn_train', N, C, P)))
    if tag == 'const':
        assert (x[:, 0, :] == np.float32(CONST_VALUE)).all(), \
            'settle moved a cell of the constant channel'
    for a in (x, res, gamma, beta, running_mean, running_var, dy):
        if a is not None:
            a.setflags(write=False)
    return dict(x=x, res=res, gamma=gamma, beta=beta,
                running_mean=running_mean, running_var=running_var, dy=dy,
                rounds=rounds)


@functools.lru_cache(maxsize=None)
def bn_train_reference(N, C, P, relu, with_res, tag=''):
    """The float64 forward, backward and one running update of a case,
    computed once and shared: dict(inp, fwd, bwd, run, undecided)."""
    inp = bn_train_inputs(N, C, P, relu, with_res, tag)
    fwd = bn_train_forward(inp['x'], inp['gamma'], inp['beta'], EPS,
                           inp['res'], relu)
    mask = (fwd['y'] > 0) if relu else None
    bwd = bn_train_backward(inp['dy'], inp['x'], mask, inp['gamma'], EPS)
    run = bn_train_running(inp['x'], f64(inp['running_mean']),
                           f64(inp['running_var']), 0, MOMENTUM)
    und = int((np.abs(fwd['pre']) <= bound(fwd['S'])).sum()) if relu else 0
    return dict(inp=inp, fwd=fwd, bwd=bwd, run=run, undecided=und)
