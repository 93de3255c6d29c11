"""CPU: the sampled float64 conv reference (tests/_conv_ref64.py) is right --
equal to torch's float64 convolutions -- and sharp: an fp32 conv of the same
operands passes its bar, and the kernel bugs it exists to catch fail it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_ref64 as R

# name, N, Cin, Cout, k, stride, pad, levels
SHAPES = [
    ('3x3_levels', 2, 48, 40, 3, 1, 1, ((9, 13), (5, 7), (3, 4), (2, 2), (1, 1))),
    ('3x3_s2_odd', 2, 32, 24, 3, 2, 1, ((11, 15), (6, 7))),
    ('1x1_s2', 2, 64, 48, 1, 2, 0, ((10, 13), )),
    ('7x7_s2_p3', 1, 3, 16, 7, 2, 3, ((19, 23), )),
    ('1x1_levels', 2, 40, 72, 1, 1, 0, ((6, 8), (3, 4), (2, 2))),
]


def _levels_view(t, levels, offs):
    """(N, C, P) -> list of (N, C, h, w) level images."""
    return [t[:, :, o:o + h * w].reshape(t.shape[0], t.shape[1], h, w)
            for (h, w), o in zip(levels, offs)]


def _cat(imgs):
    return torch.cat([i.reshape(i.shape[0], i.shape[1], -1) for i in imgs], 2)


def _operands(g, seed, absx=False, dtype=torch.float32):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(g.N, g.Cin, g.Pin, generator=gen, dtype=dtype)
    if absx:
        x = x.abs()
    w = torch.randn(g.Cout, g.Cin, g.k, g.k, generator=gen, dtype=dtype)
    dy = torch.randn(g.N, g.Cout, g.Pout, generator=gen, dtype=dtype)
    return x, w, dy


def _torch_fwd(g, x, w):
    return _cat([F.conv2d(xi, w, stride=g.stride, padding=g.pad)
                 for xi in _levels_view(x, g.levels, g.off_in)])


def _torch_dgrad(g, dy, w):
    outs = []
    for dyi, (h, wd) in zip(_levels_view(dy, g.out_levels, g.off_out),
                            g.levels):
        ho, wo = dyi.shape[2:]
        oph = h - ((ho - 1) * g.stride - 2 * g.pad + g.k)
        opw = wd - ((wo - 1) * g.stride - 2 * g.pad + g.k)
        outs.append(F.conv_transpose2d(dyi, w, stride=g.stride, padding=g.pad,
                                       output_padding=(oph, opw)))
    return _cat(outs)


def _torch_wgrad(g, x, dy):
    dw = 0
    for xi, dyi in zip(_levels_view(x, g.levels, g.off_in),
                       _levels_view(dy, g.out_levels, g.off_out)):
        dw = dw + torch.nn.grad.conv2d_weight(xi, (g.Cout, g.Cin, g.k, g.k),
                                              dyi, stride=g.stride,
                                              padding=g.pad)
    return dw


def _geom(case):
    return R.Geom(*case[1:])


@pytest.mark.parametrize('case', SHAPES, ids=[c[0] for c in SHAPES])
def test_ref_equals_torch_float64(case):
    g = _geom(case)
    x, w, dy = _operands(g, 1, dtype=torch.float64)
    # the reference works from fp32 operands: make them fp32-exact
    x, w, dy = x.float().double(), w.float().double(), dy.float().double()
    y = _torch_fwd(g, x, w)
    n, co, p = R.sample_elements(g.N, g.Cout, g.out_levels, g.off_out, g.Pout, 3)
    ref, S, K = R.forward(g, x.float(), w.float(), n, co, p)
    np.testing.assert_allclose(ref, y[n, co, p].numpy(), rtol=1e-12,
                               atol=1e-12 * float(y.abs().max()))
    assert (S >= np.abs(ref)).all() and (K <= g.Cin * g.T).all()
    dx = _torch_dgrad(g, dy, w)
    n, ci, q = R.sample_elements(g.N, g.Cin, g.levels, g.off_in, g.Pin, 4)
    ref, S, K = R.dgrad(g, dy.float(), w.float(), n, ci, q)
    np.testing.assert_allclose(ref, dx[n, ci, q].numpy(), rtol=1e-12,
                               atol=1e-12 * float(dx.abs().max()))
    dw = _torch_wgrad(g, x, dy).reshape(g.Cout, g.Cin, g.T)
    co, ci, t = R.sample_weights(g, 5)
    assert set(t.tolist()) == set(range(g.T))
    ref, S, K = R.wgrad(g, x.float(), dy.float(), co, ci, t)
    np.testing.assert_allclose(ref, dw[co, ci, t].numpy(), rtol=1e-12,
                               atol=1e-12 * float(dw.abs().max()))


def test_sampling_hits_the_edges():
    g = R.Geom(2, 300, 260, 3, 1, 1, ((40, 50), (20, 25), (10, 13)))
    n, c, p = R.sample_elements(g.N, g.Cout, g.out_levels, g.off_out, g.Pout, 0)
    ps = set(p.tolist())
    for o in g.off_out[1:]:
        assert {o - 1, o} <= ps
    assert {g.Pout - 1, 255, 256, 257, 31, 33} <= ps
    assert {0, 1, 31, 32, 255, 256, 259} <= set(c.tolist())
    co, ci, t = R.sample_weights(g, 0)
    assert {127, 128, 255, 256, 259} <= set(co.tolist())
    assert {127, 128, 255, 256, 299} <= set(ci.tolist())


# ------------------------------------------------- fp32 passes, mutants fail --
def _fp32_all(g, x, w, dy):
    return _torch_fwd(g, x, w), _torch_dgrad(g, dy, w), _torch_wgrad(g, x, dy)


@pytest.mark.parametrize('absx', [False, True])
@pytest.mark.parametrize('case', SHAPES, ids=[c[0] for c in SHAPES])
def test_fp32_conv_passes_the_bar(case, absx):
    g = _geom(case)
    x, w, dy = _operands(g, 7, absx)
    y, dx, dw = _fp32_all(g, x, w, dy)
    n, co, p = R.sample_elements(g.N, g.Cout, g.out_levels, g.off_out, g.Pout, 1)
    ref, S, _ = R.forward(g, x, w, n, co, p)
    assert R.check(y[n, co, p].numpy(), ref, S, what='fwd') <= R.BAR
    n, ci, q = R.sample_elements(g.N, g.Cin, g.levels, g.off_in, g.Pin, 2)
    ref, S, _ = R.dgrad(g, dy, w, n, ci, q)
    R.check(dx[n, ci, q].numpy(), ref, S, what='dgrad')
    co, ci, t = R.sample_weights(g, 3)
    ref, S, _ = R.wgrad(g, x, dy, co, ci, t)
    R.check(dw.reshape(g.Cout, g.Cin, -1)[co, ci, t].numpy(), ref, S,
            what='wgrad')


def test_fp32_wgrad_passes_at_the_largest_reduction():
    """The largest K on the GPU: a weight gradient over 2 x 67 200 positions
    (layer 1 of the C2 step, 200 x 336)."""
    g = R.Geom(2, 16, 16, 3, 1, 1, ((200, 336), ))
    x, _, dy = _operands(g, 11)
    dw = _torch_wgrad(g, x, dy).reshape(g.Cout, g.Cin, -1)
    co, ci, t = R.sample_weights(g, 3)
    ref, S, K = R.wgrad(g, x, dy, co, ci, t)
    assert K.max() == 2 * 67200
    worst = R.check(dw[co, ci, t].numpy(), ref, S, what='wgrad K=134400')
    print('largest-K fp32 wgrad: worst err/(uS) %.2f' % worst)
    # and one dropped term of average size is still outside the bar
    i = int(np.argmax(K))
    got = dw[co, ci, t].double().numpy().copy()
    got[i] -= S[i] / K[i]
    with pytest.raises(AssertionError):
        R.check(got, ref, S)


def _rejects(got, ref, S, bar=None):
    with pytest.raises(AssertionError, match='outside the bar'):
        R.check(got, ref, S, bar)


def test_mutant_one_term_dropped():
    g = _geom(SHAPES[0])
    x, w, dy = _operands(g, 21)
    y = _torch_fwd(g, x, w)
    n, co, p = R.sample_elements(g.N, g.Cout, g.out_levels, g.off_out, g.Pout, 1)
    ref, S, K = R.forward(g, x, w, n, co, p)
    got = y[n, co, p].double().numpy()
    R.check(got, ref, S)
    # drop the median-magnitude term of one interior element
    i = int(np.argmax(K))
    src = g.src()[p[i]]
    terms = torch.stack([x[n[i], :, s] * w[co[i], :, tp // g.k, tp % g.k]
                         for tp, s in enumerate(src.tolist()) if s >= 0]).reshape(-1)
    tm = terms[terms.abs().argsort()[len(terms) // 2]]
    bad = got.copy()
    bad[i] -= float(tm)
    _rejects(bad, ref, S)


def test_mutant_padding_tap_from_neighbouring_row():
    """A kernel that lets the left padding tap of column 0 read the previous
    row's last element (flat index - 1) instead of zero."""
    g = _geom(SHAPES[0])
    x, w, _ = _operands(g, 22)
    src = g.src().clone()
    for (h, wd), (ho, wo), oi, oo in zip(g.levels, g.out_levels, g.off_in,
                                         g.off_out):
        for r in range(1, ho):  # row 0's neighbour would be another level
            p = oo + r * wo
            for t in range(0, g.T, g.k):  # kw == 0 taps of column 0
                kh = t // g.k
                hi = r * g.stride - g.pad + kh
                if 0 <= hi < h:
                    src[p, t] = oi + hi * wd - 1
    gbug = R.Geom(*SHAPES[0][1:])
    gbug._src = src
    y = _torch_fwd(g, x, w)
    n, co, p = R.sample_elements(g.N, g.Cout, g.out_levels, g.off_out, g.Pout, 1)
    bug_ref, _, _ = R.forward(gbug, x, w, n, co, p)
    ref, S, _ = R.forward(g, x, w, n, co, p)
    got = y[n, co, p].double().numpy()
    R.check(got, ref, S)
    moved = bug_ref != ref
    assert moved.any(), 'the sample set must include column 0 of some row'
    # the fp32 result with the buggy elements replaced
    got = np.where(moved, bug_ref.astype(np.float32).astype(np.float64), got)
    _rejects(got, ref, S)


def test_mutant_shift_at_level_boundary():
    """Level 1 read one position early (off_in - 1)."""
    g = _geom(SHAPES[0])
    x, w, _ = _operands(g, 23)
    x_bug = x.clone()
    o1, o2 = g.off_in[1], g.off_in[2]
    x_bug[:, :, o1:o2] = x[:, :, o1 - 1:o2 - 1]
    y_bug = _torch_fwd(g, x_bug, w)
    n, co, p = R.sample_elements(g.N, g.Cout, g.out_levels, g.off_out, g.Pout, 1)
    ref, S, _ = R.forward(g, x, w, n, co, p)
    R.check(_torch_fwd(g, x, w)[n, co, p].numpy(), ref, S)
    _rejects(y_bug[n, co, p].numpy(), ref, S)


def test_mutant_last_k_slice_missing():
    """The last 16 input channels of the reduction skipped (forward) / the last
    16 output channels (data gradient)."""
    g = _geom(SHAPES[0])
    x, w, dy = _operands(g, 24)
    y_bug = _torch_fwd(g, x[:, :-16], w[:, :-16])
    n, co, p = R.sample_elements(g.N, g.Cout, g.out_levels, g.off_out, g.Pout, 1)
    ref, S, _ = R.forward(g, x, w, n, co, p)
    _rejects(y_bug[n, co, p].numpy(), ref, S)
    dx_bug = _torch_dgrad(g, dy[:, :-16], w[:-16])
    n, ci, q = R.sample_elements(g.N, g.Cin, g.levels, g.off_in, g.Pin, 2)
    ref, S, _ = R.dgrad(g, dy, w, n, ci, q)
    R.check(_torch_dgrad(g, dy, w)[n, ci, q].numpy(), ref, S)
    _rejects(dx_bug[n, ci, q].numpy(), ref, S)


def test_mutant_wgrad_missing_one_image():
    g = _geom(SHAPES[1])
    x, _, dy = _operands(g, 25)
    gb = R.Geom(1, *SHAPES[1][2:])
    dw_bug = _torch_wgrad(gb, x[1:], dy[1:]).reshape(g.Cout, g.Cin, -1)
    co, ci, t = R.sample_weights(g, 3)
    ref, S, _ = R.wgrad(g, x, dy, co, ci, t)
    _rejects(dw_bug[co, ci, t].numpy(), ref, S)


@pytest.mark.parametrize('absx', [False, True])
def test_mutant_bf16_rounded_toward_zero(absx):
    g = R.Geom(2, 256, 64, 3, 1, 1, ((12, 17), (6, 9)))
    x, w, dy = _operands(g, 26, absx)
    n, co, p = R.sample_elements(g.N, g.Cout, g.out_levels, g.off_out, g.Pout, 1)
    ref, S, _ = R.forward(g, x, w, n, co, p, bf16=True)
    good = _torch_fwd(g, R.bf16_rne(x), R.bf16_rne(w))
    R.check(good[n, co, p].numpy(), ref, S)
    bug = _torch_fwd(g, R.bf16_rtz(x), R.bf16_rtz(w))
    _rejects(bug[n, co, p].numpy(), ref, S)
    # the data and weight gradients round their own operand pairs
    n, ci, q = R.sample_elements(g.N, g.Cin, g.levels, g.off_in, g.Pin, 2)
    ref, S, _ = R.dgrad(g, dy, w, n, ci, q, bf16=True)
    R.check(_torch_dgrad(g, R.bf16_rne(dy), R.bf16_rne(w))[n, ci, q].numpy(),
            ref, S)
    _rejects(_torch_dgrad(g, R.bf16_rtz(dy), R.bf16_rtz(w))[n, ci, q].numpy(),
             ref, S)
    co, ci, t = R.sample_weights(g, 3)
    ref, S, _ = R.wgrad(g, x, dy, co, ci, t, bf16=True)
    dw = _torch_wgrad(g, R.bf16_rne(x), R.bf16_rne(dy)).reshape(g.Cout, g.Cin, -1)
    R.check(dw[co, ci, t].numpy(), ref, S)
    dw = _torch_wgrad(g, R.bf16_rtz(x), R.bf16_rtz(dy)).reshape(g.Cout, g.Cin, -1)
    _rejects(dw[co, ci, t].numpy(), ref, S)


def test_epilogue_bar():
    g = _geom(SHAPES[0])
    x, w, _ = _operands(g, 27)
    gen = torch.Generator().manual_seed(0)
    scale = torch.rand(g.Cout, generator=gen) + 0.5
    shift = torch.randn(g.Cout, generator=gen)
    res = torch.randn(g.N, g.Cout, g.Pout, generator=gen)
    y = torch.relu(_torch_fwd(g, x, w) * scale[:, None] + shift[:, None] + res)
    n, co, p = R.sample_elements(g.N, g.Cout, g.out_levels, g.off_out, g.Pout, 1)
    ref, S, _ = R.forward(g, x, w, n, co, p)
    v, bar = R.epilogue(ref, S, scale[co].double().numpy(),
                        shift[co].double().numpy(),
                        res[n, co, p].double().numpy(), relu=True)
    R.check(y[n, co, p].numpy(), v, S, bar)
    # the C8 image of it (bf16 RNE of the fp32 result)
    v8, bar8 = R.epilogue(ref, S, scale[co].double().numpy(),
                          shift[co].double().numpy(),
                          res[n, co, p].double().numpy(), relu=True, c8=True)
    R.check(R.bf16_rne(y)[n, co, p].numpy(), v8, S, bar8)
    # the residual forgotten
    y_bug = torch.relu(_torch_fwd(g, x, w) * scale[:, None] + shift[:, None])
    _rejects(y_bug[n, co, p].numpy(), v, S, bar)
