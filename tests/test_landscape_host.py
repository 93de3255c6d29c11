"""CPU-side checks of ld_amd.landscape (no GPU): grid ordering, chunking and
meta repetition, the ValueErrors of mismatched inputs, the C ABI's argument
validation, and the float64 restatements of tests/_landscape_oracle.py against
hand-derived answers and against the reference's literal fp32 expression."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _landscape_oracle as O  # noqa: E402

LEVELS = ((5, 7), (3, 4), (2, 2), (1, 1))
P = sum(h * w for h, w in LEVELS)


def _maps(n, c, levels=LEVELS, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, c, h, w, generator=g) for h, w in levels]


# ------------------------------------------------------------ grid, chunks --
def test_grid_is_alpha_major_and_compute_shape():
    from ld_amd.landscape import FeatureLandscape
    g = FeatureLandscape.grid([0.0, 0.5, 1.0], [0.25, 0.75])
    assert list(g) == [(0.0, 0.25), (0.0, 0.75), (0.5, 0.25), (0.5, 0.75),
                       (1.0, 0.25), (1.0, 0.75)]
    assert g.shape == (3, 2)
    g = FeatureLandscape.grid((a for a in (1, 2)), (b for b in (3, )))
    assert list(g) == [(1.0, 3.0), (2.0, 3.0)] and g.shape == (2, 1)
    with pytest.raises(ValueError):
        FeatureLandscape.grid([], [1.0])


def test_chunks_keep_the_head_batch_at_16():
    from ld_amd import lib as L
    from ld_amd.landscape import FeatureLandscape as F
    assert F.chunks(25, 1) == [(0, 16), (16, 25)]
    assert F.chunks(25, 2) == [(0, 8), (8, 16), (16, 24), (24, 25)]
    assert F.chunks(4, 3) == [(0, 4)]          # 5 points would fit
    assert F.chunks(6, 3) == [(0, 5), (5, 6)]
    assert F.chunks(3, 32) == [(0, 1), (1, 2), (2, 3)]  # never below 1
    assert F.chunks(5, 2, chunk=1) == [(k, k + 1) for k in range(5)]
    assert F.chunks(5, 2, chunk=2) == [(0, 2), (2, 4), (4, 5)]
    # one mix launch per chunk: the chunk never exceeds the launch cap
    cap = L.LD_LEVELS_MIX_MAX_K
    assert F.chunks(40, 1, chunk=100) == [(0, cap), (cap, 2 * cap),
                                          (2 * cap, 40)]
    for K, N, ch in ((25, 2, None), (7, 1, 3), (1, 1, None)):
        spans = F.chunks(K, N, ch)
        assert [k for a, b in spans for k in range(a, b)] == list(range(K))


def test_metas_repeat_grid_point_major():
    from ld_amd.landscape import repeat_metas
    metas = [dict(i=0), dict(i=1)]
    rep = repeat_metas(metas, 3)
    assert [m['i'] for m in rep] == [0, 1, 0, 1, 0, 1]
    assert rep[2] is metas[0]
    assert repeat_metas(metas, 1) == metas


class _Model:
    teacher_model = None


def test_constructor_arguments():
    from ld_amd.landscape import FeatureLandscape, TeacherStudentDiscrepancy
    made = []
    fac = lambda: made.append(1) or object()  # noqa: E731
    with pytest.raises(ValueError):           # no teacher anywhere
        FeatureLandscape(_Model(), evaluator_factory=fac)
    with pytest.raises(ValueError):
        TeacherStudentDiscrepancy(_Model())
    with pytest.raises(ValueError):
        FeatureLandscape(_Model(), _Model(), head='both',
                         evaluator_factory=fac)
    with pytest.raises(ValueError):
        FeatureLandscape(_Model(), _Model())  # no evaluator factory
    with pytest.raises(ValueError):
        FeatureLandscape(_Model(), _Model(), coefs=[], evaluator_factory=fac)
    with pytest.raises(ValueError):
        FeatureLandscape(_Model(), _Model(), coefs=[0.9, 0.7],
                         evaluator_factory=fac)
    with pytest.raises(ValueError):
        FeatureLandscape(_Model(), _Model(), chunk=0, evaluator_factory=fac)
    del made[:]
    s, t = _Model(), _Model()
    land = FeatureLandscape(s, t, coefs=FeatureLandscape.grid([1, 2], [3, 4]),
                            head='teacher', evaluator_factory=fac)
    assert len(made) == 4 == len(land.evaluators) and land.shape == (2, 2)
    assert land.own is t and land.other is s
    land = FeatureLandscape(s, t, evaluator_factory=fac)
    assert land.coefs == [(0.9, 0.7)] and land.own is s and land.shape is None


# -------------------------------------------------------------- mismatches --
def test_mismatched_inputs_raise_value_error():
    from ld_amd.landscape import TeacherStudentDiscrepancy, mix_levels
    a = _maps(2, 5)
    with pytest.raises(ValueError, match='level shapes'):
        mix_levels(a, _maps(2, 5, LEVELS[:3] + ((1, 2), )), [(1, 0)])
    with pytest.raises(ValueError, match='level shapes'):
        mix_levels(a, _maps(2, 5, LEVELS[:3]), [(1, 0)])
    with pytest.raises(ValueError, match='shapes differ'):
        mix_levels(a, _maps(2, 6), [(1, 0)])        # channels
    with pytest.raises(ValueError, match='shapes differ'):
        mix_levels(a, _maps(3, 5), [(1, 0)])        # batch
    with pytest.raises(ValueError):
        mix_levels(a, a, [])
    with pytest.raises(ValueError):
        mix_levels(a[:1] + _maps(2, 4)[1:], a, [(1, 0)])  # ragged channels
    x3 = torch.zeros(2, 5, P)
    with pytest.raises(ValueError, match='levels'):
        mix_levels(x3, x3, [(1, 0)])                # packed without levels
    with pytest.raises(ValueError, match='do not sum'):
        mix_levels(x3, x3, [(1, 0)], levels=LEVELS[:3])
    with pytest.raises(ValueError):
        mix_levels([f.double() for f in a], a, [(1, 0)])
    # valid arguments on the CPU: there is no CPU path
    from ld_amd import lib as L
    with pytest.raises(L.LdError):
        mix_levels(a, _maps(2, 5, seed=1), [(1, 0)])
    acc = TeacherStudentDiscrepancy(_Model(), _Model())
    xs, xt = _maps(1, 8), _maps(1, 8, seed=1)
    cls_s, cls_t = _maps(1, 3), _maps(1, 3, seed=1)
    box_s, box_t = _maps(1, 4), _maps(1, 4, seed=1)
    with pytest.raises(ValueError, match='feature'):
        acc.add_outputs(xs, _maps(1, 7), (cls_s, box_s), (cls_t, box_t))
    with pytest.raises(ValueError, match='cls'):
        acc.add_outputs(xs, xt, (cls_s, box_s), (_maps(1, 2), box_t))
    with pytest.raises(ValueError, match='bbox'):
        acc.add_outputs(xs, xt, (cls_s, box_s),
                        (cls_t, _maps(1, 4, LEVELS[:2] + ((2, 3), (1, 1)))))
    with pytest.raises(ValueError):
        acc.compute()


def test_forward_packed_checks_its_input():
    from ld_amd.registry import build_head
    head = build_head(dict(type='GFLHead', num_classes=3, in_channels=8,
                           feat_channels=8, stacked_convs=1,
                           norm_cfg=dict(type='GN', num_groups=2,
                                         requires_grad=True)))
    five = ((4, 4), (2, 2), (1, 1), (1, 1), (1, 1))
    with pytest.raises(ValueError, match='levels'):
        head.forward_packed(torch.zeros(1, 8, 21), five[:3])
    with pytest.raises(ValueError, match='not'):
        head.forward_packed(torch.zeros(1, 7, 23), five)
    with pytest.raises(ValueError, match='not'):
        head.forward_packed(torch.zeros(1, 8, 22), five)
    with pytest.raises(ValueError, match='contiguous'):
        head.forward_packed(torch.zeros(1, 23, 8).transpose(1, 2), five)


# -------------------------------------------------------------------- C ABI --
def test_cabi_rejects_bad_arguments_without_a_device():
    from ld_amd import layers as Y
    from ld_amd import lib as L
    lib = L.get_lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    co = C.cast((C.c_float * 64)(), C.c_void_p)
    mix = lib.ld_levels_mix
    assert mix(None, p, 16, 1, co, p, None) == -1
    assert mix(p, None, 16, 1, co, p, None) == -1
    assert mix(p, p, 16, 1, None, p, None) == -1
    assert mix(p, p, 16, 1, co, None, None) == -1
    assert mix(p, p, 0, 1, co, p, None) == -1
    assert mix(p, p, -4, 1, co, p, None) == -1
    assert mix(p, p, 16, 0, co, p, None) == -1
    assert mix(p, p, 16, L.LD_LEVELS_MIX_MAX_K + 1, co, p, None) == -1
    lv = Y.levels_desc(LEVELS)
    for size, run, extra in (
            (lib.ld_levels_abs_err_workspace_bytes, lib.ld_levels_abs_err,
             (p, )),
            (lib.ld_levels_pearson_workspace_bytes, lib.ld_levels_pearson,
             (p, p))):
        assert size(C.byref(lv), 2, 5, P) > 0
        assert size(C.byref(lv), 2, 5, P + 1) == 0   # levels do not fill P
        assert size(C.byref(lv), 2, 5, P - 1) == 0
        assert size(C.byref(lv), 0, 5, P) == 0
        assert size(C.byref(lv), 2, 0, P) == 0
        assert size(C.byref(lv), 2, 5, 0) == 0
        assert size(None, 2, 5, P) == 0
        ok = (C.byref(lv), p, p, 2, 5, P) + extra + (p, 1 << 20, None)
        for i, bad in ((0, None), (1, None), (2, None), (3, 0), (3, -1),
                       (4, 0), (5, P + 1), (5, 0), (6, None)):
            args = list(ok)
            args[i] = bad
            assert run(*args) == -1, (run.__name__, i)
        if len(extra) == 2:                           # counts
            args = list(ok)
            args[7] = None
            assert run(*args) == -1
        args = list(ok)
        args[-3] = None                               # no workspace
        assert run(*args) == -2
        args = list(ok)
        args[-2] = 8                                  # too small
        assert run(*args) == -2
    none = L.LevelsT()
    assert lib.ld_levels_abs_err_workspace_bytes(C.byref(none), 1, 1, 1) == 0
    zero = Y.levels_desc(((3, 0), (1, 1)))
    assert lib.ld_levels_pearson_workspace_bytes(C.byref(zero), 1, 1, 1) == 0


# ----------------------------------------------------------- the oracle --
def test_oracle_against_hand_derived_answers():
    N, c = 2, 6
    s3, levels = O.pack(_maps(N, c, seed=3))
    pos = torch.tensor([h * w for h, w in levels], dtype=torch.float64)
    # identical inputs: error 0, r = 1 (the single-position level is
    # degenerate: torch's 0 / 0)
    assert torch.equal(O.abs_err(s3, s3, levels), torch.zeros(N, 4).double())
    r = O.pearson_rows(s3, s3, levels)
    assert torch.isnan(r[:, 3]).all()
    np.testing.assert_allclose(r[:, :3].numpy(), 1.0, rtol=0, atol=1e-12)
    # t = -s: r = -1, error = 2 |s|
    r = O.pearson_rows(-s3, s3, levels)
    np.testing.assert_allclose(r[:, :3].numpy(), -1.0, rtol=0, atol=1e-12)
    # t = s + const (a power of two on O(1) data: the fp32 difference is exact
    # to 2^-22): error = const per position, r = 1
    e = O.abs_err(s3 + 0.5, s3, levels)
    np.testing.assert_allclose((e / pos[None]).numpy(), 0.5, rtol=1e-6)
    r = O.pearson_rows(s3 + 0.5, s3, levels)
    np.testing.assert_allclose(r[:, :3].numpy(), 1.0, rtol=0, atol=1e-6)
    # a constant row is degenerate, in either operand, and is counted
    t3 = s3.clone()
    t3[1, 2, :35] = 4.0                 # level 0 of row (1, 2)
    r = O.pearson_rows(t3, s3, levels)
    assert torch.isnan(r[1, 0, 2]) and not torch.isnan(r[1, 1, 2])
    assert torch.isnan(O.pearson_rows(s3, t3, levels)[1, 0, 2])
    rs, valid, bad = O.pearson(t3, s3, levels)
    assert valid.tolist() == [[c, c, c, 0], [c - 1, c, c, 0]]
    assert bad.tolist() == [[0, 0, 0, c], [1, 0, 0, c]]
    keep = [k for k in range(c) if k != 2]
    np.testing.assert_allclose(float(rs[1, 0]), float(r[1, 0, keep].sum()),
                               rtol=1e-15)
    # a two-point segment: r is +-1 whatever the values
    x = torch.tensor([[[1.0, 3.0]]])
    assert float(O.pearson_rows(x, x * -2, ((1, 2), ))[0, 0, 0]) == -1.0


@pytest.mark.parametrize('c', [1, 68, 80, 256])
def test_oracle_agrees_with_the_reference_fp32_expression(c):
    """float64 sums of the fp32 |t - s| against abs(t - s).mean(1).sum() in
    fp32 as the reference writes it: its pairwise fp32 sums of <= 2^16
    non-negative terms are good to about log2(n) * 2^-24 ~ 1e-6; rtol 1e-5
    leaves 10x over that."""
    levels = ((13, 21), (7, 11), (1, 1))
    t3, _ = O.pack(_maps(2, c, levels, seed=5))
    s3, _ = O.pack(_maps(2, c, levels, seed=6))
    np.testing.assert_allclose(O.abs_err(t3, s3, levels).numpy(),
                               O.abs_err_reference_fp32(t3, s3, levels)
                               .double().numpy(), rtol=1e-5)


def test_oracle_discrepancy_of_a_model_with_itself():
    xs = _maps(2, 8, seed=1)
    outs = (_maps(2, 3, seed=2), _maps(2, 4, seed=3))
    d = O.discrepancy([(xs, xs, outs, outs), (xs, xs, outs, outs)])
    assert d['num_images'] == 4
    assert d['feature_error'] == d['cls_error'] == d['bbox_error'] == 0.0
    np.testing.assert_allclose(d['pearson'][:3], 1.0, atol=1e-12)
    assert np.isnan(d['pearson'][3])
    assert d['degenerate_rows'].tolist() == [0, 0, 0, 4 * 8]
