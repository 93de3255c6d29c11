"""Host tests (no GPU, no library) of the parameter-gradient protocol of
ld_amd.layers: ``_grad_outs`` / ``_grad_done`` (where the gradients of one
backward's parameter group go: the arena slices, or fresh tensors handed to
autograd), ``_note_use`` / ``_emit`` (one emit per use, the ready callback after
the last) and the C8 predicates of the conv backward, the latter against the
expressions they replaced."""
import itertools

import pytest
import torch

from ld_amd import layers as Y


def _param(n=4, slice_=True, ready=None):
    p = torch.zeros(n, requires_grad=True)
    if slice_:
        p._ld_grad = torch.zeros(n)
        p._ld_ready = (lambda q: ready.append(q)) if ready is not None else None
        p._ld_pending = 0
    return p


def _alloc(p):
    return torch.full_like(p, 7.0).detach()


def test_noted_twice_fires_ready_once_after_the_second_emit():
    fired = []
    p = _param(ready=fired)
    Y._note_use(p)
    Y._note_use(p, None)
    assert p._ld_pending == 2
    Y._emit(p)
    assert fired == [] and p._ld_pending == 1
    Y._emit(p)
    assert len(fired) == 1 and fired[0] is p and p._ld_pending == 0
    # a parameter without a slice is not counted
    q = _param(slice_=False)
    Y._note_use(q)
    assert getattr(q, '_ld_pending', 0) == 0


def test_pair_with_both_slices_is_direct():
    fired = []
    pg, pb = _param(ready=fired), _param(ready=fired)
    Y._note_use(pg, pb)
    outs, direct = Y._grad_outs((pg, pb), (True, True), _alloc)
    assert direct
    # the kernel accumulates into the slices' storage
    assert outs[0].data_ptr() == pg._ld_grad.data_ptr()
    assert outs[1].data_ptr() == pb._ld_grad.data_ptr()
    assert fired == []  # nothing is emitted before the launch
    assert tuple(Y._grad_done((pg, pb), outs, direct)) == (None, None)
    assert [id(p) for p in fired] == [id(pg), id(pb)]
    assert pg._ld_pending == 0 and pb._ld_pending == 0


@pytest.mark.parametrize('why', ['switch_off', 'no_slice'])
def test_fresh_tensors_and_no_emit_without_a_sink(why):
    fired = []
    pg, pb = (_param(slice_=why == 'switch_off', ready=fired) for _ in range(2))
    Y._note_use(pg, pb)
    prev = Y.DIRECT_GRADS[0]
    Y.DIRECT_GRADS[0] = why != 'switch_off'
    try:
        outs, direct = Y._grad_outs((pg, pb), (True, True), _alloc)
        back = Y._grad_done((pg, pb), outs, direct)
    finally:
        Y.DIRECT_GRADS[0] = prev
    assert not direct and fired == []
    for o, b, p in zip(outs, back, (pg, pb)):
        assert b is o and float(o[0]) == 7.0
        assert o.data_ptr() != getattr(p, '_ld_grad', p).data_ptr()
    if why == 'switch_off':  # the uses stay noted: autograd's hook completes them
        assert pg._ld_pending == 1 and pb._ld_pending == 1


def test_bn_rule_fresh_only_for_the_needed_ones():
    """BN: direct only when BOTH are needed and BOTH have a slice; otherwise
    fresh tensors for those needed alone."""
    pg, pb = _param(), _param()
    for needs in ((True, False), (False, True), (False, False)):
        outs, direct = Y._grad_outs((pg, pb), needs, _alloc)
        assert not direct
        for o, need, p in zip(outs, needs, (pg, pb)):
            assert (o is not None) == need
            assert o is None or o.data_ptr() != p._ld_grad.data_ptr()
        assert list(Y._grad_done((pg, pb), outs, direct)) == list(outs)


def test_gn_rule_fresh_for_both_whenever_not_direct():
    """GN: its kernels write both gradients, so both are allocated even when
    one is not needed; both are handed back."""
    pg, pb = _param(), _param()
    for needs in ((True, False), (False, True), (False, False)):
        outs, direct = Y._grad_outs((pg, pb), needs, _alloc, fresh_all=True)
        assert not direct and all(o is not None for o in outs)
        assert all(o.data_ptr() != p._ld_grad.data_ptr()
                   for o, p in zip(outs, (pg, pb)))
        assert list(Y._grad_done((pg, pb), outs, direct)) == list(outs)
    outs, direct = Y._grad_outs((pg, pb), (True, True), _alloc, fresh_all=True)
    assert direct and outs[0].data_ptr() == pg._ld_grad.data_ptr()


def test_quality_rule_all_four_or_none():
    fired = []
    ps = [_param(ready=fired) for _ in range(4)]
    Y._note_use(*ps)
    outs, direct = Y._grad_outs(ps, (True, ) * 4, torch.empty_like)
    assert direct and [o.data_ptr() for o in outs] == \
        [p._ld_grad.data_ptr() for p in ps]
    assert tuple(Y._grad_done(ps, outs, direct)) == (None, ) * 4
    assert len(fired) == 4
    # one of the four without a slice: none is direct, four fresh tensors,
    # nothing emitted, the other three stay noted
    del fired[:]
    ps[2] = _param(slice_=False)
    Y._note_use(*ps)
    outs, direct = Y._grad_outs(ps, (True, ) * 4, torch.empty_like)
    assert not direct and len(outs) == 4
    assert all(o is not None and o.data_ptr() != getattr(p, '_ld_grad', p).data_ptr()
               for o, p in zip(outs, ps))
    assert list(Y._grad_done(ps, outs, direct)) == list(outs) and fired == []
    assert [getattr(p, '_ld_pending', 0) for p in ps] == [1, 1, 0, 1]


def test_scale_levels_rule_slice_consulted_only_when_needed(monkeypatch):
    ps = _param()
    asked = []
    real = Y._sink
    monkeypatch.setattr(Y, '_sink', lambda p: (asked.append(p), real(p))[1])
    outs, direct = Y._grad_outs((ps, ), (False, ), _alloc)
    assert not direct and list(outs) == [None] and asked == []
    assert list(Y._grad_done((ps, ), outs, direct)) == [None]
    outs, direct = Y._grad_outs((ps, ), (True, ), _alloc)
    assert direct and asked == [ps]
    assert outs[0].data_ptr() == ps._ld_grad.data_ptr()


def test_single_parameter_rule_of_the_weight_gradients():
    """wgrad / gconv wgrad / conv bias: accumulate = 1 exactly when the
    parameter has a slice; the fresh tensor is returned otherwise."""
    fired = []
    pw = _param(ready=fired)
    Y._note_use(pw)
    (dw, ), direct = Y._grad_outs((pw, ), (True, ), _alloc)
    assert direct and dw.data_ptr() == pw._ld_grad.data_ptr()
    assert Y._grad_done((pw, ), (dw, ), direct)[0] is None and fired == [pw]
    # no parameter object at all (gconv_wgrad(pw=None), a conv without bias)
    (dw, ), direct = Y._grad_outs((None, ), (True, ), lambda p: torch.ones(3))
    assert not direct and Y._grad_done((None, ), (dw, ), direct)[0] is dw


def test_mixed_slices_pair_is_not_direct_and_stays_pending():
    """gamma has an arena slice, beta has none.  The code before the helpers
    (``direct = need_g and need_b and sg is not None and sb is not None`` in the
    BN and GN bodies) took the fresh-tensor path for BOTH and emitted NEITHER:
    gamma's noted use stays pending -- its bucket is completed by autograd's
    post-accumulate hook on the returned gradient, not by ``_emit`` -- and the
    ready callback does not fire from here."""
    fired = []
    pg, pb = _param(ready=fired), _param(slice_=False)
    Y._note_use(pg, pb)
    for fresh_all in (False, True):  # the BN and the GN bodies alike
        outs, direct = Y._grad_outs((pg, pb), (True, True), _alloc,
                                    fresh_all=fresh_all)
        assert not direct
        assert outs[0] is not None and outs[1] is not None
        assert outs[0].data_ptr() != pg._ld_grad.data_ptr()
        back = Y._grad_done((pg, pb), outs, direct)
        assert back[0] is outs[0] and back[1] is outs[1]
        assert fired == []
        assert pg._ld_pending == 1
        assert getattr(pb, '_ld_pending', 0) == 0
    assert float(pg._ld_grad.abs().sum()) == 0.0  # the slice was not written


# ---- the C8 predicates against the expressions they replaced -----------------
def _ref_c8w(need_w, cin, cout):
    return need_w and Y._PRECISION[0] == 'bf16' and \
        Y._C8[0] and Y._WGRAD_C8[0] and cin % 32 == 0 and cout % 32 == 0


def _ref_c8_dead(cin, cout, need_x):
    return Y._DRAW_C8_ONLY[0] and Y._PRECISION[0] == 'bf16' and Y._C8[0] and \
        Y._WGRAD_C8[0] and cin % 32 == 0 and cout % 32 == 0 and \
        (not need_x or Y._use_bf16(cout))


def _ref_lean(N, cin, cout, P):
    return Y._BN_LEAN[0] and Y._BN_BWD_C8[0] and \
        Y._PRECISION[0] == 'bf16' and Y._C8[0] and Y._WGRAD_C8[0] and \
        cin % 32 == 0 and cout % 32 == 0 and P % 2 == 0 and \
        N * ((P // (4 if P % 4 == 0 else 2) + 63) // 64) <= 256


def _ref_rows(N, P):
    return Y._BN_BWD_C8[0] and N * ((P // 4 + 63) // 64) <= 256


def test_c8_predicates_truth_table():
    cells = (Y._PRECISION, Y._C8, Y._WGRAD_C8, Y._DRAW_C8_ONLY, Y._BN_BWD_C8,
             Y._BN_LEAN)
    saved = [c[0] for c in cells]
    chans = (16, 32, 48, 64, 68)
    # N x P on both sides of the row limit: 256 rows of 64 x 4 (or 64 x 2)
    # positions -- P = 62..64 is one row per image, so N = 256 / 257 straddle
    # it; 128 / 129 do with two rows per image (P = 256 + 62..64 -> 318..320)
    geo = [(N, P) for N in (2, 256, 257) for P in (62, 63, 64)] + \
        [(N, 256 + P) for N in (128, 129) for P in (62, 63, 64)]
    n = 0
    try:
        for prec, c8, wc8, draw, bwd, lean in itertools.product(
                ('fp32', 'bf16'), *[(False, True)] * 5):
            Y._PRECISION[0] = prec
            for cell, v in zip(cells[1:], (c8, wc8, draw, bwd, lean)):
                cell[0] = v
            for cin, cout in itertools.product(chans, chans):
                for need in (False, True):
                    assert bool(need and Y._wgrad_takes_c8(cin, cout)) == \
                        bool(_ref_c8w(need, cin, cout))
                    assert bool(Y._draw_only_c8(cin, cout, need)) == \
                        bool(_ref_c8_dead(cin, cout, need))
                for N, P in geo:
                    assert bool(Y._bn_lean_geometry(N, cin, cout, P)) == \
                        bool(_ref_lean(N, cin, cout, P))
                    n += 1
            for N, P in geo:
                assert bool(Y._bn_c8_covers(N, P)) == bool(_ref_rows(N, P))
    finally:
        for c, v in zip(cells, saved):
            c[0] = v
    assert n == 64 * 25 * len(geo)
    # the table is not vacuous: both answers occur on each side of the limit
    prev = Y._BN_BWD_C8[0]
    Y._BN_BWD_C8[0] = True
    try:
        assert Y._bn_c8_covers(256, 64) and not Y._bn_c8_covers(257, 64)
        assert Y._bn_c8_covers(128, 320) and not Y._bn_c8_covers(129, 320)
    finally:
        Y._BN_BWD_C8[0] = prev
