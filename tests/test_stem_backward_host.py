"""Host tests of the trainable stem: the numpy restatement of the max-pool
backward (tests/_stem_ref64.py) equals torch's CPU backward bit for bit on the
case list the device test uses, the planted defects break that check, and the
refusals that need no device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stem_ref64 as S  # noqa: E402


def _breaks(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


def test_torch_tie_rule_on_a_constant_map():
    """A constant 5 x 6 map: output (0, 0) -> input (0, 0), output (0, 1) ->
    input (0, 1) (the first in-bounds element of each window)."""
    x = np.full((1, 5, 6), 2.0, dtype=np.float32)
    for (oh, ow), (h, w) in (((0, 0), (0, 0)), ((0, 1), (0, 1)),
                             ((1, 1), (1, 1)), ((2, 2), (3, 3))):
        dy = np.zeros((1, 3, 3), dtype=np.float32)
        dy[0, oh, ow] = 1.0
        for dx in (S.torch_backward(x, dy), S.maxpool_backward(x, dy)):
            assert dx[0, h, w] == 1.0 and dx.sum() == 1.0, (oh, ow, dx)


@pytest.mark.parametrize('kind', S.KINDS)
@pytest.mark.parametrize('rows', S.ROWS)
def test_restatement_equals_torch_bit_for_bit(rows, kind):
    for h, w in S.SHAPES:
        x, dy = S.pool_inputs(kind, rows, h, w)
        S.check_exact(S.maxpool_backward(x, dy), S.torch_backward(x, dy),
                      f'{kind} rows {rows} {h}x{w}')


def test_inputs_are_what_they_claim():
    x, _ = S.pool_inputs('relu', 3, 9, 20)
    assert (x == 0).mean() > 0.3 and (x > 0).any()  # ties are the normal case
    assert (S.pool_inputs('negative', 3, 9, 20)[0] < 0).all()
    inc = S.pool_inputs('increasing', 3, 9, 20)[0].ravel()
    assert (np.diff(inc) > 0).all()


@pytest.mark.parametrize('defect', [dict(route='last'), dict(pad_value=0.0)])
def test_planted_defect_breaks_the_check(defect):
    """Routing to the last maximum moves the gradient wherever a window has
    ties (the ReLU map); a zero padding wins every border window of an
    all-negative map and drops its gradient."""
    kind = 'relu' if 'route' in defect else 'negative'
    x, dy = S.pool_inputs(kind, 3, 8, 12)
    ref = S.torch_backward(x, dy)
    S.check_exact(S.maxpool_backward(x, dy), ref, 'correct')
    _breaks(S.check_exact, S.maxpool_backward(x, dy, **defect), ref, 'defect')
    # and the defect is invisible without ties / negative borders
    x, dy = S.pool_inputs('increasing', 3, 8, 12)
    S.check_exact(S.maxpool_backward(x, dy, **defect), S.torch_backward(x, dy),
                  'increasing map')


def test_trainable_stem_refuses_bf16_mode_before_any_launch():
    from ld_amd import layers as Y
    from ld_amd.resnet import ResNet
    net = ResNet(depth=18).train()
    assert net.frozen_stages == -1 and net.conv1.weight.requires_grad
    Y.set_precision('bf16')
    try:
        with pytest.raises(NotImplementedError,
                           match=r'set_precision\("fp32"\)'):
            net(torch.randn(1, 3, 32, 32))
        # a frozen stem and a no-grad forward are not this refusal's business:
        # they fail later, on the host tensor
        with torch.no_grad(), pytest.raises(Exception) as e:
            net(torch.randn(1, 3, 32, 32))
        assert not isinstance(e.value, NotImplementedError)
    finally:
        Y.set_precision('fp32')


def test_trainable_stem_in_fp32_mode_reaches_the_device_check():
    """The old refusal ('a trainable stem needs a max-pool backward') is gone:
    in fp32 mode a host tensor fails on the device requirement instead."""
    from ld_amd.resnet import ResNet
    net = ResNet(depth=18).train()
    with pytest.raises(Exception) as e:
        net(torch.randn(1, 3, 32, 32))
    assert not isinstance(e.value, NotImplementedError), e.value


def test_small_cin_weight_gradient_predicate_without_a_device():
    """Which geometries the flat kernel takes (host logic only)."""
    import ctypes as C
    from ld_amd import layers as Y
    from ld_amd import lib as L
    lib = L.get_lib()

    def ok(cin, cout, k, s, p, hw=(33, 47), levels=None):
        d, _ = Y.conv_desc(2, cin, cout, k, k, s, p, levels or (hw, ))
        return lib.ld_conv_wgrad_smallc_supported(C.byref(d))

    for cin, k, s, p, cout in ((3, 7, 2, 3, 64), (3, 3, 2, 1, 32),
                               (1, 7, 2, 3, 64), (4, 3, 2, 1, 64),
                               (15, 3, 2, 1, 64), (1, 12, 1, 0, 32)):
        assert ok(cin, cout, k, s, p) == 1, (cin, k, s, p, cout)
    assert ok(16, 64, 3, 1, 1) == 0          # Cin >= 16: the generic kernels
    assert ok(3, 128, 3, 1, 1) == 0          # Cout outside {32, 64}
    assert ok(4, 64, 7, 2, 3) == 0           # 196 > 160 flat rows
    assert ok(3, 64, 3, 1, 1, levels=((8, 8), (4, 4))) == 0  # one level only
    d, _ = Y.conv_desc(2, 3, 64, 7, 7, 2, 3, ((96, 160), ))
    slabs = lib.ld_conv_wgrad_smallc_slabs(C.byref(d))
    assert slabs >= 3
    assert lib.ld_conv_wgrad_smallc_workspace_bytes(C.byref(d)) == \
        slabs * 64 * 147 * 4
