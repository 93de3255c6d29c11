"""The IoU / DIoU / CIoU box losses of ld_amd/csrc/ld_math.h compiled for the
host (tests/host_harness_iou.cpp) against the reference's own float64 run on all
257 rows of tests/golden/iou_losses.npz, and the registry / head plumbing that
needs no GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _iou_losses as IL  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP = C.POINTER(C.c_float)


@pytest.fixture(scope='module')
def hh():
    out_dir = os.path.join(REPO, 'tests', '_build')
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, 'libhost_harness_iou.so')
    src = os.path.join(REPO, 'tests', 'host_harness_iou.cpp')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-ffp-contract=off',
                           '-shared', '-fPIC', src, '-o', so])
    lib = C.CDLL(so)
    lib.h_box_loss_rows.restype = None
    lib.h_box_loss_rows.argtypes = [C.c_int, FP, FP, C.c_int, C.c_float, FP,
                                    FP, FP]
    return lib


def _run(hh, mode, pred, target, eps=1e-6):
    n = len(pred)
    loss, iou = np.empty(n, np.float32), np.empty(n, np.float32)
    grad = np.empty((n, 4), np.float32)
    pred, target = np.ascontiguousarray(pred), np.ascontiguousarray(target)
    hh.h_box_loss_rows(mode, pred.ctypes.data_as(FP),
                       target.ctypes.data_as(FP), n, eps,
                       loss.ctypes.data_as(FP), iou.ctypes.data_as(FP),
                       grad.ctypes.data_as(FP))
    return loss, iou, grad


@pytest.mark.parametrize('name', IL.LOSSES)
def test_rows_vs_float64_reference(hh, golden, name):
    g = golden['iou_losses']
    pred, target = IL.row_inputs(g)
    assert pred.shape == (257, 4)
    loss, iou, grad = _run(hh, IL.LOSSES.index(name), pred, target)
    l_rtol, g_rtol = IL.bars(g, name)
    el = np.abs(loss - g[f'{name}_loss64'])
    eg = np.abs(grad - g[f'{name}_grad64'])
    print(name, 'max |loss err|', el.max(), 'max |grad err|', eg.max(),
          'bars', l_rtol, g_rtol)
    np.testing.assert_allclose(loss, g[f'{name}_loss64'], rtol=l_rtol,
                               atol=IL.LOSS_ATOL)
    np.testing.assert_allclose(grad, g[f'{name}_grad64'], rtol=g_rtol,
                               atol=IL.GRAD_ATOL)
    # the IoU handed to the QFL quality target is bbox_overlaps' own
    import ld_oracle as O
    ref_iou = np.array([O.bbox_overlaps(p[None], t[None])[0, 0]
                        for p, t in zip(pred, target)])
    np.testing.assert_allclose(iou, ref_iou, rtol=1e-6, atol=1e-7)


def test_clamped_iou_has_no_gradient(hh):
    """iou_loss.py:31: below the module's eps the IoU is clamped, so the value
    is -log(eps) (1 - eps when linear) and nothing flows back."""
    pred = np.array([[10., 10., 20., 20.]], np.float32)
    target = np.array([[30., 35., 50., 60.]], np.float32)
    for mode, want in ((0, -np.log(np.float32(1e-3))), (1, 1 - 1e-3)):
        loss, _, grad = _run(hh, mode, pred, target, eps=1e-3)
        np.testing.assert_allclose(loss[0], want, rtol=1e-6)
        assert not grad.any()


def test_modules_registered_with_reference_arguments():
    import torch
    from ld_amd import build_loss
    from ld_amd.losses import bbox_loss_mode
    m = build_loss(dict(type='DIoULoss'))
    assert (m.eps, m.reduction, m.loss_weight) == (1e-6, 'mean', 1.0)
    m = build_loss(dict(type='IoULoss', linear=True, eps=1e-5,
                        reduction='sum', loss_weight=0.5))
    assert (m.linear, m.eps, m.reduction, m.loss_weight) == \
        (True, 1e-5, 'sum', 0.5)
    m = build_loss(dict(type='CIoULoss', eps=1e-7, reduction='none',
                        loss_weight=2.0))
    assert (m.eps, m.reduction, m.loss_weight) == (1e-7, 'none', 2.0)
    want = {'GIoULoss': 'giou', 'IoULoss': 'iou', 'DIoULoss': 'diou',
            'CIoULoss': 'ciou'}
    for typ, mode in want.items():
        assert bbox_loss_mode(build_loss(dict(type=typ))) == mode
    assert bbox_loss_mode(build_loss(dict(type='IoULoss', linear=True))) == \
        'iou_linear'
    assert bbox_loss_mode(build_loss(dict(type='SmoothL1Loss'))) is None
    # nothing the reference accepts is refused: what remains is the data
    # contract of every row loss here (float32 device tensors, no CPU path)
    p = torch.zeros(2, 4)
    for typ in ('IoULoss', 'DIoULoss', 'CIoULoss'):
        with pytest.raises(Exception) as e:
            build_loss(dict(type=typ))(p, p, weight=torch.ones(2, 4),
                                       avg_factor=2.0,
                                       reduction_override='sum')
        assert not isinstance(e.value, (NotImplementedError, TypeError)), typ


def test_make_hp_box_loss_field():
    from ld_amd import lib as L, lossblock as LB
    assert LB.make_hp().flags == 0  # GIoU: the flags word is unchanged
    for mode, code in L.LD_LOSS_BBOX_MODES.items():
        hp = LB.make_hp(flags=L.LD_LOSS_ATSS | L.LD_LOSS_FCOS, bbox_loss=mode)
        assert hp.flags >> L.LD_LOSS_BBOX_SHIFT == code
        assert hp.flags & 0xff == L.LD_LOSS_ATSS | L.LD_LOSS_FCOS
    with pytest.raises(ValueError):
        LB.make_hp(bbox_loss='bounded_iou')


def _gfl_head(loss_bbox):
    from ld_amd import build_head
    from ld_amd.config import ConfigDict
    return build_head(dict(
        type='GFLHead', num_classes=20, in_channels=256, loss_bbox=loss_bbox,
        train_cfg=ConfigDict(assigner=dict(type='ATSSAssigner', topk=9),
                             allowed_border=-1, pos_weight=-1, debug=False),
        test_cfg=None))


def test_heads_accept_the_four_box_losses_only():
    from ld_amd import lib as L
    for cfg, code in ((dict(type='GIoULoss'), 0), (dict(type='IoULoss'), 1),
                      (dict(type='IoULoss', linear=True), 2),
                      (dict(type='DIoULoss'), 3),
                      (dict(type='CIoULoss', eps=1e-7), 4)):
        head = _gfl_head(dict(loss_weight=2.0, **cfg))
        head._check_loss_cfg()
        hp = head._hp()
        assert hp.flags >> L.LD_LOSS_BBOX_SHIFT == code
        assert hp.giou_eps == np.float32(cfg.get('eps', 1e-6))
    head = _gfl_head(dict(type='SmoothL1Loss'))
    with pytest.raises(NotImplementedError,
                       match='QualityFocalLoss \\+ one of the box losses '
                       'giou, iou, iou_linear, diou, ciou '):
        head._check_loss_cfg()
