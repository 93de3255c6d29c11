"""Shared by test_iou_losses_host.py and test_gpu_iou_losses.py: the row inputs
of tests/golden/iou_losses.npz and the project's bars for them."""
import numpy as np

LOSSES = ('iou', 'iou_linear', 'diou', 'ciou')
MODULE_CFG = {'iou': dict(type='IoULoss'),
              'iou_linear': dict(type='IoULoss', linear=True),
              'diou': dict(type='DIoULoss'), 'ciou': dict(type='CIoULoss')}
# what tests/test_gpu_modules.py applies to GIoULoss rows; the value atol is the
# fixture's ATOL_LOSS (tools/gen_golden_iou_losses.py states where it comes from)
LOSS_RTOL, LOSS_ATOL = 1e-5, 5e-7
GRAD_RTOL, GRAD_ATOL = 2e-4, 1e-7


def row_inputs(g):
    """(pred, target) float32 (257, 4): the stored hand-written rows, then the
    seeded ones."""
    from ld_amd import synthetic
    n, seed = (int(v) for v in g['rows_seed'])
    hand = g['rows_hand']
    jp, jt = synthetic.box_loss_rows(n - len(hand), seed)
    pred = np.concatenate([hand[:, 0], jp.numpy()]).astype(np.float32)
    target = np.concatenate([hand[:, 1], jt.numpy()]).astype(np.float32)
    return pred, target


def bars(g, name):
    """(loss rtol, grad rtol) against the float64 reference: the project's bar,
    or 4 x the reference's own stored fp32 deviation where that exceeds it."""
    dl = float(g[f'{name}_loss_ref32_dev'])
    dg = float(g[f'{name}_grad_ref32_dev'])
    return (LOSS_RTOL if dl <= LOSS_RTOL else 4 * dl,
            GRAD_RTOL if dg <= GRAD_RTOL else 4 * dg)
