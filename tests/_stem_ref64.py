"""Host restatement of the max-pool backward of the trainable stem
(ld_maxpool_3x3s2_backward) and the cases its tests share.

The rule (torch's, which the kernel states in its own words): the gradient of
an output element goes to the FIRST in-bounds element of its 3 x 3 window, in
row-major (kh, kw) order, that attains the maximum; the padding is -inf; the
addends of one input pixel are added in ascending (oh, ow) order in fp32.  The
result is exact: it must equal torch's CPU ``max_pool2d`` backward bit for bit.

``route`` / ``pad_value`` plant the two defects the tie-heavy inputs must
catch: routing to the LAST maximum, and padding with 0.
"""
import numpy as np
import torch
import torch.nn.functional as F

SHAPES = ((1, 1), (2, 2), (3, 3), (4, 8), (5, 6), (7, 9), (8, 12), (9, 20),
          (16, 16))
ROWS = (1, 3, 128)
KINDS = ('relu', 'const', 'increasing', 'negative')


def pool_inputs(kind, rows, h, w):
    """(x, dy) fp32 of one case: x as (rows, H, W), dy as (rows, Ho, Wo)."""
    rng = np.random.default_rng([KINDS.index(kind), rows, h, w])
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    if kind == 'relu':  # a ReLU output: full of zeros, ties everywhere
        x = np.maximum(rng.standard_normal((rows, h, w)), 0.0)
    elif kind == 'const':
        x = np.full((rows, h, w), 1.5)
    elif kind == 'increasing':
        x = np.arange(rows * h * w, dtype=np.float64).reshape(rows, h, w) / 8
    else:  # all negative: a zero padding would win every border window
        x = -np.abs(rng.standard_normal((rows, h, w))) - 0.5
    dy = rng.standard_normal((rows, ho, wo))
    return x.astype(np.float32), dy.astype(np.float32)


def maxpool_backward(x, dy, route='first', pad_value=-np.inf):
    """dx (rows, H, W) fp32 of MaxPool2d(3, 2, 1) by the rule above."""
    x = np.asarray(x, dtype=np.float32)
    dy = np.asarray(dy, dtype=np.float32)
    rows, h, w = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    assert dy.shape == (rows, ho, wo)
    xp = np.full((rows, h + 2, w + 2), pad_value, dtype=np.float32)
    xp[:, 1:h + 1, 1:w + 1] = x
    dxp = np.zeros((rows, h + 2, w + 2), dtype=np.float32)  # padding: dropped
    r = np.arange(rows)
    for oh in range(ho):
        for ow in range(wo):
            win = xp[:, 2 * oh:2 * oh + 3, 2 * ow:2 * ow + 3].reshape(rows, 9)
            if route == 'first':
                am = np.argmax(win, axis=1)  # the first of equal maxima
            else:
                am = 8 - np.argmax(win[:, ::-1], axis=1)
            dxp[r, 2 * oh + am // 3, 2 * ow + am % 3] += dy[:, oh, ow]
    return dxp[:, 1:h + 1, 1:w + 1].copy()


def torch_backward(x, dy):
    """torch's CPU fp32 backward of F.max_pool2d(x, 3, 2, 1)."""
    t = torch.from_numpy(np.array(x, dtype=np.float32)).requires_grad_(True)
    y = F.max_pool2d(t[None], 3, 2, 1)[0]
    y.backward(torch.from_numpy(np.array(dy, dtype=np.float32)))
    return t.grad.numpy()


def check_exact(got, ref, what=''):
    got = np.asarray(got, dtype=np.float32)
    ref = np.asarray(ref, dtype=np.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    same = got.view(np.uint32) == ref.view(np.uint32)
    if not same.all():
        i = tuple(int(v) for v in np.argwhere(~same)[0])
        raise AssertionError(f'{what}: {int((~same).sum())}/{same.size} '
                             f'elements differ; first at {i}: got {got[i]!r} '
                             f'ref {ref[i]!r}')
