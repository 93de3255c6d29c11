"""GPU (-m gpu): DeltaXYWHBBoxCoder.encode / decode (ld_delta_encode_rows /
ld_delta_decode_rows) on the 257 rows of synthetic.delta_coder_rows() -- two
128-thread blocks and one row; degenerate 1-pixel anchors, deltas beyond the
wh_ratio_clip clamp on both sides, boxes crossing max_shape, the means / stds of
the ATSS and RetinaNet configs -- against the reference's own rows
(tests/golden/plain_heads.npz), and the L1Loss / SmoothL1Loss modules (ld_l1_rows
/ ld_smooth_l1_rows) against a float64 evaluation.

Before the feature the coder raised NotImplementedError, L1Loss was not
registered and SmoothL1Loss.forward raised."""
import os

import numpy as np
import pytest
import torch

from ld_amd import synthetic as S

import _delta_coder as DC

pytestmark = pytest.mark.gpu

# fp32 rows: the same operations in the same order as the reference's; expf /
# logf of the device and of the reference's CPU run are each within an ulp or
# two of the true value, a corner is centre -+ size / 2 -> a few ulp (6e-8 each)
# of the row's largest coordinate.  1e-6 is the bound the host test puts on the
# numpy restatement for the same reason.
CODER_RTOL = 1e-6


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                'golden', 'plain_heads.npz'))


def _coder(name, **kw):
    from ld_amd.registry import build_bbox_coder
    means, stds = S.PLAIN_CODERS[name]
    return build_bbox_coder(dict(type='DeltaXYWHBBoxCoder',
                                 target_means=means, target_stds=stds, **kw))


@pytest.mark.parametrize('name', ['atss', 'retina'])
def test_coder_rows_vs_reference(name, gold):
    dev = torch.device('cuda:0')
    anchors, gts, deltas = [t.to(dev) for t in S.delta_coder_rows()]
    assert anchors.shape[0] == 257
    coder = _coder(name)
    enc = coder.encode(anchors, gts).cpu().numpy()
    dec = coder.decode(anchors, deltas).cpu().numpy()
    clip = coder.decode(anchors, deltas,
                        max_shape=S.DELTA_MAX_SHAPE).cpu().numpy()
    clip_t = coder.decode(anchors, deltas,
                          max_shape=torch.tensor(S.DELTA_MAX_SHAPE)
                          ).cpu().numpy()
    noclip = _coder(name, clip_border=False).decode(
        anchors, deltas, max_shape=S.DELTA_MAX_SHAPE).cpu().numpy()
    worst = {}
    for key, got in (('enc', enc), ('dec', dec)):
        ok, worst[key] = DC.close_rows(got, gold[f'coder_{name}_{key}'],
                                       CODER_RTOL)
        print(f'coder {name} {key}: worst ratio {worst[key]:.3g}')
        assert ok, (key, worst[key])
    # the clip: exact where it cut, elsewhere the unclipped row's error scale
    want = gold[f'coder_{name}_dec_clip'].astype(np.float64)
    scale = np.abs(gold[f'coder_{name}_dec']).max(-1, keepdims=True)
    ratio = np.abs(clip - want) / scale
    print(f'coder {name} dec_clip: worst ratio {ratio.max():.3g}')
    assert (ratio <= CODER_RTOL).all()
    h, w = S.DELTA_MAX_SHAPE[:2]
    assert clip.min() == 0.0 and clip[:, 0::2].max() == w and \
        clip[:, 1::2].max() == h
    assert np.array_equal(clip, clip_t)
    assert np.array_equal(noclip, dec)  # clip_border=False ignores max_shape
    # the numpy restatement agrees as well (a second opinion on the rows the
    # clamp cut: they sit at exp(+-max_ratio) exactly)
    means, stds = S.PLAIN_CODERS[name]
    ok, _ = DC.close_rows(dec, DC.delta2bbox(anchors.cpu().numpy(),
                                             deltas.cpu().numpy(), means,
                                             stds), CODER_RTOL)
    assert ok
    # zero rows: nothing is launched
    assert coder.encode(anchors[:0], gts[:0]).shape == (0, 4)


def _ref64(pred, target, weight, beta):
    d = (pred.double() - target.double())
    a = d.abs()
    if beta is None:
        loss, grad = a, torch.sign(d)
    else:
        loss = torch.where(a < beta, 0.5 * a * a / beta, a - 0.5 * beta)
        grad = torch.where(a < beta, d / beta, torch.sign(d))
    if weight is not None:
        loss, grad = loss * weight.double(), grad * weight.double()
    return loss, grad


@pytest.mark.parametrize('beta', [None, 1.0, 1.0 / 9.0],
                         ids=['l1', 'smooth_b1', 'smooth_b1/9'])
def test_l1_and_smooth_l1_modules(beta):
    """Values and gradients against float64 at the tolerance
    tests/test_gpu_modules.py applies to the GIoU module: values rtol 1e-5,
    gradients rtol 2e-4 / atol 1e-7.  |x| = beta exactly, an ulp on either side
    of it, zero, and 257 * 4 seeded elements."""
    from ld_amd import build_loss
    dev = torch.device('cuda:0')
    b32 = np.float32(1.0 if beta is None else beta)
    edge = np.array([b32, np.nextafter(b32, np.float32(0)),
                     np.nextafter(b32, np.float32(2)), -b32,
                     -np.nextafter(b32, np.float32(0)),
                     -np.nextafter(b32, np.float32(2)), 0.0, 0.5 * b32],
                    dtype=np.float32)
    gen = torch.Generator().manual_seed(5)
    pred = torch.cat([torch.from_numpy(edge).reshape(2, 4),
                      (torch.rand(257, 4, generator=gen) - 0.5) * 3.0])
    target = torch.cat([torch.zeros(2, 4),
                        (torch.rand(257, 4, generator=gen) - 0.5) * 3.0])
    weight = torch.rand(259, 4, generator=gen)
    weight[5] = 0.0
    cfg = dict(type='L1Loss', loss_weight=1.5) if beta is None else \
        dict(type='SmoothL1Loss', beta=beta, loss_weight=1.5)
    mod = build_loss(cfg)
    # the kernel takes beta as a float32
    beta64 = None if beta is None else float(np.float32(beta))
    for w, avg in ((None, None), (weight, None), (weight, 37.0),
                   (None, 11.0)):
        p = pred.to(dev).requires_grad_(True)
        wd = None if w is None else w.to(dev)
        rows = mod(p, target.to(dev), weight=wd, reduction_override='none')
        l64, g64 = _ref64(pred, target, w, beta64)
        assert rows.shape == pred.shape
        np.testing.assert_allclose(rows.detach().cpu().numpy(),
                                   1.5 * l64.numpy(), rtol=1e-5, atol=1e-12)
        loss = mod(p, target.to(dev), weight=wd, avg_factor=avg)
        denom = avg if avg is not None else pred.numel()
        np.testing.assert_allclose(float(loss), 1.5 * float(l64.sum()) / denom,
                                   rtol=1e-5)
        loss.backward()
        np.testing.assert_allclose(p.grad.cpu().numpy(),
                                   1.5 * g64.numpy() / denom, rtol=2e-4,
                                   atol=1e-7)
    s = mod(pred.to(dev), target.to(dev), reduction_override='sum')
    np.testing.assert_allclose(float(s),
                               1.5 * float(_ref64(pred, target, None,
                                                  beta64)[0].sum()),
                               rtol=1e-5)
    # the edge rows took the branch the reference's `diff < beta` takes
    if beta is not None:
        p = pred[:2].to(dev).requires_grad_(True)
        mod(p, target[:2].to(dev), reduction_override='sum').backward()
        g = p.grad.cpu().numpy().reshape(-1) / 1.5
        assert g[0] == 1.0 and g[2] == 1.0 and g[3] == -1.0 and g[5] == -1.0
        assert 0.0 < g[1] < 1.0 and -1.0 < g[4] < 0.0 and g[6] == 0.0
    assert float(mod(pred[:0].to(dev), target[:0].to(dev))) == 0.0
