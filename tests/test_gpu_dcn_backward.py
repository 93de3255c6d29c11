"""GPU tests (-m gpu) of the deformable-convolution backward (csrc/dcn.hip:
ld_deform_offset_grad, ld_deform_col2im_index / _sum; layers.DeformIm2colFn;
the trainable path of cnn.DeformConv2dPack) against the float64 autograd
restatement tests/_dcn_ref64.py.

Bands.  (F) "as good as fp32 can be": our worst error against float64 is at most
3 x the worst error of the same restatement evaluated in float32 on the CPU,
plus 5e-5 of max|g| (band (2) of tests/_gradcheck.py) -- used where the sampled
cells are provably the same in both formats (offsets on a 1/64 grid).  (1) of
_gradcheck: |got - ref| <= 1e-3 |ref| + 1e-3 max|ref| per element -- used where
the device computes the offsets itself in fp32.  (C) 2e-4 rel + 2e-5 of the
tensor scale, the band of test_dcn_forward_vs_oracle, between two device
results that differ in summation order only."""
import copy

import numpy as np
import pytest
import torch

import _dcn_ref64 as R
import _gradcheck as G
from ld_amd import synthetic

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _band_f(got, g64, g32, what):
    """Band (F), on every element."""
    got = got.detach().double().cpu()
    ours = float((got - g64).abs().max())
    theirs = float((g32.double() - g64).abs().max())
    am = float(g64.abs().max())
    print(f'{what}: ours {ours:.3e} fp32-cpu {theirs:.3e} max|g| {am:.3e}')
    assert am > 0
    assert ours <= 3.0 * theirs + 5e-5 * am, (what, ours, theirs, am)


def _band_1(got, ref, what):
    """Band (1), element-wise, no exclusions."""
    got = got.detach().double().cpu().reshape(-1)
    ref = ref.detach().double().cpu().reshape(-1)
    am = float(ref.abs().max())
    err = (got - ref).abs()
    tol = 1e-3 * ref.abs() + 1e-3 * am + 1e-30
    worst = float((err / tol).max())
    print(f'{what}: worst err/tol {worst:.3f}, max err {float(err.max()):.3e}, '
          f'max|ref| {am:.3e}')
    assert worst <= 1.0, (what, worst, int((err / tol).argmax()))


def _ratio_1(got, ref):
    """(worst err / band-(1) tolerance, worst err / max|ref|)."""
    got = got.detach().double().reshape(-1)
    ref = ref.detach().double().reshape(-1)
    am = float(ref.abs().max()) + 1e-30
    err = (got - ref).abs()
    tol = 1e-3 * ref.abs() + 1e-3 * am
    return float((err / tol).max()), float(err.max()) / am


def _close(got, ref, what, rtol=2e-4, atol_rel=2e-5):
    """Band (C)."""
    got = got.detach().double().cpu().numpy()
    ref = ref.detach().double().cpu().numpy()
    scale = float(np.abs(ref).max()) + 1e-30
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol_rel * scale,
                               err_msg=what)


# --------------------------------------------- 1 / 2: the sampling alone ---
SAMPLING = [(2, 5, 7, 11, 1), (1, 5, 9, 10, 2)]


def _sampling_reference(x, off, dcol, stride):
    """d_x, d_offset of the restatement in float64 and in float32 (CPU)."""
    out = []
    for dt in (torch.float64, torch.float32):
        a = x.detach().clone().to(dt).requires_grad_(True)
        b = off.detach().clone().to(dt).requires_grad_(True)
        col = R.deform_im2col(a, b, 3, stride, 1)
        col.backward(dcol.to(dt))
        out.append((col.detach(), a.grad, b.grad))
    return out


def _device_sampling(x, off, dcol, stride, dev):
    from ld_amd import layers as Y
    N, C, H, W = x.shape
    x3 = x.detach().float().reshape(N, C, H * W).to(dev).requires_grad_(True)
    o3 = off.detach().float().reshape(N, 18, -1).to(dev).requires_grad_(True)
    col = Y.DeformIm2colFn.apply(x3, o3, H, W, 3, stride, 1)
    col.backward(dcol.float().to(dev))
    torch.cuda.synchronize()
    return col.detach(), x3.grad.view(N, C, H, W), o3.grad.view(off.shape)


@pytest.mark.parametrize('N,C,H,W,stride', SAMPLING)
def test_sampling_gradients_vs_float64(N, C, H, W, stride):
    """DeformIm2colFn.backward on a random d_col, no GEMM.  Offsets on a 1/64
    grid in [-4, 4]: the coordinates are exact in fp32 and fp64, no floor can
    flip, so every element of d_x and d_offset is compared, in band (F)."""
    dev = _dev()
    g = torch.Generator().manual_seed(100 * H + W)
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64).float().double()
    off = R.grid_offsets((N, 18, Ho, Wo), g)
    # forced regions.  position (0, 0): offsets exactly 0 (integer coordinates;
    # its tap (0, 0) sits at (-1, -1), outside); position (0, 1): tap 0 at
    # h = -0.5; the last position: tap 8 half a cell above the bottom edge
    off[:, :, 0, 0] = 0.0
    off[:, 0, 0, 1], off[:, 1, 0, 1] = 0.5, 1.25
    off[:, 16, Ho - 1, Wo - 1], off[:, 17, Ho - 1, Wo - 1] = -0.5, -1.5
    py, px = R.sample_coords(off, H, W, 3, stride, 1)
    in_w = (px > -1) & (px < W)
    assert bool(((py > -1) & (py < 0) & in_w).any())
    assert bool(((py > H - 1) & (py < H) & in_w).any())
    assert bool(((py <= -1) | (py >= H) | (px <= -1) | (px >= W)).any())
    integer = (py == py.round()) & (px == px.round()) & (py >= 0) & \
        (py <= H - 1) & (px >= 0) & (px <= W - 1)
    assert int(integer[:, :, 0, 0].sum()) >= N * 4
    dcol = torch.randn(N, C * 9, Ho * Wo, generator=g,
                       dtype=torch.float64).float().double()
    (c64, dx64, do64), (c32, dx32, do32) = _sampling_reference(x, off, dcol,
                                                               stride)
    col, dx, doff = _device_sampling(x, off, dcol, stride, dev)
    _band_f(col, c64, c32, 'col')
    _band_f(dx, dx64, dx32, 'd_x')
    _band_f(doff, do64, do32, 'd_offset')
    # exactly zero where the sample is outside (-1, H) x (-1, W)
    outside = ((py <= -1) | (py >= H) | (px <= -1) | (px >= W))
    dsel = doff.cpu().view(N, 9, 2, Ho, Wo)
    assert float(dsel[:, :, 0][outside].abs().max()) == 0.0
    assert float(dsel[:, :, 1][outside].abs().max()) == 0.0


@pytest.mark.parametrize('N,C,H,W,stride', SAMPLING)
def test_data_gradient_reproducible_under_collisions(N, C, H, W, stride):
    """Every sample of an image lands in one 2x2 neighbourhood: four cells
    receive N*9*Pout contributions each (segments many chunks long, the
    degenerate case of the per-cell sum).  Two runs are bit-identical, and the
    result is in band (F) of float64."""
    dev = _dev()
    g = torch.Generator().manual_seed(7 * H + W + stride)
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64).float().double()
    zero = torch.zeros(N, 18, Ho, Wo, dtype=torch.float64)
    by, bx = R.sample_coords(zero, H, W, 3, stride, 1)
    fy = torch.randint(1, 64, by.shape, generator=g).double() / 64
    fx = torch.randint(1, 64, bx.shape, generator=g).double() / 64
    off = zero.clone()
    off[:, 0::2] = 3 + fy - by  # rows 3..4, columns 4..5
    off[:, 1::2] = 4 + fx - bx
    py, px = R.sample_coords(off, H, W, 3, stride, 1)
    assert bool(((py > 3) & (py < 4) & (px > 4) & (px < 5)).all())
    dcol = torch.randn(N, C * 9, Ho * Wo, generator=g,
                       dtype=torch.float64).float().double()
    (_, dx64, do64), (_, dx32, do32) = _sampling_reference(x, off, dcol, stride)
    _, dx_a, doff = _device_sampling(x, off, dcol, stride, dev)
    _, dx_b, _ = _device_sampling(x, off, dcol, stride, dev)
    assert torch.equal(dx_a, dx_b)
    touched = dx_a.cpu().abs().sum(dim=(0, 1)) > 0
    assert int(touched.sum()) == 4 and bool(touched[3:5, 4:6].all())
    _band_f(dx_a, dx64, dx32, 'd_x (collisions)')
    _band_f(doff, do64, do32, 'd_offset (collisions)')


# ------------------------------------------------- 3 / 4: the whole module ---
def _module(cin, cout, stride, g, oscale=None):
    from ld_amd.cnn import DeformConv2dPack
    m = DeformConv2dPack(cin, cout, 3, stride=stride, padding=1)
    with torch.no_grad():
        m.weight.copy_(torch.randn(m.weight.shape, generator=g) / (9 * cin)**0.5)
        if oscale is not None:
            m.conv_offset.weight.copy_(
                torch.randn(m.conv_offset.weight.shape, generator=g) * oscale /
                (9 * cin)**0.5)
            m.conv_offset.bias.copy_(torch.randn(18, generator=g) * 0.7)
    return m


def _module_reference(m, x, gy, stride, dt):
    """(y, dx, d weight, d conv_offset.weight, d conv_offset.bias, offset)."""
    ps = [p.detach().clone().to(dt).requires_grad_(True)
          for p in (m.weight, m.conv_offset.weight, m.conv_offset.bias)]
    a = x.detach().clone().to(dt).requires_grad_(True)
    y, off = R.dcn_pack_forward(a, ps[0], ps[1], ps[2], stride, 1)
    y.backward(gy.to(dt))
    return [y.detach(), a.grad] + [p.grad for p in ps] + [off.detach()]


def _module_device(m, x, gy, dev):
    N, C, H, W = x.shape
    m = copy.deepcopy(m).to(dev)
    x3 = x.reshape(N, C, H * W).to(dev).requires_grad_(True)
    y3, lv = m.forward3(x3, ((H, W), ))
    y3.backward(gy.reshape(N, gy.shape[1], -1).to(dev))
    torch.cuda.synchronize()
    (ho, wo), = lv
    return [y3.detach().view(N, -1, ho, wo), x3.grad.view(N, C, H, W),
            m.weight.grad, m.conv_offset.weight.grad, m.conv_offset.bias.grad]


@pytest.mark.parametrize('H,W,stride', [(20, 28, 1), (21, 27, 2)])
def test_zero_offsets_are_the_convolution(H, W, stride):
    """conv_offset at its zero init: y, weight.grad and the input gradient of the
    trainable DeformConv2dPack equal those of a cnn.Conv2d with the same weight
    on the device, band (C) -- except that the DCN's input gradient also
    carries the conv_offset path, which is exactly 0 here (zero conv_offset
    weights).  conv_offset's own gradients are NOT zero (the offset gradient is
    the forward difference of x) and match float64 in band (1): coordinates are
    exact integers on both sides, so the cells are the same, and these are the
    quantities test 4 holds to that band."""
    from ld_amd.cnn import Conv2d
    dev = _dev()
    g = torch.Generator().manual_seed(H * 31 + stride)
    N, cin, cout = 2, 128, 128
    x = torch.randn(N, cin, H, W, generator=g)
    m = _module(cin, cout, stride, g)
    ho, wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    gy = torch.randn(N, cout, ho, wo, generator=g)
    y, dx, dw, dow, dob = _module_device(m, x, gy, dev)
    c = Conv2d(cin, cout, 3, stride=stride, padding=1, bias=False).to(dev)
    with torch.no_grad():
        c.weight.copy_(m.weight)
    xc = x.reshape(N, cin, H * W).to(dev).requires_grad_(True)
    yc, _ = c.forward3(xc, ((H, W), ))
    yc.backward(gy.reshape(N, cout, -1).to(dev))
    torch.cuda.synchronize()
    _close(y.reshape(N, cout, -1), yc, 'y')
    _close(dw, c.weight.grad, 'weight.grad')
    _close(dx.reshape(N, cin, -1), xc.grad, 'input gradient')
    ref = _module_reference(m, x, gy, stride, torch.float64)
    assert float(ref[5].abs().max()) == 0.0
    assert float(dow.abs().max()) > 0 and float(dob.abs().max()) > 0
    _band_1(dow, ref[3], 'conv_offset.weight.grad')
    _band_1(dob, ref[4], 'conv_offset.bias.grad')


MODULE_CASES = [  # the first three DCN_CASES of tests/test_gpu_v2.py
    ('c3_like', 2, 128, 128, 20, 28, 1, 1.5),
    ('c3_first_s2', 1, 128, 128, 21, 27, 2, 2.0),
    ('c5_like', 2, 512, 512, 7, 11, 1, 4.0),
]


@pytest.mark.parametrize('case', MODULE_CASES, ids=[c[0] for c in MODULE_CASES])
def test_module_gradients_vs_float64(case):
    """Whole trainable module with offsets that leave the 3x3 window: y, the
    input gradient and all four parameter gradients against float64, band (1) on
    every element.  The device computes the offsets in fp32, so a sample within
    rounding of an integer coordinate could take the neighbouring cell; the seeds
    are fixed ones for which the restatement evaluated in fp32 on the CPU stays
    inside the same band (asserted here too)."""
    name, N, cin, cout, H, W, stride, oscale = case
    dev = _dev()
    g = torch.Generator().manual_seed(len(name) * 17 + cin + 1)
    x = torch.randn(N, cin, H, W, generator=g)
    m = _module(cin, cout, stride, g, oscale)
    ho, wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    gy = torch.randn(N, cout, ho, wo, generator=g)
    ref = _module_reference(m, x, gy, stride, torch.float64)
    assert float(ref[5].abs().max()) > 2.0
    cpu32 = _module_reference(m, x, gy, stride, torch.float32)
    names = ('y', 'input gradient', 'weight.grad', 'conv_offset.weight.grad',
             'conv_offset.bias.grad')
    for what, a, b in zip(names, cpu32, ref):
        _band_1(a, b, f'{name} fp32-cpu {what}')
    got = _module_device(m, x, gy, dev)
    for what, a, b in zip(names, got, ref):
        _band_1(a, b, f'{name} {what}')


# ------------------------------------------------------- 5: train steps ---
def _batch(dev):
    b = synthetic.synthetic_batch(2, (128, 150), (128, 160), [3, 2], 21)
    return dict(img=b['img'].to(dev), img_metas=b['img_metas'],
                gt_bboxes=[x.to(dev) for x in b['gt_bboxes']],
                gt_labels=[x.to(dev) for x in b['gt_labels']])


def _table(log_vars):
    return {k: float(log_vars[k]) for k in list(log_vars.keys())}


def _detectors(dev, weight_seed=1):
    """gfl_dcn_detector(101) with conv_offset zeroed and gfl_detector(101) on
    the same seeded weights."""
    from ld_amd import build_detector, model_zoo
    det = build_detector(model_zoo.gfl_dcn_detector(101))
    plain = build_detector(model_zoo.gfl_detector(101))
    sd = synthetic.seeded_state_dict(plain.state_dict(), seed=weight_seed)
    plain.load_state_dict(sd)
    missing = det.load_state_dict(sd, strict=False)
    assert all('conv_offset' in k for k in missing.missing_keys)
    assert len(missing.missing_keys) == 2 * (4 + 23 + 3)
    assert not missing.unexpected_keys
    for k, v in det.state_dict().items():
        if 'conv_offset' in k:
            v.zero_()
    det.to(dev).train()
    plain.to(dev).train()
    return det, plain


def _first_step_rows(det, plain, d):
    """One SGDTrainer step of both; -> [((err/tol, err/max|g|), name)] of every
    shared trainable parameter's gradient, worst first."""
    from ld_amd.train import SGDTrainer
    t1 = torch.stack([torch.stack(v) for v in det(**d).values()])
    t0 = torch.stack([torch.stack(v) for v in plain(**d).values()])
    np.testing.assert_allclose(t1.detach().cpu().numpy(),
                               t0.detach().cpu().numpy(), rtol=2e-4, atol=2e-5)
    tr, tp = SGDTrainer(det, lr=0.0025), SGDTrainer(plain, lr=0.0025)
    tr.check_grads = tp.check_grads = True  # every parameter gets its gradient
    o1, o0 = tr.step(d), tp.step(d)
    torch.cuda.synchronize()
    t1, t0 = _table(o1['log_vars']), _table(o0['log_vars'])
    assert t1.keys() == t0.keys()
    for k in t0:
        np.testing.assert_allclose(t1[k], t0[k], rtol=2e-4, atol=2e-5,
                                   err_msg=k)
    pp = dict(plain.named_parameters())
    rows = []
    for k, p in det.named_parameters():
        assert bool(torch.isfinite(p).all()), k
        if 'conv_offset' in k:
            assert float(p.detach().abs().max()) > 0, k  # it has moved
            continue
        if not p.requires_grad:
            assert torch.equal(p, pp[k]), k
            continue
        rows.append((_ratio_1(p.grad, pp[k].grad), k))
        _band_1(p, pp[k], 'param ' + k)
    rows.sort(reverse=True)
    return tr, rows


N_TWINS = 2


def _rounding_twin_grads(dev, d, seed, weight_seed=1):
    """The gradients of one SGDTrainer step of gfl_detector(101) whose 30 c3-c5
    conv2 weights -- the layers the DCN net computes another way -- are each
    multiplied by (1 + 2^-23 randn): a K-term dot product then moves by about
    sqrt(K) 2^-23 of a term, the size of a change of fp32 summation order
    (im2col + GEMM against the direct conv).  What this does to the plain
    net's gradients is the reference's own error for this comparison."""
    from ld_amd import build_detector, model_zoo
    from ld_amd.train import SGDTrainer
    twin = build_detector(model_zoo.gfl_detector(101))
    sd = synthetic.seeded_state_dict(twin.state_dict(), seed=weight_seed)
    g = torch.Generator().manual_seed(seed)
    n = 0
    for k, v in sd.items():
        if k.endswith('conv2.weight') and k.split('.')[1] in ('layer2', 'layer3',
                                                              'layer4'):
            v.mul_(1 + 2.0**-23 * torch.randn(v.shape, generator=g))
            n += 1
    assert n == 30
    twin.load_state_dict(sd)
    twin.to(dev).train()
    tr = SGDTrainer(twin, lr=0.0025)
    tr.check_grads = True
    tr.step(d)
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in twin.named_parameters()
            if p.requires_grad}


def test_first_train_step_is_the_plain_gfl_step():
    """gfl_dcn_detector(101) with conv_offset zeroed against gfl_detector(101) on
    the same seeded weights, one SGDTrainer.step each: loss tables in band (C),
    every updated parameter in band (1), conv_offset has moved, all finite.

    On top of that every element of every shared GRADIENT is compared.  The two
    nets differ in fp32 summation order in 30 layers, so behind them a ReLU
    input within rounding of 0 takes the other branch in one of them, and the
    gradients that element feeds move by one element's worth
    (tests/_gradcheck.py).  As there, the bulk is held to the tight band (1) --
    all but at most MAX_OUTLIERS parameters.  How far an outlier may go is NOT
    _gradcheck's OUTLIER_REL: that constant was sized on 256 sampled elements
    per parameter at the golden step's shape, and does not carry over to every
    element at 2 x 128 x 160, where P5-P7 are maps of 20, 6 and 2 positions and
    one position is percents of a sum.  It is the reference's own error at this
    shape, measured here: N_TWINS plain nets with the same 30 layers perturbed
    at rounding level (_rounding_twin_grads) against the plain net; our worst
    outlier is at most 3 x theirs + 5e-5 max|g|, the form of band (2) of
    _gradcheck.  (Measured once before this bound: 309 of 311 parameters inside
    the tight band, worst 0.44 of the tolerance, every backbone gradient within
    0.22; neck.fpn_convs.2.conv.weight / .bias 4.05e-3 / 3.61e-3 of max|g|.)"""
    dev = _dev()
    det, plain = _detectors(dev)
    n_dcn = sum(1 for k, p in det.named_parameters()
                if k.endswith('conv_offset.weight') and p.requires_grad)
    assert n_dcn == 30
    d = _batch(dev)
    _, rows = _first_step_rows(det, plain, d)
    print('worst gradients (err/tol, err/max|g|, name):', rows[:8])
    ref = {k: p.grad for k, p in plain.named_parameters() if p.requires_grad}
    theirs = 0.0
    for seed in range(N_TWINS):
        tw = _rounding_twin_grads(dev, d, 50 + seed)
        trows = sorted(((_ratio_1(tw[k], g), k) for k, g in ref.items()),
                       reverse=True)
        print(f'rounding twin {seed} vs plain, worst:', trows[:4])
        theirs = max(theirs, max(e for (_, e), _ in trows))
    ours = max(e for (_, e), _ in rows)
    print(f'worst err/max|g|: ours {ours:.3e}, the twins {theirs:.3e}')
    assert sum(1 for (r, _), _ in rows if r > 1.0) <= G.MAX_OUTLIERS, rows[:8]
    assert ours <= 3.0 * theirs + 5e-5, (ours, theirs, rows[:8])


def test_train_steps_with_offsets_reproducible_and_frozen_path():
    """Steps with non-zero offsets stay finite; the same backward twice from the
    same state leaves bit-identical arena gradients; and a fully frozen DCN
    backbone (the config-4 teacher's use) gives the same bits with grad mode on
    as under no_grad: the inference path did not move."""
    from ld_amd import build_detector, model_zoo
    from ld_amd.train import SGDTrainer
    dev = _dev()
    det, _ = _detectors(dev)
    d = _batch(dev)
    with torch.no_grad():
        for k, p in det.named_parameters():
            if k.endswith('conv_offset.bias'):
                p.fill_(0.6)
    tr = SGDTrainer(det, lr=0.0025)
    tr.check_grads = True
    for _ in range(2):
        out = tr.step(d)
        assert np.isfinite(float(out['loss']))
    for k, p in det.named_parameters():
        assert bool(torch.isfinite(p).all()), k
    grads = []
    for _ in range(2):
        tr.arena.zero_grad()
        loss, _ = det._parse_losses(det(**d))
        loss.backward()
        tr.arena.finish()
        torch.cuda.synchronize()
        grads.append(tr.arena.flat_grad.clone())
    assert float(grads[0].abs().max()) > 0
    assert torch.equal(grads[0], grads[1])
    bb = build_detector(model_zoo.gfl_dcn_detector(101)).backbone
    bb.load_state_dict(det.backbone.state_dict())
    bb.to(dev).requires_grad_(False).eval()
    with torch.no_grad():
        ya = bb(d['img'])
    yb = bb(d['img'])
    assert all(not t.requires_grad for t in yb)
    for a, b in zip(ya, yb):
        assert torch.equal(a, b)


def test_trainable_dcn_refusals():
    from ld_amd import layers as Y
    from ld_amd.cnn import DeformConv2dPack
    dev = _dev()
    x3 = torch.randn(1, 64, 6 * 7, device=dev).requires_grad_(True)
    lv = ((6, 7), )
    grouped = DeformConv2dPack(64, 64, 3, padding=1, groups=16).to(dev)
    with pytest.raises(NotImplementedError, match='grouped DCN'):
        grouped.forward3(x3, lv)
    with torch.no_grad():
        grouped.forward3(x3, lv)  # still runs frozen
    m = DeformConv2dPack(64, 64, 3, padding=1).to(dev)
    c8 = Y.C8Act(torch.zeros(1, 8, 42, 8, dtype=torch.bfloat16, device=dev),
                 (1, 64, 42))
    with pytest.raises(NotImplementedError, match='C8'):
        m.forward3(c8, lv)
    ghost = Y._image_only_output((1, 64, 42), c8.buf)  # what trunk_c8_scope leaves
    with pytest.raises(NotImplementedError, match='C8'):
        m.forward3(ghost, lv)
    with pytest.raises(NotImplementedError, match='deform_groups'):
        DeformConv2dPack(64, 64, 3, padding=1, deform_groups=2)
    with pytest.raises(NotImplementedError, match='dilated'):
        DeformConv2dPack(64, 64, 3, padding=2, dilation=2)
    # the folded-epilogue entry point stays inference-only
    s = torch.ones(64, device=dev)
    with pytest.raises(NotImplementedError, match='forward3_bn'):
        m.forward3_fused(x3, lv, s, s, None, True)
    y3, _ = m.forward3(x3, lv)
    y3.sum().backward()
    assert x3.grad is not None and m.conv_offset.bias.grad is not None
