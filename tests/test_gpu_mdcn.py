"""GPU tests (-m gpu) of modulated deformable convolution, DCNv2 (csrc/dcn.hip:
ld_mdeform_im2col, ld_mdeform_offset_mask_grad, ld_mdeform_col2im_index;
layers.ModulatedDeformIm2colFn; cnn.ModulatedDeformConv2dPack; the zoo's
gfl_dcnv2_detector / ld_r101_dcnv2_detector) against the float64 autograd
restatement tests/_mdcn_ref64.py.

Bands, exactly those of tests/test_gpu_dcn_backward.py.  (F) "as good as fp32
can be": our worst error against float64 is at most 3 x the worst error of the
same restatement evaluated in float32 on the CPU, plus 5e-5 of max|g| -- used
where the sampled cells are provably the same in both formats (offsets on a
1/64 grid).  (1): |got - ref| <= 1e-3 |ref| + 1e-3 max|ref| per element -- used
where the device computes the offsets itself in fp32.  (C) 2e-4 rel + 2e-5 of
the tensor scale, between two device results that differ in summation order
only.  No element is excluded from any comparison."""
import copy

import numpy as np
import pytest
import torch

import _dcn_ref64 as R
import _mdcn_ref64 as M
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


def _close(got, ref, what, rtol=2e-4, atol_rel=2e-5):
    """Band (C)."""
    got = got.detach().double().cpu().numpy()
    ref = ref.detach().double().cpu().numpy()
    scale = float(np.abs(ref).max()) + 1e-30
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol_rel * scale,
                               err_msg=what)


# ------------------------------------------------ 1 - 3: the sampling alone ---
SAMPLING = [(2, 5, 7, 11, 1), (1, 5, 9, 10, 2)]


def _out_hw(H, W, stride):
    return (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1


def _sampling_reference(x, om, dcol, stride):
    """(col, d_x, d_om) of the restatement in float64 and in float32 (CPU)."""
    out = []
    for dt in (torch.float64, torch.float32):
        a = x.detach().clone().to(dt).requires_grad_(True)
        b = om.detach().clone().to(dt).requires_grad_(True)
        col = M.modulated_im2col(a, b, 3, stride, 1)
        col.backward(dcol.to(dt))
        out.append((col.detach(), a.grad, b.grad))
    return out


def _device_sampling(x, om, dcol, stride, dev):
    from ld_amd import layers as Y
    N, C, H, W = x.shape
    x3 = x.detach().float().reshape(N, C, H * W).to(dev).requires_grad_(True)
    o3 = om.detach().float().reshape(N, 27, -1).to(dev).requires_grad_(True)
    col = Y.ModulatedDeformIm2colFn.apply(x3, o3, H, W, 3, stride, 1)
    col.backward(dcol.float().to(dev))
    torch.cuda.synchronize()
    return col.detach(), x3.grad.view(N, C, H, W), o3.grad.view(om.shape)


def _logits(shape, gen):
    """Mask logits in [-4, 4], exact in fp32."""
    return (torch.rand(shape, generator=gen, dtype=torch.float64) * 8 -
            4).float().double()


@pytest.mark.parametrize('N,C,H,W,stride', SAMPLING)
def test_sampling_and_gradients_vs_float64(N, C, H, W, stride):
    """ld_mdeform_im2col and ModulatedDeformIm2colFn.backward on a random d_col,
    no GEMM.  Offsets on the 1/64 grid with v1's three forced regions; logits
    random in [-4, 4] with a +30 row (mask 1) and a -30 row (mask ~ 1e-13).
    col, d_x, d_offset and d_logit: every element in band (F)."""
    dev = _dev()
    g = torch.Generator().manual_seed(100 * H + W)
    Ho, Wo = _out_hw(H, W, stride)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64).float().double()
    om = torch.empty(N, 27, Ho, Wo, dtype=torch.float64)
    off = R.grid_offsets((N, 18, Ho, Wo), g)
    # v1's forced regions.  position (0, 0): offsets exactly 0 (integer
    # coordinates; its tap (0, 0) sits at (-1, -1), outside); position (0, 1):
    # tap 0 at h = -0.5; the last position: tap 8 half a cell above the bottom
    off[:, :, 0, 0] = 0.0
    off[:, 0, 0, 1], off[:, 1, 0, 1] = 0.5, 1.25
    off[:, 16, Ho - 1, Wo - 1], off[:, 17, Ho - 1, Wo - 1] = -0.5, -1.5
    om[:, :18] = off
    om[:, 18:] = _logits((N, 9, Ho, Wo), g)
    om[:, 18:, 1, :] = 30.0
    om[:, 18:, 2, :] = -30.0
    assert float(torch.sigmoid(om[:, 18:, 1]).min()) > 1 - 1e-12
    assert 0 < float(torch.sigmoid(om[:, 18:, 2]).max()) < 1e-12
    py, px = R.sample_coords(off, H, W, 3, stride, 1)
    in_w = (px > -1) & (px < W)
    assert bool(((py > -1) & (py < 0) & in_w).any())
    assert bool(((py > H - 1) & (py < H) & in_w).any())
    outside = (py <= -1) | (py >= H) | (px <= -1) | (px >= W)
    assert bool(outside.any())
    integer = (py == py.round()) & (px == px.round()) & (py >= 0) & \
        (py <= H - 1) & (px >= 0) & (px <= W - 1)
    assert int(integer[:, :, 0, 0].sum()) >= N * 4
    # the 1/64 grid: fp32 and fp64 see the same coordinates, hence the same cells
    py32, px32 = R.sample_coords(off.float(), H, W, 3, stride, 1)
    assert torch.equal(py32.double(), py) and torch.equal(px32.double(), px)
    dcol = torch.randn(N, C * 9, Ho * Wo, generator=g,
                       dtype=torch.float64).float().double()
    (c64, dx64, do64), (c32, dx32, do32) = _sampling_reference(x, om, dcol,
                                                               stride)
    col, dx, dom = _device_sampling(x, om, dcol, stride, dev)
    _band_f(col, c64, c32, 'col')
    _band_f(dx, dx64, dx32, 'd_x')
    _band_f(dom[:, :18], do64[:, :18], do32[:, :18], 'd_offset')
    _band_f(dom[:, 18:], do64[:, 18:], do32[:, 18:], 'd_logit')
    # exactly zero where the sample is outside (-1, H) x (-1, W)
    dom = dom.cpu()
    dsel = dom[:, :18].reshape(N, 9, 2, Ho, Wo)
    assert float(dsel[:, :, 0][outside].abs().max()) == 0.0
    assert float(dsel[:, :, 1][outside].abs().max()) == 0.0
    assert float(dom[:, 18:][outside].abs().max()) == 0.0
    assert float(col.cpu().view(N, C, 9, Ho, Wo).permute(0, 2, 3, 4, 1)
                 [outside].abs().max()) == 0.0


@pytest.mark.parametrize('N,C,H,W,stride', SAMPLING)
def test_data_gradient_reproducible_under_collisions(N, C, H, W, stride):
    """v1's construction -- every sample of an image lands in one 2x2
    neighbourhood, so four cells receive N*9*Pout contributions each -- with
    random logits.  Two runs are bit-identical, exactly four cells are touched,
    and the result is in band (F) of float64."""
    dev = _dev()
    g = torch.Generator().manual_seed(7 * H + W + stride)
    Ho, Wo = _out_hw(H, W, stride)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64).float().double()
    zero = torch.zeros(N, 18, Ho, Wo, dtype=torch.float64)
    by, bx = R.sample_coords(zero, H, W, 3, stride, 1)
    fy = torch.randint(1, 64, by.shape, generator=g).double() / 64
    fx = torch.randint(1, 64, bx.shape, generator=g).double() / 64
    om = torch.empty(N, 27, Ho, Wo, dtype=torch.float64)
    om[:, 0:18:2] = 3 + fy - by  # rows 3..4, columns 4..5
    om[:, 1:18:2] = 4 + fx - bx
    om[:, 18:] = _logits((N, 9, Ho, Wo), g)
    py, px = R.sample_coords(om[:, :18], H, W, 3, stride, 1)
    assert bool(((py > 3) & (py < 4) & (px > 4) & (px < 5)).all())
    dcol = torch.randn(N, C * 9, Ho * Wo, generator=g,
                       dtype=torch.float64).float().double()
    (_, dx64, do64), (_, dx32, do32) = _sampling_reference(x, om, dcol, stride)
    _, dx_a, dom = _device_sampling(x, om, dcol, stride, dev)
    _, dx_b, _ = _device_sampling(x, om, dcol, stride, dev)
    assert torch.equal(dx_a, dx_b)
    touched = dx_a.cpu().abs().sum(dim=(0, 1)) > 0
    assert int(touched.sum()) == 4 and bool(touched[3:5, 4:6].all())
    _band_f(dx_a, dx64, dx32, 'd_x (collisions)')
    _band_f(dom, do64, do32, 'd_om (collisions)')


@pytest.mark.parametrize('N,C,H,W,stride', SAMPLING)
@pytest.mark.parametrize('offsets', ['zero', 'grid'])
def test_zero_logits_are_half_of_v1_bit_for_bit(N, C, H, W, stride, offsets):
    """om = 0 (and, beyond it, grid offsets with zero logits): the mask is
    exactly 0.5, a multiplication by 0.5 is exact and the four-term expression
    is v1's, so col == 0.5 * ld_deform_im2col and d_x == 0.5 * v1's d_x bit
    for bit; so are the offset channels of d_om, and the logit channels are
    0.25 x sum_ci d_col * v1's column."""
    from ld_amd import layers as Y
    dev = _dev()
    g = torch.Generator().manual_seed(H + 13 * W)
    Ho, Wo = _out_hw(H, W, stride)
    x = torch.randn(N, C, H, W, generator=g)
    om = torch.zeros(N, 27, Ho, Wo)
    if offsets == 'grid':
        om[:, :18] = R.grid_offsets((N, 18, Ho, Wo), g).float()
    dcol = torch.randn(N, C * 9, Ho * Wo, generator=g)
    col, dx, dom = _device_sampling(x, om, dcol, stride, dev)
    x3 = x.reshape(N, C, H * W).to(dev).requires_grad_(True)
    o3 = om[:, :18].reshape(N, 18, -1).contiguous().to(dev).requires_grad_(True)
    col1 = Y.DeformIm2colFn.apply(x3, o3, H, W, 3, stride, 1)
    col1.backward(dcol.to(dev))
    torch.cuda.synchronize()
    assert float(col1.detach().abs().max()) > 0
    assert torch.equal(col, 0.5 * col1.detach())
    assert torch.equal(dx.reshape(N, C, -1), 0.5 * x3.grad)
    assert torch.equal(dom[:, :18].reshape(N, 18, -1), 0.5 * o3.grad)
    want = 0.25 * (dcol.double() * col1.detach().double().cpu()).view(
        N, C, 9, Ho * Wo).sum(1)
    _close(dom[:, 18:].reshape(N, 9, -1), want, 'd_logit at m = 0.5')


# ------------------------------------------------------ 4: the whole module ---
def _bn(c, g):
    from ld_amd.cnn import BatchNorm2d
    bn = BatchNorm2d(c).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.2)
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(c, generator=g) * 0.4 + 0.8)
    return bn


def _module(cin, cout, stride, groups, bias, g, oscale):
    from ld_amd.cnn import ModulatedDeformConv2dPack
    m = ModulatedDeformConv2dPack(cin, cout, 3, stride=stride, padding=1,
                                  groups=groups, bias=bias)
    with torch.no_grad():
        m.weight.copy_(torch.randn(m.weight.shape, generator=g) /
                       (9 * cin // groups)**0.5)
        if bias:
            m.bias.copy_(torch.randn(cout, generator=g) * 0.5)
        m.conv_offset.weight.copy_(
            torch.randn(m.conv_offset.weight.shape, generator=g) * oscale /
            (9 * cin)**0.5)
        m.conv_offset.bias.copy_(torch.randn(27, generator=g) * 0.7)
    return m


def _module_reference(m, bn, x, gy, stride, dt):
    """[y, dx, d weight, d conv_offset.weight, d conv_offset.bias, (d bias |
    d gamma, d beta)], om -- the float64 / float32 module on the CPU; with
    ``bn`` the eval-mode affine follows the (grouped) product."""
    ps = [m.weight, m.conv_offset.weight, m.conv_offset.bias]
    if m.bias is not None:
        ps.append(m.bias)
    if bn is not None:
        ps += [bn.weight, bn.bias]
    ps = [p.detach().clone().to(dt).requires_grad_(True) for p in ps]
    a = x.detach().clone().to(dt).requires_grad_(True)
    if m.groups != 1:
        y, om = M.mdcn_pack_forward_grouped(a, ps[0], ps[1], ps[2], m.groups,
                                            stride, 1)
    else:
        y, om = M.mdcn_pack_forward(a, ps[0], ps[3] if m.bias is not None
                                    else None, ps[1], ps[2], stride, 1)
    if bn is not None:
        inv = (bn.running_var.to(dt) + bn.eps).rsqrt().view(1, -1, 1, 1)
        y = (y - bn.running_mean.to(dt).view(1, -1, 1, 1)) * inv * \
            ps[-2].view(1, -1, 1, 1) + ps[-1].view(1, -1, 1, 1)
    y.backward(gy.to(dt))
    return [y.detach(), a.grad] + [p.grad for p in ps], om.detach()


def _module_device(m, bn, x, gy, dev):
    N, C, H, W = x.shape
    m = copy.deepcopy(m).to(dev)
    bn = copy.deepcopy(bn).to(dev) if bn is not None else None
    x3 = x.reshape(N, C, H * W).to(dev).requires_grad_(True)
    lv = ((H, W), )
    if bn is None:
        y3, olv = m.forward3(x3, lv)
    else:
        y3, olv = m.forward3_bn(x3, lv, bn, None, False)
    y3.backward(gy.reshape(N, gy.shape[1], -1).to(dev))
    torch.cuda.synchronize()
    (ho, wo), = olv
    got = [y3.detach().view(N, -1, ho, wo), x3.grad.view(N, C, H, W),
           m.weight.grad, m.conv_offset.weight.grad, m.conv_offset.bias.grad]
    if m.bias is not None:
        got.append(m.bias.grad)
    if bn is not None:
        got += [bn.weight.grad, bn.bias.grad]
    # the frozen forward: the same module under no_grad (three launches), the
    # eval-BN node applied to its raw result as the trainable pair applies it
    with torch.no_grad():
        f3, _ = m.forward3(x3.detach(), lv)
        if bn is not None:
            f3 = bn.forward3(f3, None, False)
    torch.cuda.synchronize()
    return got, y3.detach(), f3


MODULE_CASES = [  # name, N, cin, cout, H, W, stride, groups, bias, bn, oscale
    ('plain', 2, 8, 16, 9, 11, 1, 1, False, False, 1.5),
    ('plain_bias_s2', 2, 16, 8, 9, 11, 2, 1, True, False, 2.0),
    ('plain_bn_pair', 1, 16, 16, 9, 11, 1, 1, False, True, 1.5),
    ('grouped_8_per_group', 2, 16, 16, 9, 11, 1, 2, False, True, 1.5),
    ('grouped_4_per_group_s2', 1, 16, 16, 9, 11, 2, 4, False, True, 2.0),
]


@pytest.mark.parametrize('case', MODULE_CASES, ids=[c[0] for c in MODULE_CASES])
def test_module_gradients_vs_float64(case):
    """The whole trainable ModulatedDeformConv2dPack with non-zero conv_offset
    weights (offsets that leave the 3x3 window, masks away from 0.5): y, the
    input gradient and every parameter gradient against the float64 module,
    band (1) on every element -- plain with and without bias, the conv + eval-BN
    pair, and grouped (8 and 4 output channels per group) as conv + BN.

    The device computes om in fp32, so a sample within rounding of an integer
    coordinate could take the neighbouring cell.  The seeds are fixed ones for
    which no float64 coordinate lies within 2e-5 of an integer -- twenty times
    the fp32 rounding of a coordinate below 16 -- so fp32 and fp64 sample the
    same cells (asserted), and the restatement evaluated in fp32 on the CPU
    stays in the same band (asserted too).

    The frozen (no_grad) forward of the same module equals the trainable
    forward bit for bit; for the pairs the eval-BN node is applied to the
    frozen raw result, which is how the trainable grouped pair computes it."""
    name, N, cin, cout, H, W, stride, groups, bias, with_bn, oscale = case
    dev = _dev()
    g = torch.Generator().manual_seed(len(name) * 17 + cin + 1)
    x = torch.randn(N, cin, H, W, generator=g)
    m = _module(cin, cout, stride, groups, bias, g, oscale)
    bn = _bn(cout, g) if with_bn else None
    ho, wo = _out_hw(H, W, stride)
    gy = torch.randn(N, cout, ho, wo, generator=g)
    ref, om64 = _module_reference(m, bn, x, gy, stride, torch.float64)
    cpu32, om32 = _module_reference(m, bn, x, gy, stride, torch.float32)
    assert float(om64[:, :18].abs().max()) > 2.0
    assert float(torch.sigmoid(om64[:, 18:]).min()) < 0.3
    assert float(torch.sigmoid(om64[:, 18:]).max()) > 0.7
    py, px = R.sample_coords(om64[:, :18], H, W, 3, stride, 1)
    for c in (py, px):
        assert float((c - c.round()).abs().min()) > 2e-5, name
    q = R.sample_coords(om32[:, :18], H, W, 3, stride, 1)
    assert torch.equal(q[0].floor().double(), py.floor())
    assert torch.equal(q[1].floor().double(), px.floor())
    names = ['y', 'input gradient', 'weight.grad', 'conv_offset.weight.grad',
             'conv_offset.bias.grad']
    names += ['bias.grad'] if bias else []
    names += ['bn.weight.grad', 'bn.bias.grad'] if with_bn else []
    assert len(names) == len(ref)
    for what, a, b in zip(names, cpu32, ref):
        _band_1(a, b, f'{name} fp32-cpu {what}')
    got, y_train, y_frozen = _module_device(m, bn, x, gy, dev)
    assert len(got) == len(ref)
    for what, a, b in zip(names, got, ref):
        _band_1(a, b, f'{name} {what}')
    assert torch.equal(y_train, y_frozen)


def test_zero_conv_offset_is_half_the_convolution():
    """conv_offset at its zero init: the layer is 0.5 x cnn.Conv2d with the
    same weight (band (C): im2col + GEMM against the direct conv), with the
    bias added once."""
    from ld_amd.cnn import Conv2d, ModulatedDeformConv2dPack
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    N, cin, cout, H, W = 2, 16, 16, 9, 11
    m = ModulatedDeformConv2dPack(cin, cout, 3, padding=1).to(dev)
    c = Conv2d(cin, cout, 3, padding=1, bias=False).to(dev)
    with torch.no_grad():
        m.bias.copy_(torch.randn(cout, generator=g))
        c.weight.copy_(m.weight)
    x3 = torch.randn(N, cin, H * W, generator=g).to(dev)
    with torch.no_grad():
        y, _ = m.forward3(x3, ((H, W), ))
        yc, _ = c.forward3(x3, ((H, W), ))
    torch.cuda.synchronize()
    _close(y, 0.5 * yc + m.bias.view(1, -1, 1), 'zero-init DCNv2')


# ---------------------------------------------------------- 5: detectors ---
def _batch(dev):
    b = synthetic.synthetic_batch(2, (128, 150), (128, 160), [3, 2], 21)
    return dict(img=b['img'].to(dev), img_metas=b['img_metas'],
                gt_bboxes=[x.to(dev) for x in b['gt_bboxes']],
                gt_labels=[x.to(dev) for x in b['gt_labels']])


def _perturbed_detector(dev):
    """gfl_dcnv2_detector(101) on gfl_detector(101)'s seeded weights, its
    conv_offset perturbed: small seeded weights, offsets 0.6, logits 0.3."""
    from ld_amd import build_detector, model_zoo
    det = build_detector(model_zoo.gfl_dcnv2_detector(101))
    plain_sd = build_detector(model_zoo.gfl_detector(101)).state_dict()
    sd = synthetic.seeded_state_dict(plain_sd, seed=1)
    missing = det.load_state_dict(sd, strict=False)
    assert all('conv_offset' in k for k in missing.missing_keys)
    assert len(missing.missing_keys) == 2 * (4 + 23 + 3)
    assert not missing.unexpected_keys
    g = torch.Generator().manual_seed(9)
    for k, v in det.state_dict().items():
        if k.endswith('conv_offset.weight'):
            v.copy_(torch.randn(v.shape, generator=g) * 0.02 /
                    (9 * v.shape[1])**0.5)
        elif k.endswith('conv_offset.bias'):
            v[:18] = 0.6
            v[18:] = 0.3
    return det.to(dev).train()


def test_detector_train_step_finite_nonzero_and_reproducible():
    """gfl_dcnv2_detector(101) at 2 x 128 x 160 with perturbed offsets: the
    first SGDTrainer step runs with finite losses, every DCNv2 parameter gets a
    non-zero gradient and moves, and the same step from a copy of the same
    state leaves bit-identical parameters."""
    from ld_amd.cnn import ModulatedDeformConv2dPack
    from ld_amd.train import SGDTrainer
    dev = _dev()
    det = _perturbed_detector(dev)
    twin = copy.deepcopy(det)
    d = _batch(dev)
    before = {k: p.detach().clone() for k, p in det.named_parameters()}
    outs = []
    for net in (det, twin):
        tr = SGDTrainer(net, lr=0.0025)
        tr.check_grads = True  # every parameter gets its gradient
        out = tr.step(d)
        torch.cuda.synchronize()
        assert np.isfinite(float(out['loss']))
        for k, v in out['log_vars'].items():
            assert np.isfinite(float(v)), k
        outs.append(out)
    assert float(outs[0]['loss']) == float(outs[1]['loss'])
    n = 0
    for name, mod in det.named_modules():
        if not isinstance(mod, ModulatedDeformConv2dPack):
            continue
        n += 1
        for k, p in mod.named_parameters():
            assert p.requires_grad and p.grad is not None, (name, k)
            assert bool(torch.isfinite(p.grad).all()), (name, k)
            assert float(p.grad.abs().max()) > 0, (name, k)
            assert not torch.equal(p.detach(), before[f'{name}.{k}']), (name, k)
    assert n == 30
    tp = dict(twin.named_parameters())
    for k, p in det.named_parameters():
        assert bool(torch.isfinite(p).all()), k
        assert torch.equal(p, tp[k]), k


def test_frozen_dcnv2_teacher_in_an_ld_pair():
    """ld_r101_dcnv2_detector in its R18 <- R50 form (the config-4 pair with a
    DCNv2 teacher): an LD step runs with a finite loss, and what the step takes
    from the teacher -- through the warm, the recorded and the replayed forward
    -- equals the teacher's own no_grad forward bit for bit."""
    from ld_amd import model_zoo
    from ld_amd.cnn import ModulatedDeformConv2dPack
    from ld_amd.train import SGDTrainer
    dev = _dev()
    cfg = model_zoo.ld_r101_dcnv2_detector(student_depth=18, teacher_depth=50)
    det = model_zoo.build_seeded(cfg, dev)
    layers = [m for m in det.teacher_model.modules()
              if isinstance(m, ModulatedDeformConv2dPack)]
    assert len(layers) == 4 + 6 + 3
    assert all(float(m.conv_offset.weight.detach().abs().max()) > 0
               for m in layers)
    d = _batch(dev)
    with torch.no_grad():
        tx = det.teacher_model.extract_feat(d['img'])
        out = det.teacher_model.bbox_head(tx)
    want = [t.float().clone() for t in list(tx) + [t for lvl in out
                                                   for t in lvl]]
    tr = SGDTrainer(det, lr=0.0025)
    for _ in range(2):
        res = tr.step(d)
        assert np.isfinite(float(res['loss']))
    for i in range(5):
        tx, out = det._teacher_forward(d['img'])
        got = list(tx) + [t for lvl in out for t in lvl]
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert torch.equal(a.float(), b), i
    torch.cuda.synchronize()
