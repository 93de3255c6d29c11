"""GPU tests (-m gpu) of the grouped-convolution backward (csrc/gconv.hip:
ld_gconv_dgrad, ld_gconv_wgrad; layers.GroupedConvFn; the trainable paths of
cnn.GroupedConv2d and of the grouped cnn.DeformConv2dPack) against the float64
restatement tests/_gconv_ref64.py.

Bands, as in tests/test_gpu_dcn_backward.py.  (F): our worst error against
float64 <= 3 x the worst error of the float32 CPU evaluation + 5e-5 max|g|, on
every element.  (C): 2e-4 rel + 2e-5 of the tensor scale, between two device
results that differ in summation order only."""
import numpy as np
import pytest
import torch

import _dcn_ref64 as D
import _gconv_ref64 as R
from ld_amd import synthetic

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _band_f(got, g64, g32, what):
    got = got.detach().double().cpu().reshape(g64.shape)
    ours = float((got - g64).abs().max())
    theirs = float((g32.double() - g64).abs().max())
    am = float(g64.abs().max())
    print(f'{what}: ours {ours:.3e} fp32-cpu {theirs:.3e} max|g| {am:.3e}')
    assert am > 0
    assert ours <= 3.0 * theirs + 5e-5 * am, (what, ours, theirs, am)


def _close(got, ref, what, rtol=2e-4, atol_rel=2e-5):
    got = got.detach().double().cpu().numpy()
    ref = ref.detach().double().cpu().numpy()
    scale = float(np.abs(ref).max()) + 1e-30
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol_rel * scale,
                               err_msg=what)


# ------------------------------------------------------ 1: kernel level ---
def _multi_slab_case():
    """A CG-4 case whose N * Pout positions span 3 slabs, the last one partial
    (sized through ld_gconv_wgrad_slabs)."""
    from ld_amd import lib as L
    lib = L.get_lib()
    H, W = 67, 71
    one = lib.ld_gconv_wgrad_slabs(1, 3, 1, 1, 1, 1)
    assert one == 1
    # the slab size: the largest P that is still one slab
    lo, hi = 1, 1 << 20
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if lib.ld_gconv_wgrad_slabs(1, 1, 1, 0, 1, mid) == 1:
            lo = mid
        else:
            hi = mid - 1
    slab = lo
    # one image of 2 * slab + a partial slab
    W1 = (2 * slab + slab // 3) // H + 1
    assert 2 * slab < H * W1 < 3 * slab
    return (1, 128, 32, H, W1, 3, 1)


CASES = [
    (2, 128, 32, 17, 19, 3, 1),    # CG 4, P = 323: a partial second block
    (1, 256, 32, 21, 27, 3, 2),    # CG 8, odd sizes under stride 2
    (2, 512, 32, 13, 17, 3, 2),    # CG 16
    (1, 1024, 32, 7, 9, 3, 1),     # CG 32
    (1, 128, 32, 1, 1, 3, 1),      # only the centre tap is in range
    (1, 256, 64, 9, 11, 3, 1),     # 64x4d
    (1, 144 * 32, 32, 9, 11, 1, 1),  # DCN GEMM, cin_g 144, Cout 512
    (2, 288 * 32, 32, 5, 7, 1, 1),   # DCN GEMM, cin_g 288, Cout 1024
    'multi_slab',
]


def _case(c):
    return _multi_slab_case() if c == 'multi_slab' else c


def _tensors(case):
    N, C, G, H, W, k, s = case
    cout = C if k == 3 else C // 9
    g = torch.Generator().manual_seed(C + 31 * H + W + s)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(cout, C // G, k, k, generator=g) / (C // G * k * k) ** 0.5
    ho, wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    dy = torch.randn(N, cout, ho, wo, generator=g)
    return x, w, dy, cout


def _device_grads(case, dev, addend=None, preload=None):
    from ld_amd import layers as Y
    N, C, G, H, W, k, s = case
    x, w, dy, cout = _tensors(case)
    lv = ((H, W), )
    x3 = x.reshape(N, C, H * W).to(dev)
    dy3 = dy.reshape(N, cout, -1).to(dev).contiguous()
    wd = w.to(dev)
    dx = Y.gconv_dgrad(dy3, wd, G, s, k // 2, lv, x3.shape, addend=addend)
    if preload is None:
        dw = Y.gconv_wgrad(x3, dy3, wd, G, s, k // 2, lv)
    else:
        pw = wd.clone().requires_grad_(True)
        pw._ld_grad = preload
        assert Y.gconv_wgrad(x3, dy3, pw, G, s, k // 2, lv, pw=pw) is None
        Y.wgrad_join()
        dw = preload
    torch.cuda.synchronize()
    return dx, dw


@pytest.mark.parametrize('case', CASES, ids=[str(c) for c in CASES])
def test_dgrad_wgrad_vs_float64(case):
    """Every element of dx and dw, band (F)."""
    dev = _dev()
    case = _case(case)
    N, C, G, H, W, k, s = case
    if case == _multi_slab_case():
        from ld_amd import lib as L
        lib = L.get_lib()
        n = lib.ld_gconv_wgrad_slabs(N, k, s, k // 2, H, W)
        # at least 3 slabs, and one position fewer per slab would not fit:
        # the last slab is partial
        assert n >= 3, n
        assert lib.ld_gconv_wgrad_slabs(N, 1, 1, 0, 1, H * W // n) == 1
        assert lib.ld_gconv_wgrad_slabs(N, 1, 1, 0, 1, H * W // (n - 1)) == 2
    x, w, dy, _ = _tensors(case)
    _, dx64, dw64 = R.gconv_grads(x, w, dy, G, s, k // 2, torch.float64)
    _, dx32, dw32 = R.gconv_grads(x, w, dy, G, s, k // 2, torch.float32)
    dx, dw = _device_grads(case, dev)
    _band_f(dx, dx64, dx32, 'dx')
    _band_f(dw, dw64, dw32, 'dw')


def test_addend_and_accumulate():
    """dx = addend + dgrad and dw += wgrad (the arena destination), band (F)
    around preloaded buffer + gradient."""
    dev = _dev()
    case = CASES[1]
    N, C, G, H, W, k, s = case
    x, w, dy, _ = _tensors(case)
    g = torch.Generator().manual_seed(5)
    add = torch.randn(N, C, H * W, generator=g)
    pre = torch.randn(w.shape, generator=g)
    _, dx64, dw64 = R.gconv_grads(x, w, dy, G, s, k // 2, torch.float64)
    _, dx32, dw32 = R.gconv_grads(x, w, dy, G, s, k // 2, torch.float32)
    dx, dw = _device_grads(case, dev, addend=add.to(dev),
                           preload=pre.to(dev).clone())
    a4 = add.view(N, C, H, W)
    _band_f(dx, dx64 + a4.double(), dx32 + a4, 'addend + dx')
    _band_f(dw, dw64 + pre.double(), dw32 + pre, 'preload + dw')


# ------------------------------------------------- 2: reproducibility ---
@pytest.mark.parametrize('case', [CASES[1], 'multi_slab'], ids=['case2', 'slabs'])
def test_backward_twice_is_bit_identical(case):
    dev = _dev()
    a = _device_grads(_case(case), dev)
    b = _device_grads(_case(case), dev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert float(a[0].abs().max()) > 0 and float(a[1].abs().max()) > 0


# -------------------------------------------------------- 3: modules ---
def _bn(c, g, dev=None):
    from ld_amd.cnn import BatchNorm2d
    bn = BatchNorm2d(c).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.2)
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    return bn


def _bn_tuple(bn):
    return (bn.weight.detach(), bn.bias.detach(), bn.running_mean,
            bn.running_var, bn.eps)


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('tail', [False, True], ids=['plain', 'res_relu'])
def test_grouped_conv_bn_vs_float64(stride, tail):
    """GroupedConv2d.forward3_bn, BN affine trainable: d_x, d_weight, d_gamma,
    d_beta in band (F)."""
    from ld_amd.cnn import GroupedConv2d
    dev = _dev()
    N, C, G, H, W = 2, 256, 32, 14, 18
    g = torch.Generator().manual_seed(7 + stride + 2 * tail)
    m = GroupedConv2d(C, C, 3, stride=stride, padding=1, groups=G)
    with torch.no_grad():
        m.weight.copy_(torch.randn(m.weight.shape, generator=g) / 8.5)
    bn = _bn(C, g)
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = torch.randn(N, C, H, W, generator=g)
    res = torch.randn(N, C, ho, wo, generator=g) if tail else None
    dy = torch.randn(N, C, ho, wo, generator=g)
    r64 = R.gconv_bn_grads(x, m.weight, _bn_tuple(bn), res, tail, dy, G, stride,
                           torch.float64)
    r32 = R.gconv_bn_grads(x, m.weight, _bn_tuple(bn), res, tail, dy, G, stride,
                           torch.float32)
    m.to(dev), bn.to(dev)
    x3 = x.reshape(N, C, -1).to(dev).requires_grad_(True)
    r3 = res.reshape(N, C, -1).to(dev) if tail else None
    y3, lv = m.forward3_bn(x3, ((H, W), ), bn, r3, tail)
    assert lv == ((ho, wo), )
    y3.backward(dy.reshape(N, C, -1).to(dev))
    torch.cuda.synchronize()
    got = (y3, x3.grad, m.weight.grad, bn.weight.grad, bn.bias.grad)
    for what, a, b, c in zip(('y', 'd_x', 'd_weight', 'd_gamma', 'd_beta'), got,
                             r64, r32):
        _band_f(a, b, c, what)


def _grouped_dcn(cin, groups, g, bias):
    from ld_amd.cnn import DeformConv2dPack
    m = DeformConv2dPack(cin, cin, 3, padding=1, groups=groups)
    with torch.no_grad():
        m.weight.copy_(torch.randn(m.weight.shape, generator=g) /
                       (9 * cin // groups) ** 0.5)
        if bias is not None:
            m.conv_offset.bias.copy_(bias)
    return m


def test_grouped_dcn_bn_vs_float64():
    """Grouped DeformConv2dPack.forward3_bn at (1, 512, 32, 9, 12).  The offset
    conv's weight is zero and its bias sits on _dcn_ref64.grid_offsets' 1/64
    grid, so the offsets are the same exact numbers in every format and no
    floor can flip: band (F) for d_x, d_weight, d_gamma, d_beta and
    d conv_offset.{weight, bias}."""
    dev = _dev()
    N, C, G, H, W = 1, 512, 32, 9, 12
    g = torch.Generator().manual_seed(11)
    bias = D.grid_offsets((18, ), g, lo=-2.0, hi=2.0).float()
    m = _grouped_dcn(C, G, g, bias)
    bn = _bn(C, g)
    x = torch.randn(N, C, H, W, generator=g)
    dy = torch.randn(N, C, H, W, generator=g)
    args = (x, m.weight, m.conv_offset.weight, m.conv_offset.bias, _bn_tuple(bn),
            dy, G, 1)
    r64 = R.gdcn_bn_grads(*args, torch.float64)
    r32 = R.gdcn_bn_grads(*args, torch.float32)
    m.to(dev), bn.to(dev)
    x3 = x.reshape(N, C, -1).to(dev).requires_grad_(True)
    y3, _ = m.forward3_bn(x3, ((H, W), ), bn, None, False)
    y3.backward(dy.reshape(N, C, -1).to(dev))
    torch.cuda.synchronize()
    got = (y3, x3.grad, m.weight.grad, m.conv_offset.weight.grad,
           m.conv_offset.bias.grad, bn.weight.grad, bn.bias.grad)
    names = ('y', 'd_x', 'd_weight', 'd_offset_weight', 'd_offset_bias',
             'd_gamma', 'd_beta')
    for what, a, b, c in zip(names, got, r64, r32):
        _band_f(a, b, c, what)


# --------------------------------------------------- 4: zero offsets ---
def test_zero_offset_grouped_dcn_is_the_grouped_conv():
    from ld_amd.cnn import GroupedConv2d
    dev = _dev()
    N, C, G, H, W = 1, 512, 32, 9, 12
    g = torch.Generator().manual_seed(13)
    m = _grouped_dcn(C, G, g, None).to(dev)
    c = GroupedConv2d(C, C, 3, padding=1, groups=G).to(dev)
    with torch.no_grad():
        c.weight.copy_(m.weight)
    bn = _bn(C, g).to(dev)
    x = torch.randn(N, C, H * W, generator=g).to(dev)
    dy = torch.randn(N, C, H * W, generator=g).to(dev)
    outs = []
    for mod in (m, c):
        x3 = x.clone().requires_grad_(True)
        bn.zero_grad()
        y3, _ = mod.forward3_bn(x3, ((H, W), ), bn, None, True)
        y3.backward(dy)
        torch.cuda.synchronize()
        outs.append((y3.detach(), x3.grad, mod.weight.grad))
    for what, a, b in zip(('y', 'd_x', 'd_weight'), *outs):
        _close(a, b, what)


# ------------------------------------------------------- 5: backbone ---
def _pin_restatement_on_reference(golden):
    """The float64 restatement's forward against the reference's own ResNeXt
    (tests/golden/resnext.npz, case x50_odd; 2e-4 of the tensor scale, the bar
    tests/test_gpu_resnext.py holds the device to)."""
    from ld_amd import model_zoo
    from ld_amd.registry import build_backbone
    g = golden['resnext']
    depth, n, h, w, seed, step = [int(v) for v in g['x50_odd_cfg']]
    net = build_backbone(model_zoo._x101_backbone(depth))
    sd = synthetic.seeded_state_dict(net.state_dict(), seed=seed)
    x = torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(seed + 100))
    with torch.no_grad():
        outs = R.resnext_forward({k: v.double() for k, v in sd.items()},
                                 x.double())
    for i, o in enumerate(outs):
        assert tuple(o.shape) == tuple(int(v) for v in g[f'x50_odd_shape{i}'])
        ref = g[f'x50_odd_out{i}'].astype(np.float64)
        got = o.numpy().reshape(-1)[::step]
        sc = float(np.abs(ref).max())
        assert float(np.abs(got - ref).max()) <= 2e-4 * sc, i


def _restatement_grads(sd, trainable, x, projs, dtype):
    t = {k: v.detach().clone().to(dtype) for k, v in sd.items()
         if v.is_floating_point()}
    for k in trainable:
        t[k].requires_grad_(True)
    outs = R.resnext_forward(t, x.to(dtype))
    loss = sum((o * p.to(dtype)).sum() for o, p in zip(outs, projs))
    loss.backward()
    return [o.detach() for o in outs], {k: t[k].grad for k in trainable}


def test_resnext50_backbone_gradients_vs_float64(golden):
    """ResNeXt(depth=50, groups=32, base_width=4, frozen_stages=1), seeded
    weights, 2 x 3 x 64 x 96; loss = fixed random projections of the four stage
    outputs.  Every trainable parameter gradient against the float64
    restatement, band (F) per parameter (route: the restatement, pinned first
    on the reference's own ResNeXt through the committed golden)."""
    from ld_amd import model_zoo
    from ld_amd.registry import build_backbone
    _pin_restatement_on_reference(golden)
    dev = _dev()
    net = build_backbone(model_zoo._x101_backbone(50))
    assert net.frozen_stages == 1 and net.groups == 32 and net.base_width == 4
    sd = synthetic.seeded_state_dict(net.state_dict(), seed=33)
    net.load_state_dict(sd)
    net.train()
    trainable = [k for k, p in net.named_parameters() if p.requires_grad]
    assert trainable and not any(k.startswith(('conv1', 'bn1', 'layer1'))
                                 for k in trainable)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, 64, 96, generator=g)
    shapes = [(2, 256, 16, 24), (2, 512, 8, 12), (2, 1024, 4, 6), (2, 2048, 2, 3)]
    projs = [torch.randn(sh, generator=g) / (sh[1] * sh[2] * sh[3]) ** 0.5
             for sh in shapes]
    o64, g64 = _restatement_grads(sd, trainable, x, projs, torch.float64)
    o32, g32 = _restatement_grads(sd, trainable, x, projs, torch.float32)
    net.to(dev)
    outs = net(x.to(dev))
    loss = sum((o * p.to(dev)).sum() for o, p in zip(outs, projs))
    loss.backward()
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        _band_f(o, o64[i], o32[i], f'stage {i}')
    params = dict(net.named_parameters())
    bad = []
    for k in trainable:
        got = params[k].grad.detach().double().cpu()
        ours = float((got - g64[k]).abs().max())
        theirs = float((g32[k].double() - g64[k]).abs().max())
        am = float(g64[k].abs().max())
        if not ours <= 3.0 * theirs + 5e-5 * am:
            bad.append((k, ours, theirs, am))
    print(f'{len(trainable)} parameters, outside band (F): {bad[:8]}')
    assert not bad, (len(bad), bad[:8])


# -------------------------------------------------------- 6: trainer ---
def _batch(dev):
    b = synthetic.synthetic_batch(2, (128, 150), (128, 160), [3, 2], 21)
    return dict(img=b['img'].to(dev), img_metas=b['img_metas'],
                gt_bboxes=[x.to(dev) for x in b['gt_bboxes']],
                gt_labels=[x.to(dev) for x in b['gt_labels']])


def _detector(cfg, dev):
    from ld_amd import build_detector
    det = build_detector(cfg)
    det.load_state_dict(synthetic.seeded_state_dict(det.state_dict(), seed=3))
    return det.to(dev).train()


def _two_steps(cfg, dev, d):
    from ld_amd import layers as Y
    from ld_amd import lib as L
    from ld_amd.cnn import GroupedConv2d
    from ld_amd.train import SGDTrainer
    det = _detector(cfg, dev)
    tr = SGDTrainer(det, lr=0.0025)
    tr.check_grads = True
    tables, grads = [], None
    for i in range(2):
        out = tr.step(d)
        torch.cuda.synchronize()
        assert np.isfinite(float(out['loss']))
        tables.append({k: float(v) for k, v in out['log_vars'].items()})
        if i == 0:
            grads = tr.arena.flat_grad.clone()
            # the images of a trainable grouped weight follow the optimizer step
            lib = L.get_lib()
            for k, m in det.named_modules():
                if isinstance(m, GroupedConv2d) and m.weight.requires_grad:
                    cache = m.weight._ld_gimages
                    fresh = torch.empty_like(cache['fwd'])
                    Y._gconv_xform(lib, m.weight, m.groups, fresh, False)
                    assert torch.equal(cache['fwd'], fresh), k
                    fresh = torch.empty_like(cache['bwd'])
                    Y._gconv_xform(lib, m.weight, m.groups, fresh, True)
                    assert torch.equal(cache['bwd'], fresh), k
    params = torch.cat([p.detach().reshape(-1) for p in det.parameters()])
    return det, tr, tables, grads, params


@pytest.mark.parametrize('which', ['gfl_x101', 'gflv2_x101_dcn'])
def test_trainer_steps(which):
    """Two SGDTrainer steps.  (a) the arena gradients of step 1 equal a plain
    loss.backward() with DIRECT_GRADS off, band (C); (d) the same two steps
    from the same seed again are bit-identical (loss tables, gradients,
    parameters); after step 1 every trainable grouped weight's cached images
    equal a fresh transform of the updated weight (no stale image)."""
    from ld_amd import layers as Y
    from ld_amd import model_zoo
    dev = _dev()
    cfg = model_zoo.gfl_x101_detector() if which == 'gfl_x101' else \
        model_zoo.gflv2_x101_detector(dcn=True)
    d = _batch(dev)
    _, _, t1, g1, p1 = _two_steps(cfg, dev, d)
    _, _, t2, g2, p2 = _two_steps(cfg, dev, d)
    assert t1 == t2
    assert torch.equal(g1, g2) and torch.equal(p1, p2)
    assert float(g1.abs().max()) > 0
    # (a): plain autograd, no arena
    det = _detector(cfg, dev)
    from ld_amd.train import SGDTrainer
    tr = SGDTrainer(det, lr=0.0025)
    tr.arena.zero_grad()
    loss, _ = det._parse_losses(det(**d))
    loss.backward()
    tr.arena.finish()
    torch.cuda.synchronize()
    arena = {k: p._ld_grad.detach().clone() for k, p in det.named_parameters()
             if p.requires_grad}
    plain = _detector(cfg, dev)  # no trainer, no arena: autograd's own sums
    prev = Y.DIRECT_GRADS[0]
    Y.DIRECT_GRADS[0] = False
    try:
        loss, _ = plain._parse_losses(plain(**d))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        Y.DIRECT_GRADS[0] = prev
    pg = {k: p.grad for k, p in plain.named_parameters() if p.requires_grad}
    n = 0
    for k, p in det.named_parameters():
        if p.requires_grad:
            _close(arena[k], pg[k], k)
            n += 'conv2.weight' in k
    assert n >= 30


def _cfg(which):
    from ld_amd import model_zoo
    return model_zoo.gfl_x101_detector() if which == 'gfl_x101' else \
        model_zoo.gflv2_x101_detector(dcn=True)


def _dense_twin(cfg, dev):
    """The detector of ``_detector`` with every grouped conv2 swapped for its
    dense block-diagonal twin on the existing dense kernels: cnn.Conv2d, or a
    groups = 1 DeformConv2dPack with the same offset conv.  -> (det, [(weight
    parameter, block mask)])."""
    from ld_amd import build_detector
    from ld_amd.cnn import Conv2d, DeformConv2dPack, GroupedConv2d
    det = build_detector(cfg)
    det.load_state_dict(synthetic.seeded_state_dict(det.state_dict(), seed=3))
    masks = []
    for blk in [m for m in det.modules() if hasattr(m, 'conv2')]:
        c = blk.conv2
        if isinstance(c, GroupedConv2d):
            t = Conv2d(c.in_channels, c.out_channels, 3, stride=c.stride[0],
                       padding=1, bias=False)
        elif isinstance(c, DeformConv2dPack) and c.groups > 1:
            t = DeformConv2dPack(c.in_channels, c.out_channels, 3,
                                 stride=c.stride[0], padding=1)
            t.conv_offset.load_state_dict(c.conv_offset.state_dict())
        else:
            continue
        dense, mask = R.block_diagonal(c.weight.detach(), c.groups)
        with torch.no_grad():
            t.weight.copy_(dense)
        blk.conv2 = t
        masks.append((t, mask))
    assert len(masks) == 33
    det.to(dev).train()  # ResNet.train() freezes stage 1 of the twin as well
    return det, [(t.weight, m.to(dev)) for t, m in masks]


@pytest.mark.parametrize('which', ['gfl_x101', 'gflv2_x101_dcn'])
def test_trainer_steps_vs_dense_block_diagonal_twin(which):
    """(b) The same two SGDTrainer steps on the dense twins: the loss tables of
    step 1 and of step 2 agree in band (C).  The off-block entries of a twin's
    weight receive a gradient the grouped conv does not have; they are put
    back to zero after step 1, so both nets take the same step.  A grouped
    weight image that did not follow the optimizer step shows in step 2."""
    from ld_amd.train import SGDTrainer
    dev = _dev()
    d = _batch(dev)
    _, _, tables, _, _ = _two_steps(_cfg(which), dev, d)
    twin, masks = _dense_twin(_cfg(which), dev)
    tr = SGDTrainer(twin, lr=0.0025)
    got = []
    for i in range(2):
        out = tr.step(d)
        torch.cuda.synchronize()
        got.append({k: float(v) for k, v in out['log_vars'].items()})
        with torch.no_grad():
            for w, m in masks:
                if w.requires_grad:
                    w.mul_(m)
    moved = 0
    for i in range(2):
        assert got[i].keys() == tables[i].keys()
        for k in tables[i]:
            print(which, 'step', i + 1, k, tables[i][k], got[i][k])
            np.testing.assert_allclose(tables[i][k], got[i][k], rtol=2e-4,
                                       atol=2e-5, err_msg=f'step {i + 1} {k}')
            moved += tables[0][k] != tables[1][k]
    assert moved  # step 2 is not step 1 again


@pytest.mark.parametrize('which', ['gfl_x101', 'gflv2_x101_dcn'])
def test_step_list_equals_eager(which):
    """(c) Steps captured by the step list (launcher='list') are bit-identical
    to eager ones: two eager warm-up steps, then two replays, against four
    eager steps.  Every grouped launch, the side-stream weight gradient and
    refresh_params' grouped image rebuild are inside the captured step."""
    from ld_amd.train import GraphedStep, SGDTrainer
    dev = _dev()
    cfg = _cfg(which)
    eager = SGDTrainer(_detector(cfg, dev), lr=0.0025)
    for _ in range(4):
        out_e = eager.step(_batch(dev))
    torch.cuda.synchronize()
    tr = SGDTrainer(_detector(cfg, dev), lr=0.0025)
    g = GraphedStep(tr, _batch(dev), warmup=2, launcher='list')
    assert g.list.info['kernels'] > 100
    for _ in range(2):
        out_g = g.replay()
        torch.cuda.synchronize()
    assert torch.equal(tr.arena.flat_param, eager.arena.flat_param)
    assert torch.equal(tr.flat_momentum, eager.flat_momentum)
    assert dict(out_g['log_vars']) == dict(out_e['log_vars'])
    assert np.isfinite(float(out_g['loss']))


# ------------------------------------------------------- 7: refusals ---
def test_refusals_still_raise():
    from ld_amd import build_detector, model_zoo
    from ld_amd import layers as Y
    from ld_amd.cnn import DeformConv2dPack, GroupedConv2d
    from ld_amd.optim import classify
    dev = _dev()
    lv = ((6, 7), )
    m = GroupedConv2d(128, 128, 3, padding=1, groups=32).to(dev)
    c8 = Y.C8Act(torch.zeros(1, 16, 42, 8, dtype=torch.bfloat16, device=dev),
                 (1, 128, 42))
    with pytest.raises(NotImplementedError, match='C8'):
        m.forward3(c8, lv)
    ghost = Y._image_only_output((1, 128, 42), c8.buf)
    with pytest.raises(NotImplementedError, match='C8'):
        m.forward3(ghost, lv)
    x3 = torch.randn(1, 128, 42, device=dev).requires_grad_(True)
    Y.set_precision('bf16')
    try:
        with pytest.raises(NotImplementedError, match='bf16'):
            m.forward3(x3, lv)
    finally:
        Y.set_precision('fp32')
    gd = DeformConv2dPack(128, 128, 3, padding=1, groups=32).to(dev)
    bn = _bn(128, torch.Generator().manual_seed(1)).to(dev)
    with pytest.raises(NotImplementedError, match='grouped DCN'):
        gd.forward3_bn(x3, lv)  # trains only as the conv + BN pair
    Y.set_precision('bf16')
    try:
        with pytest.raises(NotImplementedError, match='bf16'):
            gd.forward3_bn(x3, lv, bn, None, True)
    finally:
        Y.set_precision('fp32')
    y3, _ = gd.forward3_bn(x3, lv, bn, None, True)
    y3.sum().backward()
    assert gd.weight.grad is not None and x3.grad is not None
    with pytest.raises(NotImplementedError, match='deform_groups'):
        DeformConv2dPack(128, 128, 3, padding=1, groups=32, deform_groups=2)
    with pytest.raises(NotImplementedError, match='dilated'):
        DeformConv2dPack(128, 128, 3, padding=2, dilation=2, groups=32)
    det = build_detector(model_zoo.gfl_x101_dcn_detector()).train()
    with pytest.raises(NotImplementedError, match='deformable'):
        classify(det, dict(norm_decay_mult=0.0))
