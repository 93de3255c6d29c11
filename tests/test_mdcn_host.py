"""CPU tests of modulated deformable convolution (DCNv2): the float64
restatement tests/_mdcn_ref64.py against a literal per-sample loop, the module
cnn.ModulatedDeformConv2dPack (names, shapes, init, mmcv's version-2 state_dict
rename), the backbones / zoo entries that build with ``type='DCNv2'`` and every
refusal at the feature's edges.  Nothing here launches a kernel."""
import math
from collections import OrderedDict

import pytest
import torch
import torch.nn as nn

import _dcn_ref64 as R
import _mdcn_ref64 as M
from ld_amd import build_detector, cnn, model_zoo
from ld_amd.cnn import (DeformConv2dPack, ModulatedDeformConv2dPack,
                        build_conv_layer)
from ld_amd.registry import build_backbone

DCNV2 = dict(type='DCNv2', deform_groups=1, fallback_on_stride=False)


# ------------------------------------------------------ the restatement ---
def _loop_im2col(x, om, k, stride, pad):
    """The formula of the kernel header, one sample at a time in Python
    floats: col[n][ci*kk + t][p] = sigmoid(logit_t(p)) * (w1 x1 + w2 x2 + w3 x3
    + w4 x4), zero outside (-1, H) x (-1, W), corners outside the map 0."""
    N, C, H, W = x.shape
    kk = k * k
    Ho, Wo = om.shape[2:]
    col = torch.zeros(N, C * kk, Ho * Wo, dtype=torch.float64)
    for n in range(N):
        for t in range(kk):
            for ho in range(Ho):
                for wo in range(Wo):
                    h = ho * stride - pad + t // k + float(om[n, 2 * t, ho, wo])
                    w = wo * stride - pad + t % k + \
                        float(om[n, 2 * t + 1, ho, wo])
                    m = 1.0 / (1.0 + math.exp(-float(om[n, 2 * kk + t, ho, wo])))
                    if not (h > -1 and w > -1 and h < H and w < W):
                        continue
                    hl, wl = math.floor(h), math.floor(w)
                    lh, lw = h - hl, w - wl
                    for ci in range(C):
                        v = 0.0
                        for yy, xx, wt in ((hl, wl, (1 - lh) * (1 - lw)),
                                           (hl, wl + 1, (1 - lh) * lw),
                                           (hl + 1, wl, lh * (1 - lw)),
                                           (hl + 1, wl + 1, lh * lw)):
                            if 0 <= yy <= H - 1 and 0 <= xx <= W - 1:
                                v += wt * float(x[n, ci, yy, xx])
                        col[n, ci * kk + t, ho * Wo + wo] = m * v
    return col


@pytest.mark.parametrize('stride', [1, 2])
def test_restatement_equals_the_literal_loop(stride):
    g = torch.Generator().manual_seed(40 + stride)
    H, W = 4, 5
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    x = torch.randn(1, 2, H, W, generator=g, dtype=torch.float64)
    om = torch.empty(1, 27, Ho, Wo, dtype=torch.float64)
    om[:, :18] = R.grid_offsets((1, 18, Ho, Wo), g, lo=-3.0, hi=3.0)
    om[:, 18:] = torch.rand(1, 9, Ho, Wo, generator=g,
                            dtype=torch.float64) * 8 - 4
    om[:, :18, 0, 0] = 0.0  # integer coordinates, tap 0 outside
    py, px = R.sample_coords(om[:, :18], H, W, 3, stride, 1)
    outside = (py <= -1) | (py >= H) | (px <= -1) | (px >= W)
    assert bool(outside.any()) and not bool(outside.all())
    got = M.modulated_im2col(x, om, 3, stride, 1)
    ref = _loop_im2col(x, om, 3, stride, 1)
    assert got.shape == ref.shape == (1, 18, Ho * Wo)
    assert float(ref.abs().max()) > 0.1
    assert float((got - ref).abs().max()) <= 1e-12


@pytest.mark.parametrize('stride', [1, 2])
def test_zero_om_is_half_the_v1_columns(stride):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 6, 7, generator=g, dtype=torch.float64)
    Ho, Wo = (6 + 2 - 3) // stride + 1, (7 + 2 - 3) // stride + 1
    om = torch.zeros(2, 27, Ho, Wo, dtype=torch.float64)
    v1 = R.deform_im2col(x, om[:, :18], 3, stride, 1)
    assert torch.equal(M.modulated_im2col(x, om, 3, stride, 1), 0.5 * v1)
    w = torch.randn(4, 3, 3, 3, generator=g, dtype=torch.float64)
    y, _ = M.mdcn_pack_forward(x, w, None, torch.zeros(27, 3, 3, 3).double(),
                               torch.zeros(27).double(), stride, 1)
    conv = torch.nn.functional.conv2d(x, w, stride=stride, padding=1)
    assert float((y - 0.5 * conv).abs().max()) <= 1e-12


# ------------------------------------------------------------ the module ---
def test_build_conv_layer_gives_the_modulated_pack():
    m = build_conv_layer(dict(type='DCNv2', deform_groups=1), 8, 8, 3,
                         padding=1)
    assert type(m) is ModulatedDeformConv2dPack
    assert not isinstance(m, DeformConv2dPack)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes == {'weight': (8, 8, 3, 3), 'bias': (8, ),  # mmcv: bias=True
                      'conv_offset.weight': (27, 8, 3, 3),
                      'conv_offset.bias': (27, )}
    assert [k for k, _ in m.named_parameters()] == list(shapes)
    sd = m.state_dict()  # detached
    assert float(sd['conv_offset.weight'].abs().max()) == 0.0
    assert float(sd['conv_offset.bias'].abs().max()) == 0.0
    assert float(sd['bias'].abs().max()) == 0.0
    stdv = 1.0 / math.sqrt(8 * 9)
    assert 0 < float(sd['weight'].abs().max()) <= stdv
    # ResNet / ConvModule pass bias=False; groups gives the grouped weight
    nb = build_conv_layer(dict(DCNV2), 8, 8, 3, padding=1, bias=False)
    assert nb.bias is None and 'bias' not in nb.state_dict()
    gr = build_conv_layer(dict(type='DCNv2'), 64, 64, 3, padding=1, groups=16,
                          bias=False)
    assert tuple(gr.weight.shape) == (64, 4, 3, 3)
    assert tuple(gr.conv_offset.weight.shape) == (27, 64, 3, 3)
    # v1 is what it was
    v1 = build_conv_layer(dict(type='DCN', deform_groups=1), 8, 8, 3,
                          padding=1)
    assert type(v1) is DeformConv2dPack
    assert {k: tuple(v.shape) for k, v in v1.state_dict().items()} == {
        'weight': (8, 8, 3, 3), 'conv_offset.weight': (18, 8, 3, 3),
        'conv_offset.bias': (18, )}


def _filled(m, seed):
    g = torch.Generator().manual_seed(seed)
    return OrderedDict((k, torch.randn(v.shape, generator=g))
                       for k, v in m.state_dict().items())


def test_load_state_dict_current_and_pre_version_2_keys():
    m = ModulatedDeformConv2dPack(8, 8, 3, padding=1)
    assert m.state_dict()._metadata['']['version'] == 2
    sd = _filled(m, 1)
    m.load_state_dict(sd)  # current keys, no metadata
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # a round trip through its own state_dict (metadata says version 2)
    m2 = ModulatedDeformConv2dPack(8, 8, 3, padding=1)
    m2.load_state_dict(m.state_dict())
    assert torch.equal(m2.conv_offset.weight, sd['conv_offset.weight'])
    # pre-version-2: the offset conv was `<name>_offset` next to the layer
    old = OrderedDict((k.replace('conv_offset.', '_offset.'), v)
                      for k, v in _filled(m, 2).items())
    assert '_offset.weight' in old and 'conv_offset.weight' not in old
    m.load_state_dict(old)  # strict
    assert torch.equal(m.conv_offset.weight, old['_offset.weight'])
    assert torch.equal(m.conv_offset.bias, old['_offset.bias'])
    assert torch.equal(m.weight, old['weight'])
    # a version-2 checkpoint is not searched for the old names
    stamped = m.state_dict()
    del stamped['conv_offset.weight']
    stamped['_offset.weight'] = torch.ones(27, 8, 3, 3)
    res = m.load_state_dict(stamped, strict=False)
    assert res.missing_keys == ['conv_offset.weight']
    assert res.unexpected_keys == ['_offset.weight']


def test_checkpoint_loader_renames_at_every_depth():
    """nn.Module.load_state_dict shows a nested module only the keys under its
    own prefix; the project's mmcv-style loader (checkpoint.load_state_dict,
    behind load_checkpoint) applies the rename wherever the layer sits:
    ``layer.conv2_offset.*`` loads into ``layer.conv2.conv_offset.*``."""
    from ld_amd.checkpoint import load_state_dict
    block = nn.Sequential(OrderedDict(
        conv2=ModulatedDeformConv2dPack(8, 8, 3, padding=1, bias=False)))
    parent = nn.Sequential(OrderedDict(layer=block))
    new = _filled(parent, 3)
    old = OrderedDict((k.replace('conv2.conv_offset.', 'conv2_offset.'), v)
                      for k, v in new.items())
    assert set(old) == {'layer.conv2.weight', 'layer.conv2_offset.weight',
                        'layer.conv2_offset.bias'}
    res = load_state_dict(parent, old, strict=True)
    assert not res['missing'] and not res['unexpected']
    assert set(old) == {'layer.conv2.weight', 'layer.conv2_offset.weight',
                        'layer.conv2_offset.bias'}  # the caller's dict is whole
    for k, v in parent.state_dict().items():
        assert torch.equal(v, new[k]), k
    # current keys load as before; a version-2 dict is not searched
    load_state_dict(parent, _filled(parent, 4), strict=True)
    stamped = parent.state_dict()
    del stamped['layer.conv2.conv_offset.bias']
    stamped['layer.conv2_offset.bias'] = torch.ones(27)
    with pytest.warns(UserWarning):
        res = load_state_dict(parent, stamped)
    assert res['missing'] == ['layer.conv2.conv_offset.bias']
    assert res['unexpected'] == ['layer.conv2_offset.bias']


# ------------------------------------------------------ backbones and zoo ---
def _layers(net):
    return [(k, m) for k, m in net.named_modules()
            if isinstance(m, ModulatedDeformConv2dPack)]


def test_gfl_dcnv2_detector_has_30_layers_in_c3_c5():
    det = build_detector(model_zoo.gfl_dcnv2_detector(101))
    det.train()
    layers = _layers(det)
    assert len(layers) == 4 + 23 + 3
    assert all(k.startswith(('backbone.layer2', 'backbone.layer3',
                             'backbone.layer4')) and k.endswith('conv2')
               for k, _ in layers)
    for _, m in layers:
        assert m.deform_groups == 1 and m.groups == 1 and m.bias is None
        assert all(p.requires_grad for p in m.parameters())
        assert tuple(m.conv_offset.weight.shape)[:2] == (27, m.in_channels)
        assert float(m.conv_offset.weight.detach().abs().max()) == 0.0
    assert not any(isinstance(m, DeformConv2dPack) for m in det.modules())
    cfg = model_zoo.gfl_dcnv2_detector(101)
    assert cfg['backbone'].pop('dcn') == DCNV2
    assert cfg['backbone'].pop('stage_with_dcn') == (False, True, True, True)
    assert cfg == model_zoo.gfl_detector(101)
    # init_weights keeps the offsets / masks at zero (resnet.py:607-611)
    det.backbone.init_weights(None)
    assert all(float(m.conv_offset.weight.detach().abs().max()) == 0.0
               for _, m in _layers(det))


def test_ld_r101_dcnv2_detector_is_config_4_with_the_type_switched():
    cfg = model_zoo.ld_r101_dcnv2_detector()
    ref = model_zoo.ld_r101_dcn_detector()
    tb = cfg['teacher_config']['model']['backbone']
    assert tb['dcn'] == DCNV2
    tb['dcn'] = dict(tb['dcn'], type='DCN')
    assert cfg == ref
    small = build_detector(model_zoo.ld_r101_dcnv2_detector(
        student_depth=18, teacher_depth=50))
    assert len(_layers(small.teacher_model)) == 4 + 6 + 3
    assert not _layers(small.backbone)


def test_resnext_and_res2net_dcn_backbones_build_with_dcnv2():
    cfg = model_zoo._x101_backbone(50, dcn=True)
    cfg['dcn'] = dict(DCNV2)
    net = build_backbone(cfg)
    layers = _layers(net)
    assert len(layers) == 6 + 3
    assert all(m.groups == 32 and m.bias is None for _, m in layers)
    assert all(k.endswith('conv2') for k, _ in layers)
    cfg = model_zoo._r2n_backbone(50, dcn=True)
    cfg['dcn'] = dict(DCNV2)
    net = build_backbone(cfg)
    net.init_weights(None)
    layers = _layers(net)
    assert len(layers) == 3 * (6 + 3)  # three 3x3 convs per c4-c5 Bottle2neck
    assert all('.convs.' in k for k, _ in layers)
    assert all(float(m.conv_offset.weight.detach().abs().max()) == 0.0
               for _, m in layers)
    assert not any(isinstance(m, DeformConv2dPack) for m in net.modules())


# ---------------------------------------------------------------- refusals ---
def test_refusals_name_the_feature():
    with pytest.raises(NotImplementedError, match='DCNv2.*deform_groups'):
        ModulatedDeformConv2dPack(8, 8, 3, padding=1, deform_groups=2)
    with pytest.raises(NotImplementedError, match='DCNv2.*deform_groups'):
        build_conv_layer(dict(type='DCNv2', deform_groups=4), 8, 8, 3,
                         padding=1)
    with pytest.raises(NotImplementedError, match='dilated DCNv2'):
        ModulatedDeformConv2dPack(8, 8, 3, padding=2, dilation=2)
    with pytest.raises(NotImplementedError, match='DCNv2.*square'):
        ModulatedDeformConv2dPack(8, 8, (3, 1), padding=(1, 0))
    with pytest.raises(NotImplementedError, match='DCNv2.*square'):
        ModulatedDeformConv2dPack(8, 8, 3, stride=(1, 2), padding=1)
    with pytest.raises(NotImplementedError, match='grouped DCNv2 48->48 / 4'):
        ModulatedDeformConv2dPack(48, 48, 3, padding=1, groups=4, bias=False)
    with pytest.raises(NotImplementedError, match='grouped DCNv2 with a bias'):
        ModulatedDeformConv2dPack(64, 64, 3, padding=1, groups=16)
    m = ModulatedDeformConv2dPack(8, 8, 3, padding=1, bias=False)
    x3 = torch.zeros(1, 8, 12 + 2).requires_grad_(True)
    two = ((3, 4), (1, 2))
    with pytest.raises(NotImplementedError,
                       match='DCNv2 on level-concatenated'):
        m.forward3(x3, two)  # trainable path
    with torch.no_grad(), pytest.raises(NotImplementedError,
                                        match='DCNv2 on level-concatenated'):
        m.forward3(x3, two)  # frozen path
    with pytest.raises(NotImplementedError, match='DCNv2 epilogue'):
        m.forward3_bn(x3[:, :, :12], ((3, 4), ), None, None, True)
    s = torch.ones(8)
    with pytest.raises(NotImplementedError,
                       match='ModulatedDeformConv2dPack.forward3_fused'):
        m.forward3_fused(x3[:, :, :12], ((3, 4), ), s, s, None, True)
    with pytest.raises(NotImplementedError,
                       match='ModulatedDeformConv2dPack.forward .4-D.'):
        m(torch.zeros(1, 8, 3, 4))
    grouped = ModulatedDeformConv2dPack(64, 64, 3, padding=1, groups=16,
                                        bias=False)
    g3 = torch.zeros(1, 64, 12).requires_grad_(True)
    with pytest.raises(NotImplementedError, match='grouped DCNv2 trains as'):
        grouped.forward3(g3, ((3, 4), ))
    with torch.no_grad(), pytest.raises(NotImplementedError,
                                        match='grouped DCNv2 with a fused'):
        grouped.forward3_fused(g3, ((3, 4), ), s, s, g3, True)


def test_bias_refused_with_a_folded_norm():
    b = ModulatedDeformConv2dPack(8, 8, 3, padding=1)
    assert b.bias is not None
    bn = cnn.BatchNorm2d(8).eval()
    x3 = torch.zeros(1, 8, 12).requires_grad_(True)
    with pytest.raises(NotImplementedError, match='DCNv2 with a bias.*bn'):
        b.forward3_bn(x3, ((3, 4), ), bn, None, True)
    s = torch.ones(8)
    with torch.no_grad():
        with pytest.raises(NotImplementedError,
                           match='DCNv2 with a bias.*scale'):
            b.forward3_fused(x3, ((3, 4), ), s, None)
        with pytest.raises(NotImplementedError,
                           match='DCNv2 with a bias.*shift'):
            b.forward3_fused(x3, ((3, 4), ), None, s)


def test_training_bn_and_paramwise_cfg_cover_the_new_class():
    from ld_amd.optim import classify
    from ld_amd.resnet import _conv_bn
    conv = build_conv_layer(dict(DCNV2), 16, 16, 3, padding=1, bias=False)
    bn = cnn.BatchNorm2d(16).train()
    with pytest.raises(NotImplementedError,
                       match='ModulatedDeformConv2dPack.*DCNv2'):
        _conv_bn(torch.zeros(2, 16, 12), ((3, 4), ), conv, bn)
    mod = cnn.ConvModule(16, 16, 3, padding=1, conv_cfg=dict(type='DCNv2'),
                         norm_cfg=dict(type='BN')).train()
    assert isinstance(mod.conv, ModulatedDeformConv2dPack)
    with pytest.raises(NotImplementedError, match='ModulatedDeformConv2dPack'):
        mod.forward3(torch.zeros(2, 16, 12), ((3, 4), ))
    model = nn.Sequential(OrderedDict(
        conv=cnn.Conv2d(8, 8, 3),
        dcn=ModulatedDeformConv2dPack(8, 8, 3, padding=1)))
    with pytest.raises(NotImplementedError, match='dcn'):
        classify(model, dict(bias_lr_mult=2.0))
    model.dcn.requires_grad_(False)  # a frozen DCNv2 teacher
    names, mults = classify(model, dict(bias_lr_mult=2.0))
    m = dict(zip(names, mults))
    assert m['conv.bias'] == (2.0, 1.0)
    assert all(v == (1.0, 1.0) for k, v in m.items() if k.startswith('dcn.'))


def test_dcn_on_last_conv_and_unknown_types_stay_refused():
    from ld_amd.heads import FCOSGFLHead
    with pytest.raises(NotImplementedError, match='dcn_on_last_conv'):
        FCOSGFLHead(80, 256, dcn_on_last_conv=True)
    with pytest.raises(NotImplementedError, match='DCNv3.*DCNv2') as e:
        build_conv_layer(dict(type='DCNv3'), 8, 8, 3)
    assert 'outside SURVEY' not in str(e.value)
