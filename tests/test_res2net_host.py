"""Res2Net on the host (no GPU): the registry builds the reference's module tree
key for key (tests/golden/res2net.npz holds the reference's own state_dict key
lists), freezing follows resnet.py:572-588 with the deep stem, the DCN variant
has the reference's 78 zero-initialised DeformConv2dPack at depth 101, both
reference configs resolve to model_zoo.gflv2_r2n101_dcn_detector, and the new C
entry points (csrc/res2net.hip) refuse bad arguments before any launch."""
import ctypes as C
import os

import pytest
import torch

from ld_amd import build_detector, model_zoo
from ld_amd.cnn import BatchNorm2d, DeformConv2dPack
from ld_amd.config import Config
from ld_amd.registry import build_backbone

REFERENCE = os.environ.get('LD_REFERENCE_ROOT', '/root/reference')
HAVE_REF = os.path.isdir(os.path.join(REFERENCE, 'configs'))
R2N_CONFIGS = ['configs/imv2/gflv2_r2n101_dcn_fpn_2x.py',
               'configs/im/gflv2_r2n101_dcn_fpn_2x.py']


def _plain(o):
    """Config nodes / tuples -> plain dicts / lists, for comparing settings."""
    if hasattr(o, 'items'):
        return {k: _plain(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_plain(v) for v in o]
    return o


def _shapes(sd):
    return ['x'.join(str(v) for v in t.shape) for t in sd.values()]


@pytest.mark.parametrize('depth', [50, 101])
def test_registry_build_matches_reference_keys(golden, depth):
    g = golden['res2net']
    net = build_backbone(dict(type='Res2Net', depth=depth, scales=4,
                              base_width=26))
    sd = net.state_dict()
    assert list(sd) == [str(k) for k in g[f'd{depth}_keys']]
    assert _shapes(sd) == [str(s) for s in g[f'd{depth}_shapes']]
    assert not any(k.startswith(('conv1', 'bn1')) for k in sd)
    assert [getattr(net, f'layer{i + 1}')[0].width for i in range(4)] == \
        [26, 52, 104, 208]
    for i in range(4):
        layer = getattr(net, f'layer{i + 1}')
        assert layer[0].stage_type == 'stage'
        assert all(b.stage_type == 'normal' for b in list(layer)[1:])
        assert not any(k.startswith(('conv2', 'bn2'))
                       for k in layer[0].state_dict())


def test_plain_resnet_keeps_refusing_the_variants():
    for kw in (dict(deep_stem=True), dict(avg_down=True)):
        with pytest.raises(NotImplementedError):
            build_backbone(dict(type='ResNet', depth=50, **kw))


def test_frozen_stages_and_norm_eval():
    net = build_backbone(model_zoo._r2n_backbone(50, dcn=False))
    net.train()
    frozen = [k for k, p in net.named_parameters() if not p.requires_grad]
    assert frozen and all(k.startswith(('stem.', 'layer1.')) for k in frozen)
    assert all(not p.requires_grad for p in net.stem.parameters())
    assert all(not p.requires_grad for p in net.layer1.parameters())
    assert all(p.requires_grad for n in ('layer2', 'layer3', 'layer4')
               for p in getattr(net, n).parameters())
    bns = [m for m in net.modules() if isinstance(m, BatchNorm2d)]
    assert bns and not any(m.training for m in bns)
    assert not net.stem.training and not net.layer1.training
    assert net.layer2.training
    # bf16 mode never takes this backbone C8-only
    assert net._c8_only() is False and net._frozen_c8_stages() == 0


def test_dcn_variant_has_78_zero_offset_dcns(golden):
    cfg = model_zoo._r2n_backbone(101, dcn=True)
    assert cfg['stage_with_dcn'] == (False, False, True, True)
    net = build_backbone(cfg)
    # a non-zero starting point, so that init_weights is what zeroes them
    for m in net.modules():
        if isinstance(m, DeformConv2dPack):
            torch.nn.init.constant_(m.conv_offset.weight, 0.5)
            torch.nn.init.constant_(m.conv_offset.bias, 0.5)
    net.init_weights(None)
    dcns = [(k, m) for k, m in net.named_modules()
            if isinstance(m, DeformConv2dPack)]
    assert len(dcns) == 3 * (23 + 3) == 78
    assert all(k.startswith(('layer3.', 'layer4.')) and '.convs.' in k
               for k, _ in dcns)
    for _, m in dcns:
        assert m.in_channels == m.out_channels and m.in_channels in (104, 208)
        assert float(m.conv_offset.weight.detach().abs().max()) == 0.0
        assert float(m.conv_offset.bias.detach().abs().max()) == 0.0
    # the DCN keys by construction: the plain keys + convs.i.conv_offset.*
    plain = [str(k) for k in golden['res2net']['d101_keys']]
    extra = {f'{k}.convs.{i}.conv_offset.{p}'
             for k in {k.rsplit('.convs.', 1)[0] for k, _ in dcns}
             for i in range(3) for p in ('weight', 'bias')}
    assert set(net.state_dict()) == set(plain) | extra
    assert len(extra) == 2 * 78


def test_model_zoo_entries():
    t = model_zoo.gflv2_r2n101_dcn_detector()
    assert t['backbone'] == dict(
        type='Res2Net', depth=101, num_stages=4, scales=4, base_width=26,
        out_indices=(0, 1, 2, 3), frozen_stages=1,
        norm_cfg=dict(type='BN', requires_grad=True),
        dcn=dict(type='DCN', deform_groups=1, fallback_on_stride=False),
        stage_with_dcn=(False, False, True, True), norm_eval=True,
        style='pytorch')
    assert t['bbox_head']['type'] == 'GFocalHead' and t['pretrained'] is None
    kd = model_zoo.ldv2_x101_r2n101_detector()
    assert kd['bbox_head']['type'] == 'LDv2Head'
    assert kd['backbone'] == model_zoo._x101_backbone(101, dcn=True)
    assert kd['teacher_config']['model'] == t


@pytest.mark.skipif(not HAVE_REF,
                    reason='needs the reference checkout (build container)')
@pytest.mark.parametrize('path', R2N_CONFIGS)
def test_reference_r2n_configs_build_in_train_mode(monkeypatch, path):
    monkeypatch.chdir(REFERENCE)
    monkeypatch.setenv('LD_ALLOW_MISSING_CKPT', '1')
    cfg = Config.fromfile(path)
    assert cfg.model['pretrained'] == 'open-mmlab://res2net101_v1d_26w_4s'
    with pytest.warns(UserWarning):
        det = build_detector(dict(cfg.model), train_cfg=cfg.get('train_cfg'),
                             test_cfg=cfg.get('test_cfg'))
    det.train()
    assert type(det).__name__ == 'GFL'
    assert type(det.backbone).__name__ == 'Res2Net'
    assert sum(isinstance(m, DeformConv2dPack)
               for m in det.backbone.modules()) == 78
    zoo = build_detector(model_zoo.gflv2_r2n101_dcn_detector())
    assert list(det.state_dict()) == list(zoo.state_dict())
    assert _shapes(det.state_dict()) == _shapes(zoo.state_dict())
    want = dict(cfg.model)
    want['pretrained'] = None
    mine = model_zoo.gflv2_r2n101_dcn_detector()
    mine.pop('train_cfg')
    mine.pop('test_cfg')
    assert _plain(want) == _plain(mine)


def test_glue_entry_points_validate_without_gpu():
    """Null pointers and bad geometry: LD_EINVAL (-1) before any launch."""
    from ld_amd import lib as L
    lib = L.get_lib()
    p = C.c_void_p(4096)  # never dereferenced: every call below is refused
    assert lib.ld_res2_gather(None, None, 2, 104, 26, 0, 63, p, None) == -1
    assert lib.ld_res2_gather(p, None, 2, 104, 26, 0, 63, None, None) == -1
    assert lib.ld_res2_gather(p, None, 0, 104, 26, 0, 63, p, None) == -1
    assert lib.ld_res2_gather(p, None, 2, 104, 26, 4, 63, p, None) == -1
    assert lib.ld_res2_gather(p, None, 2, 104, 26, -1, 63, p, None) == -1
    assert lib.ld_res2_gather(p, None, 2, 104, 0, 0, 63, p, None) == -1
    assert lib.ld_res2_gather(p, None, 2, 104, 26, 0, 0, p, None) == -1
    assert lib.ld_res2_gather(p, None, 70000, 104, 26, 0, 63, p, None) == -1
    ok = (p, p, p, p, 2, 26, 104, 3, 7, 9, 2, 1, p, None)

    def cat(**kw):
        names = ('a', 'b', 'c', 't', 'N', 'w', 'Ct', 'tslice', 'H', 'W',
                 'stride', 'mode', 'y', 'stream')
        args = dict(zip(names, ok))
        args.update(kw)
        return lib.ld_res2_concat(*[args[n] for n in names])
    for name in ('a', 'b', 'c', 't', 'y'):
        assert cat(**{name: None}) == -1
    for kw in (dict(N=0), dict(w=0), dict(tslice=4), dict(tslice=-1),
               dict(Ct=103), dict(H=0), dict(W=-3), dict(stride=0),
               dict(mode=3), dict(mode=-1), dict(H=1 << 16, W=1 << 16)):
        assert cat(**kw) == -1, kw
    for fn in (lib.ld_avgpool_ceil_forward, lib.ld_avgpool_ceil_backward):
        assert fn(None, 4, 7, 9, 2, p, None) == -1
        assert fn(p, 4, 7, 9, 2, None, None) == -1
        assert fn(p, 0, 7, 9, 2, p, None) == -1
        assert fn(p, 4, 0, 9, 2, p, None) == -1
        assert fn(p, 4, 7, 0, 2, p, None) == -1
        assert fn(p, 4, 7, 9, 0, p, None) == -1
