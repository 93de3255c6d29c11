"""Host tests of the trainable ResNeXt configs: the three model_zoo X-101
detectors are the reference config files' resolved ``model`` entries, the
trainable and the frozen ResNeXt share their state-dict keys, and the grouped
backward's C ABI is declared in include/ld_hip.h (tests/test_cabi.py then checks
every declared symbol is exported)."""
import os
import re

import numpy as np
import pytest
import torch

from ld_amd import build_backbone, build_detector, model_zoo
from ld_amd.config import Config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get('LD_REFERENCE_ROOT', '/root/reference')
HAVE_REF = os.path.isdir(os.path.join(REFERENCE, 'configs', 'imv2'))

ZOO = [
    ('configs/gfl/gfl_x101_32x4d_fpn_mstrain_2x_coco.py',
     model_zoo.gfl_x101_detector),
    ('configs/gfl/gfl_x101_32x4d_fpn_dconv_c4-c5_mstrain_2x_coco.py',
     model_zoo.gfl_x101_dcn_detector),
    ('configs/imv2/gflv2_x101_fpn_2x_coco.py',
     lambda: model_zoo.gflv2_x101_detector(dcn=True)),
]


def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


@pytest.mark.skipif(not HAVE_REF,
                    reason='needs the reference checkout (build container)')
@pytest.mark.parametrize('path,zoo', ZOO, ids=[p.split('/')[-1] for p, _ in ZOO])
def test_zoo_dict_is_the_reference_config(path, zoo, monkeypatch):
    """Key for key, value for value; ``pretrained`` apart (the zoo builds from
    seeded weights: the open-mmlab checkpoint is not available offline)."""
    monkeypatch.chdir(REFERENCE)
    ref = _plain(Config.fromfile(path).model)
    ours = _plain(zoo())
    assert ref.pop('pretrained') == 'open-mmlab://resnext101_32x4d'
    assert ours.pop('pretrained') is None
    assert ours == ref


def test_trainable_and_frozen_resnext_share_state_dict_keys():
    cfg = model_zoo._x101_backbone(50, dcn=True)
    train = build_backbone(cfg).train()
    frozen = build_backbone(cfg).requires_grad_(False).eval()
    assert any(p.requires_grad for p in train.parameters())
    a, b = train.state_dict(), frozen.state_dict()
    assert list(a) == list(b)
    assert [tuple(v.shape) for v in a.values()] == \
        [tuple(v.shape) for v in b.values()]


def test_x101_detectors_differ_only_in_the_backbone():
    base = model_zoo.gfl_detector(101)
    for cfg in (model_zoo.gfl_x101_detector(), model_zoo.gfl_x101_dcn_detector()):
        assert cfg['backbone']['type'] == 'ResNeXt'
        assert {k: v for k, v in cfg.items() if k != 'backbone'} == \
            {k: v for k, v in base.items() if k != 'backbone'}
    assert 'dcn' not in model_zoo.gfl_x101_detector()['backbone']
    assert model_zoo.gflv2_x101_detector()['backbone']['stage_with_dcn'] == \
        (False, False, True, True)
    assert model_zoo.gflv2_x101_detector()['bbox_head']['type'] == 'GFocalHead'


def test_grouped_backward_abi_is_declared():
    with open(os.path.join(ROOT, 'include', 'ld_hip.h')) as f:
        header = f.read()
    for sym in ('ld_gconv_weight_image_bwd_floats',
                'ld_gconv_weight_transform_bwd', 'ld_gconv_dgrad',
                'ld_gconv_wgrad', 'ld_gconv_wgrad_slabs',
                'ld_gconv_wgrad_workspace_floats'):
        assert re.search(r'\b' + sym + r'\s*\(', header), sym


def test_paramwise_cfg_treats_grouped_convs_as_mmcv_does():
    """DefaultOptimizerConstructor: a conv is depthwise only when groups ==
    in_channels, so ResNeXt's grouped conv2 (groups 32, 128+ channels) takes the
    plain decay, norms take norm_decay_mult, frozen parameters the defaults."""
    from ld_amd.cnn import GroupedConv2d
    from ld_amd.optim import classify
    det = build_detector(model_zoo.gfl_x101_detector()).train()
    names, mults = classify(det, dict(dwconv_decay_mult=0.0, norm_decay_mult=0.5))
    by = dict(zip(names, mults))
    params = dict(det.named_parameters())
    grouped = [k + '.weight' for k, m in det.named_modules()
               if isinstance(m, GroupedConv2d)]
    assert len(grouped) == 33
    assert all(m.groups != m.in_channels for m in det.modules()
               if isinstance(m, GroupedConv2d))
    assert all(by[k] == (1.0, 1.0) for k in grouped)
    assert by['backbone.layer2.0.bn2.weight'] == (1.0, 0.5)
    assert by['backbone.layer1.0.bn2.weight'] == (1.0, 1.0)  # frozen
    assert not params['backbone.layer1.0.conv2.weight'].requires_grad
    assert params['backbone.layer2.0.conv2.weight'].requires_grad


def test_restatement_forward_is_the_reference_resnext(golden):
    """tests/_gconv_ref64.resnext_forward in float64 against the reference's
    own ResNeXt (tests/golden/resnext.npz, case x50_odd)."""
    import _gconv_ref64 as R
    from ld_amd import synthetic
    g = golden['resnext']
    depth, n, h, w, seed, step = [int(v) for v in g['x50_odd_cfg']]
    net = build_backbone(model_zoo._x101_backbone(depth))
    sd = synthetic.seeded_state_dict(net.state_dict(), seed=seed)
    x = torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(seed + 100))
    with torch.no_grad():
        outs = R.resnext_forward({k: v.double() for k, v in sd.items()},
                                 x.double())
    for i, o in enumerate(outs):
        ref = g[f'x50_odd_out{i}'].astype(np.float64)
        got = o.numpy().reshape(-1)[::step]
        assert float(np.abs(got - ref).max()) <= 2e-4 * float(np.abs(ref).max())


def test_block_diagonal_embedding_is_the_grouped_conv():
    import _gconv_ref64 as R
    g = torch.Generator().manual_seed(2)
    w = torch.randn(16, 3, 3, 3, generator=g, dtype=torch.float64)
    x = torch.randn(1, 12, 5, 6, generator=g, dtype=torch.float64)
    dense, mask = R.block_diagonal(w, 4)
    assert int(mask.sum()) == w.numel() and bool((dense * (1 - mask) == 0).all())
    a = torch.nn.functional.conv2d(x, w, None, 1, 1, 1, 4)
    b = torch.nn.functional.conv2d(x, dense, None, 1, 1)
    assert float((a - b).abs().max()) < 1e-12
