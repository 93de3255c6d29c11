"""The trainable GFL-R101-DCN teacher as a config: model_zoo.gfl_dcn_detector is
configs/gfl/gfl_r101_fpn_dconv_c3-c5_mstrain_2x_coco.py, which builds through
the registry in train mode with 30 trainable DCNv1 layers and hands SGDTrainer
a plain SGD recipe (no paramwise_cfg: that stays refused on a trainable DCN)."""
import os

import pytest

from ld_amd import build_detector, model_zoo
from ld_amd.cnn import DeformConv2dPack
from ld_amd.config import Config

REFERENCE = os.environ.get('LD_REFERENCE_ROOT', '/root/reference')
HAVE_REF = os.path.isdir(os.path.join(REFERENCE, 'configs'))
DCONV = 'configs/gfl/gfl_r101_fpn_dconv_c3-c5_mstrain_2x_coco.py'


def _dcn_layers(det):
    return [(k, m) for k, m in det.named_modules()
            if isinstance(m, DeformConv2dPack)]


def test_gfl_dcn_detector_is_trainable_dcn_in_c3_c5():
    det = build_detector(model_zoo.gfl_dcn_detector(101))
    det.train()
    layers = _dcn_layers(det)
    assert len(layers) == 4 + 23 + 3
    assert all(k.startswith(('backbone.layer2', 'backbone.layer3',
                             'backbone.layer4')) and k.endswith('conv2')
               for k, _ in layers)
    for _, m in layers:
        assert m.deform_groups == 1 and m.groups == 1
        assert all(p.requires_grad for p in m.parameters())
        assert float(m.conv_offset.weight.detach().abs().max()) == 0.0
    cfg = model_zoo.gfl_dcn_detector(101)
    plain = model_zoo.gfl_detector(101)
    assert cfg['backbone'].pop('dcn') == dict(type='DCN', deform_groups=1,
                                              fallback_on_stride=False)
    assert cfg['backbone'].pop('stage_with_dcn') == (False, True, True, True)
    assert cfg == plain


@pytest.mark.skipif(not HAVE_REF,
                    reason='needs the reference checkout (build container)')
def test_reference_dconv_config_builds_in_train_mode(monkeypatch):
    monkeypatch.chdir(REFERENCE)
    monkeypatch.setenv('LD_ALLOW_MISSING_CKPT', '1')
    cfg = Config.fromfile(DCONV)
    with pytest.warns(UserWarning):
        det = build_detector(dict(cfg.model), train_cfg=cfg.get('train_cfg'),
                             test_cfg=cfg.get('test_cfg'))
    det.train()
    assert type(det).__name__ == 'GFL'
    assert len(_dcn_layers(det)) == 30
    zoo = build_detector(model_zoo.gfl_dcn_detector(101))
    assert list(det.state_dict()) == list(zoo.state_dict())
    assert [tuple(v.shape) for v in det.state_dict().values()] == \
        [tuple(v.shape) for v in zoo.state_dict().values()]
    assert cfg.optimizer.get('paramwise_cfg') is None
    assert cfg.optimizer['type'] == 'SGD'
