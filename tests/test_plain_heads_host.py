"""Plain ATSS / RetinaNet on the CPU: the detectors of
configs/atss/atss_r50_fpn_1x_coco.py and
configs/retinanet/retinanet_r50_fpn_1x_coco.py build through build_detector,
the heads' state_dict keys are the reference's (tests/golden/plain_heads.npz,
written by tools/gen_golden_plain_heads.py), what the heads do not implement is
refused by name, and the numpy restatement of DeltaXYWHBBoxCoder
(tests/_delta_coder.py) equals the reference's stored rows.

Before ATSSHead / RetinaHead / L1Loss were registered every test here but the
numpy-coder and golden-geometry ones failed: at the missing zoo entry or at the
registry lookup."""
import copy
import os

import numpy as np
import pytest
import torch

from ld_amd import Config, build_detector, model_zoo, registry
from ld_amd import synthetic as S

import _delta_coder as DC

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden', 'plain_heads.npz')
from test_boundary import REFERENCE  # the reference checkout, when present

HAVE_REF = os.path.isdir(os.path.join(REFERENCE, 'configs', 'atss'))


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


ZOO = [('atss', 'atss_detector', 'ATSS', 'ATSSHead'),
       ('retina', 'retinanet_detector', 'RetinaNet', 'RetinaHead')]


@pytest.mark.parametrize('kind,make,det_type,head_type', ZOO,
                         ids=[z[0] for z in ZOO])
def test_zoo_detector_builds_with_reference_keys(kind, make, det_type,
                                                 head_type, gold):
    make = getattr(model_zoo, make)
    det = build_detector(make(50))
    assert type(det).__name__ == det_type
    head = det.bbox_head
    assert type(head).__name__ == head_type
    assert list(head.state_dict().keys()) == [str(k) for k in
                                              gold[f'keys_{kind}']]
    # the box branch: 4 deltas per anchor
    reg = head.atss_reg if kind == 'atss' else head.retina_reg
    assert reg.weight.shape[0] == head.num_anchors * 4
    assert head.num_anchors == (1 if kind == 'atss' else 9)
    assert registry.build_loss(dict(type='L1Loss')).loss_weight == 1.0
    # R101 comes with the depth argument
    assert build_detector(make(101)).backbone.depth == 101


@pytest.mark.skipif(not HAVE_REF,
                    reason='needs the reference checkout (build container)')
@pytest.mark.parametrize('path,head_type', [
    ('configs/atss/atss_r50_fpn_1x_coco.py', 'ATSSHead'),
    ('configs/atss/atss_r101_fpn_1x_coco.py', 'ATSSHead'),
    ('configs/retinanet/retinanet_r50_fpn_1x_coco.py', 'RetinaHead'),
    ('configs/retinanet/retinanet_r101_fpn_2x_coco.py', 'RetinaHead'),
    ('configs/retinanet/retinanet_x101_32x4d_fpn_1x_coco.py', 'RetinaHead')])
def test_reference_config_files_build(path, head_type, monkeypatch):
    monkeypatch.chdir(REFERENCE)
    monkeypatch.setenv('LD_ALLOW_MISSING_CKPT', '1')
    cfg = Config.fromfile(path)
    with pytest.warns(UserWarning):
        det = build_detector(dict(cfg.model), train_cfg=cfg.get('train_cfg'),
                             test_cfg=cfg.get('test_cfg'))
    assert type(det.bbox_head).__name__ == head_type
    # the zoo entry is the r50 file, value for value
    if path.endswith('_r50_fpn_1x_coco.py'):
        zoo = model_zoo.atss_detector(50) if head_type == 'ATSSHead' \
            else model_zoo.retinanet_detector(50)

        def plain(o):
            if isinstance(o, dict):
                return {k: plain(v) for k, v in o.items()}
            if isinstance(o, (list, tuple)):
                return [plain(v) for v in o]
            return o
        ref = plain(dict(cfg.model))
        for k in ('bbox_head', 'neck', 'backbone', 'train_cfg', 'test_cfg'):
            assert plain(zoo[k]) == ref[k], k


def _head(kind, train_over=None, **over):
    m = (model_zoo.atss_detector if kind == 'atss'
         else model_zoo.retinanet_detector)(50)
    cfg = dict(m['bbox_head'], num_classes=S.PLAIN_CLASSES,
               in_channels=S.PLAIN_FEAT, feat_channels=S.PLAIN_FEAT)
    if kind == 'atss':
        cfg['norm_cfg'] = dict(type='GN', num_groups=S.PLAIN_FEAT,
                               requires_grad=True)
    cfg.update(over)
    train = copy.deepcopy(m['train_cfg'])
    train.update(train_over or {})
    cfg.update(train_cfg=Config(train), test_cfg=Config(m['test_cfg']))
    return registry.build_head(cfg)


def _loss_call(kind, head):
    """head.loss on CPU tensors: a refusal must come before any device work."""
    hi = S.plain_head_inputs(kind, 1)
    batch = S.plain_batch('multi')
    outs = [hi['cls'], hi['reg']] + ([hi['ctr']] if kind == 'atss' else [])
    return head.loss(*outs, batch['gt_bboxes'], batch['gt_labels'],
                     batch['img_metas'])


FOCAL = dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25,
             loss_weight=1.0)


@pytest.mark.parametrize('kind', ['atss', 'retina'])
def test_refusals_by_name(kind):
    with pytest.raises(NotImplementedError, match='pos_weight'):
        _loss_call(kind, _head(kind, train_over=dict(pos_weight=2.0)))
    with pytest.raises(NotImplementedError, match='allowed_border'):
        _loss_call(kind, _head(kind, train_over=dict(allowed_border=0)))
    with pytest.raises(NotImplementedError, match='gamma'):
        _loss_call(kind, _head(kind, loss_cls=dict(FOCAL, gamma=1.5)))
    hi, metas = S.plain_infer_inputs(kind)
    outs = [hi['cls'], hi['reg']] + ([hi['ctr']] if kind == 'atss' else [])
    head = _head(kind)
    cfg = Config(dict(head.test_cfg, min_bbox_size=2))
    with pytest.raises(NotImplementedError, match='min_bbox_size'):
        head.get_bboxes(*outs, metas, cfg=cfg)


def test_retina_refuses_sampling_loss_cls_and_odd_box_losses():
    head = _head('retina', loss_cls=dict(type='CrossEntropyLoss',
                                         use_sigmoid=True, loss_weight=1.0))
    assert head.sampling
    with pytest.raises(NotImplementedError, match='sampling loss_cls'):
        _loss_call('retina', head)
    # GIoU on raw deltas, L1 on decoded boxes: neither is a reference recipe
    with pytest.raises(NotImplementedError, match='L1Loss or SmoothL1Loss'):
        _loss_call('retina', _head('retina', loss_bbox=dict(type='GIoULoss')))
    with pytest.raises(NotImplementedError, match='reg_decoded_bbox=True'):
        _loss_call('retina', _head('retina', reg_decoded_bbox=True))
    # the configs that are built
    for over in (dict(), dict(loss_bbox=dict(type='SmoothL1Loss',
                                             beta=1.0 / 9.0)),
                 dict(reg_decoded_bbox=True,
                      loss_bbox=dict(type='GIoULoss', loss_weight=2.0))):
        _head('retina', **over)._check_loss_cfg()


@pytest.mark.parametrize('coder', ['atss', 'retina'])
def test_numpy_coder_equals_reference_rows(coder, gold):
    """Encode and decode within 1e-6 relative of the reference's own fp32 rows
    (relative to the row's largest coordinate, see _delta_coder.close_rows):
    same operations in the same order, exp / log at most an ulp apart."""
    anchors, gts, deltas = [t.numpy() for t in S.delta_coder_rows()]
    means, stds = S.PLAIN_CODERS[coder]
    assert anchors.shape == (S.DELTA_ROWS, 4)
    assert (anchors[:, 2] - anchors[:, 0]).min() == 1.0  # degenerate anchors
    checks = [
        ('enc', DC.bbox2delta(anchors, gts, means, stds)),
        ('dec', DC.delta2bbox(anchors, deltas, means, stds)),
        ('dec_clip', DC.delta2bbox(anchors, deltas, means, stds,
                                   max_shape=S.DELTA_MAX_SHAPE))]
    for name, got in checks:
        ok, worst = DC.close_rows(got, gold[f'coder_{coder}_{name}'], 1e-6)
        assert ok, (name, worst)
    clip = gold[f'coder_{coder}_dec_clip']
    assert clip.min() == 0.0 and clip[:, 0::2].max() == S.DELTA_MAX_SHAPE[1]


def test_golden_geometry(gold):
    """What the issue asks of the stored cases, read off the reference's own
    targets: ATSS positives on >= 3 levels, RetinaNet positives on >= 2 levels
    and an ignore band, an image without GT, a batch without positives."""
    assert (gold['atss_multi_pos'] > 0).sum() >= 3
    assert (gold['retina_l1_multi_pos'] > 0).sum() >= 2
    assert int(gold['retina_l1_multi_ignored']) >= 1
    assert S.PLAIN_CASES['empty_img'][1] == []
    assert gold['atss_no_pos_pos'].sum() == 0
    assert gold['retina_l1_no_pos_pos'].sum() == 0
    # bbox_avg_factor < EPS -> 1: zero box and centerness rows, finite class row
    assert (gold['atss_no_pos_losses'][1:] == 0).all()
    assert np.isfinite(gold['atss_no_pos_losses']).all()
