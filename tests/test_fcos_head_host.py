"""Plain FCOS on the CPU: the float64 restatement of tests/_fcos_ref64.py
(targets, box branch, loss, decode) equals the REFERENCE's own FCOSHead outputs
(tests/golden/fcos_head.npz, written by tools/gen_golden_fcos_head.py); the
zoo's two configs -- configs/fcos/fcos_r50_caffe_fpn_gn-head_1x_coco.py and
fcos_center-normbbox-centeronreg-giou_r50_caffe_fpn_gn-head_1x_coco.py -- read
back through Config.fromfile build the detector and its SGDTrainer; the head's
state_dict keys are the reference's; what the head does not implement is
refused by name.

Before the feature every test here failed at the registry lookup of FCOSHead
(the module's autouse fixture builds the head first)."""
import os

import numpy as np
import pytest
import torch

from ld_amd import Config, build_detector, model_zoo, registry
from ld_amd import synthetic as S

import _fcos_ref64 as R

HERE = os.path.dirname(os.path.abspath(__file__))
# the bars of tests/test_gpu_plain_heads.py
LOSS_TOL = dict(rtol=1e-4, atol=1e-4)
GRAD_TOL = dict(rtol=5e-4, atol=1e-7)
BOX_ATOL, SCORE_ATOL = 2e-3, 1e-6

CASES = [(v, c) for v in S.FCOS_VARIANTS for c in S.PLAIN_CASES
         if v == 'plain' or c == 'multi']
BBOX_LOSS = dict(IoULoss='iou', GIoULoss='giou')


@pytest.fixture(scope='module', autouse=True)
def fcos_head_registered():
    """Every test of this file is about FCOSHead: look it up first."""
    return registry.build_head(dict(
        type='FCOSHead', num_classes=S.PLAIN_CLASSES, in_channels=8,
        feat_channels=8, norm_cfg=dict(type='GN', num_groups=8,
                                       requires_grad=True)))


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(HERE, 'golden', 'fcos_head.npz'))


def small_head(variant='plain', nms_pre=1000, **over):
    """The zoo config's head at the fixture's size: 4 classes, 8 channels."""
    m = model_zoo.fcos_detector(50)
    cfg = dict(m['bbox_head'], num_classes=S.PLAIN_CLASSES,
               in_channels=S.PLAIN_FEAT, feat_channels=S.PLAIN_FEAT,
               norm_cfg=dict(type='GN', num_groups=S.PLAIN_FEAT,
                             requires_grad=True))
    cfg.update(S.FCOS_VARIANTS[variant])
    cfg.update(over)
    cfg.update(train_cfg=Config(m['train_cfg']),
               test_cfg=Config(dict(m['test_cfg'], nms_pre=nms_pre)))
    return registry.build_head(cfg)


def ref64_case(head, case, labels=None, targets=None, bbox_loss=None):
    """The float64 loss table of ``head``'s settings on a PLAIN_CASES case and
    the leaves autograd filled: (table (3, L), maps, scales)."""
    batch = S.plain_batch(case)
    sizes = S.level_shapes(S.PLAIN_PAD)
    if labels is None:
        labels, targets = R.fcos_targets(
            batch['gt_bboxes'], batch['gt_labels'], sizes, head.strides,
            head.num_classes, head.center_sampling, head.center_sample_radius,
            head.regress_ranges)
    hi = S.fcos_head_inputs(S.PLAIN_SEEDS[case], relu=head.norm_on_bbox)
    maps = {k: [t.double().requires_grad_(True) for t in v]
            for k, v in hi.items()}
    scales = torch.tensor(S.FCOS_SCALES, dtype=torch.float64,
                          requires_grad=True)
    table = R.fcos_loss(
        maps, scales, labels, targets, head.strides, head.num_classes,
        norm_on_bbox=head.norm_on_bbox,
        bbox_loss=bbox_loss or BBOX_LOSS[type(head.loss_bbox).__name__],
        eps=head.loss_bbox.eps, lw_bbox=head.loss_bbox.loss_weight)
    table.sum().backward()
    return table.detach(), maps, scales, labels


@pytest.mark.parametrize('variant,case', CASES,
                         ids=[f'{v}-{c}' for v, c in CASES])
def test_restatement_equals_reference(variant, case, gold):
    head = small_head(variant)
    table, maps, scales, labels = ref64_case(head, case)
    key = f'{variant}_{case}'
    # targets: positives per level
    off, pos = 0, []
    for h, w in S.level_shapes(S.PLAIN_PAD):
        lab = labels[:, off:off + h * w]
        pos.append(int(((lab >= 0) & (lab < head.num_classes)).sum()))
        off += h * w
    assert pos == gold[key + '_pos'].tolist()
    np.testing.assert_allclose(table.sum(1).numpy(), gold[key + '_losses'],
                               **LOSS_TOL)
    for k in ('cls', 'raw', 'ctr'):
        for l, t in enumerate(maps[k]):
            np.testing.assert_allclose(t.grad.numpy(),
                                       gold[f'{key}_g{k}_{l}'], **GRAD_TOL,
                                       err_msg=f'{k}[{l}]')
    np.testing.assert_allclose(scales.grad.numpy(), gold[key + '_gscales'],
                               rtol=5e-4, atol=1e-6)


def test_golden_geometry(gold):
    """The cases the issue names, read off the reference's own targets."""
    assert gold['plain_multi_pos'].tolist() == [118, 48, 16, 0, 0]
    assert gold['plain_empty_img_pos'].tolist() == [88, 16, 0, 0, 0]
    assert gold['center_multi_pos'].tolist() == [21, 4, 4, 0, 0]
    assert gold['tricks_multi_pos'].tolist() == [21, 4, 4, 0, 0]
    assert gold['plain_no_pos_pos'].sum() == 0
    assert (gold['plain_no_pos_losses'][1:] == 0).all()
    for k in ('raw', 'ctr'):
        for l in range(5):
            assert not gold[f'plain_no_pos_g{k}_{l}'].any()
    # one point of 'multi' lies inside two GT boxes' regress ranges
    batch = S.plain_batch('multi')
    sizes = S.level_shapes(S.PLAIN_PAD)
    pts = torch.cat([R.points(h, w, s)
                     for (h, w), s in zip(sizes, S.FCOS_STRIDES)])
    rr = torch.cat([torch.tensor([r], dtype=torch.float64).expand(h * w, 2)
                    for (h, w), r in zip(sizes, R.REGRESS_RANGES)])
    both = 0
    for gb in batch['gt_bboxes']:
        gb = gb.double()
        t = torch.stack([pts[:, 0:1] - gb[None, :, 0],
                         pts[:, 1:2] - gb[None, :, 1],
                         gb[None, :, 2] - pts[:, 0:1],
                         gb[None, :, 3] - pts[:, 1:2]], -1)
        ok = (t.min(-1)[0] > 0) & (t.max(-1)[0] >= rr[:, 0:1]) & \
            (t.max(-1)[0] <= rr[:, 1:2])
        both += int((ok.sum(1) >= 2).sum())
    assert both >= 1
    # the ReLU fixtures: a zero-area box costs -log(eps) and moves nothing
    n, l, y, x = S.FCOS_NEG['all']
    assert not gold[f'norm_iou_multi_graw_{l}'][n, :, y, x].any()
    n, l, y, x = S.FCOS_NEG['one']
    g = gold[f'tricks_multi_graw_{l}'][n, :, y, x]
    assert g[S.FCOS_NEG_CH] == 0 and (g != 0).sum() == 3


def test_forward_golden_carries_the_stride_factor(gold):
    for l, s in enumerate(S.FCOS_STRIDES):
        tr, ev = (gold[f'fwd_tricks_{m}_reg_{l}'] for m in ('train', 'eval'))
        assert (tr >= 0).all() and (tr == 0).any()
        np.testing.assert_array_equal(ev, tr * np.float32(s))
        assert (gold[f'fwd_plain_train_reg_{l}'] > 0).all()


def test_decode_restatement_equals_reference(gold):
    hi, metas = S.fcos_infer_inputs()
    nms_pre = S.PLAIN_INFER['nms_pre']
    for i, meta in enumerate(metas):
        rows = [R.decode_level(hi['cls'][l][i].double(),
                               hi['reg'][l][i].double(),
                               hi['ctr'][l][i].double(), s,
                               meta['img_shape'], nms_pre)
                for l, s in enumerate(S.FCOS_STRIDES)]
        boxes, scores, fac = (torch.cat([r[k] for r in rows]).numpy()
                              for k in range(3))
        np.testing.assert_allclose(boxes, gold[f'pre_bboxes_{i}'],
                                   atol=BOX_ATOL, rtol=0)
        np.testing.assert_allclose(scores, gold[f'pre_scores_{i}'][:, :-1],
                                   atol=SCORE_ATOL, rtol=0)
        assert not gold[f'pre_scores_{i}'][:, -1].any()
        np.testing.assert_allclose(fac, gold[f'pre_factors_{i}'],
                                   atol=SCORE_ATOL, rtol=0)
    h, w = S.PLAIN_INFER['img_shapes'][1][:2]
    assert gold['pre_bboxes_1'][:, 2].max() == w
    assert gold['pre_bboxes_1'][:, 3].max() == h


# ------------------------------------------------------- zoo and configs --
@pytest.mark.parametrize('tricks', [False, True], ids=['plain', 'tricks'])
def test_zoo_detector_builds_with_reference_keys(tricks, gold):
    det = build_detector(model_zoo.fcos_detector(50, tricks=tricks))
    assert type(det).__name__ == 'FCOS'
    head = det.bbox_head
    assert type(head).__name__ == 'FCOSHead'
    assert list(head.state_dict().keys()) == [
        str(k) for k in gold['keys_tricks' if tricks else 'keys_plain']]
    assert head.conv_reg.weight.shape[0] == 4
    assert head.conv_centerness.weight.shape[:2] == (1, 256)
    assert head.norm_on_bbox == head.centerness_on_reg == \
        head.center_sampling == tricks
    assert type(head.loss_bbox).__name__ == \
        ('GIoULoss' if tricks else 'IoULoss')
    assert head.test_cfg['nms']['iou_threshold'] == (0.6 if tricks else 0.5)
    assert det.backbone.style == 'caffe'
    assert build_detector(model_zoo.fcos_detector(101)).backbone.depth == 101
    # FCOSGFLHead is what it was: 68 channels, centerness on the reg tower
    gfl = build_detector(model_zoo.fcos_gfl_detector(50)).bbox_head
    assert gfl.conv_reg.weight.shape[0] == 68 and hasattr(gfl, 'integral')


@pytest.mark.parametrize('tricks', [False, True], ids=['plain', 'tricks'])
def test_config_file_builds_detector_and_trainer(tricks, tmp_path):
    """The zoo's settings written out as a config file and read back with
    Config.fromfile: build_detector and SGDTrainer.from_config take them."""
    from ld_amd.train import SGDTrainer
    text = f'model = {model_zoo.fcos_detector(50, tricks=tricks)!r}\n'
    for k, v in model_zoo.fcos_schedule(tricks).items():
        text += f'{k} = {v!r}\n'
    path = tmp_path / ('fcos_tricks.py' if tricks else 'fcos_plain.py')
    path.write_text(text)
    cfg = Config.fromfile(str(path))
    det = build_detector(dict(cfg.model), train_cfg=cfg.get('train_cfg'),
                         test_cfg=cfg.get('test_cfg'))
    assert type(det.bbox_head).__name__ == 'FCOSHead'
    tr = SGDTrainer.from_config(det, cfg)
    mults = set(tr.param_classes.mults)
    assert (2.0, 0.0) in mults and (1.0, 1.0) in mults  # bias_lr / decay mult
    if tricks:
        assert tr.grad_clip is None
        assert cfg.lr_config['warmup'] == 'linear'
    else:
        assert tr.grad_clip == dict(max_norm=35.0, norm_type=2)
        assert cfg.lr_config['warmup'] == 'constant'
    assert tr.lr_schedule is not None


# --------------------------------------------------------------- refusals --
def test_refusals_by_name():
    with pytest.raises(NotImplementedError, match='dcn_on_last_conv'):
        small_head(dcn_on_last_conv=True)
    focal = dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25,
                 loss_weight=1.0)
    with pytest.raises(NotImplementedError, match='gamma 1.5'):
        small_head(loss_cls=dict(focal, gamma=1.5))
    with pytest.raises(NotImplementedError, match='loss_cls CrossEntropyLoss'):
        small_head(loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True,
                                 loss_weight=1.0))
    # a loss_bbox outside the five box losses: refused before any device work
    head = small_head(loss_bbox=dict(type='L1Loss', loss_weight=1.0))
    hi = S.fcos_head_inputs(1)
    batch = S.plain_batch('multi')
    with pytest.raises(NotImplementedError, match='one of the box losses'):
        head.loss(hi['cls'], S.fcos_activate(hi['raw']), hi['ctr'],
                  batch['gt_bboxes'], batch['gt_labels'], batch['img_metas'])
    hi, metas = S.fcos_infer_inputs()
    head = small_head()
    with pytest.raises(NotImplementedError, match='min_bbox_size'):
        head.get_bboxes(hi['cls'], hi['reg'], hi['ctr'], metas,
                        cfg=Config(dict(head.test_cfg, min_bbox_size=2)))
    # every one of the five box losses is taken
    for t in ('IoULoss', 'GIoULoss', 'DIoULoss', 'CIoULoss'):
        small_head(loss_bbox=dict(type=t, loss_weight=1.0))._check_loss_cfg()
    # the distribution head still refuses norm_on_bbox
    with pytest.raises(NotImplementedError, match='norm_on_bbox'):
        registry.build_head(dict(type='FCOSGFLHead', num_classes=4,
                                 in_channels=32, norm_on_bbox=True))


def test_flag_and_abi_constants():
    from ld_amd import lib as L
    flags = (L.LD_LOSS_PROB_CLS, L.LD_IM_CENTER_INSIDE, L.LD_LOSS_ATSS,
             L.LD_LOSS_FCOS, L.LD_LOSS_RETINA, L.LD_LOSS_DELTA,
             L.LD_LOSS_DIST, L.LD_LOSS_DIST_NORM)
    assert len(set(flags)) == len(flags)
    assert all(f & (f - 1) == 0 and f < (1 << L.LD_LOSS_BBOX_SHIFT)
               for f in flags)
    assert L.LD_INFER_DIST == 32 and L.LD_INFER_DIST not in (
        L.LD_INFER_VOTING, L.LD_INFER_PROB, L.LD_INFER_POINTS,
        L.LD_INFER_DELTA, L.LD_AUG_RESCALE)
    hp = small_head('tricks')._hp()
    assert hp.flags & L.LD_LOSS_DIST and hp.flags & L.LD_LOSS_DIST_NORM
    assert not small_head()._hp().flags & L.LD_LOSS_DIST_NORM
