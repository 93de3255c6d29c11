"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/plain_heads.npz by EXECUTING THE
REFERENCE's DeltaXYWHBBoxCoder, ATSSHead and RetinaHead on CPU (the reference
package is imported, unmodified, through oracle/ref_shim.py).  Run from the repo
root in the build container, never on the GPU machine:

    python tools/gen_golden_plain_heads.py

Reference entry points exercised (file:line under the reference tree):
  mmdet/core/bbox/coder/delta_xywh_bbox_coder.py:35-237  encode / decode
  mmdet/models/dense_heads/atss_head.py:145-296,376-508  loss / _get_bboxes
  mmdet/models/dense_heads/anchor_head.py:376-495,591-727 loss / _get_bboxes
  mmdet/models/dense_heads/retina_head.py:8-114
  mmdet/models/losses/focal_loss.py:12-47   py_sigmoid_focal_loss -- the shim's
      mmcv.ops.sigmoid_focal_loss is a dummy, so the module-level
      ``_sigmoid_focal_loss`` of focal_loss.py is replaced AT RUN TIME by a
      wrapper that one-hot encodes the labels and calls the reference's own
      py_sigmoid_focal_loss(..., reduction='none')

Only seeds, the hand-written boxes (ld_amd.synthetic: PLAIN_CASES, DELTA_HAND)
and reference outputs are stored; every input is regenerated from
ld_amd.synthetic.

CODER -- the DELTA_ROWS rows of synthetic.delta_coder_rows(), per coder C in
atss (stds 0.1 / 0.2), retina (stds 1):
  coder_C_enc (257, 4)       encode(anchors, gts)
  coder_C_dec (257, 4)       decode(anchors, deltas)
  coder_C_dec_clip (257, 4)  decode(anchors, deltas, max_shape=DELTA_MAX_SHAPE)

LOSS -- per head H / variant and PLAIN_CASES case:
  H_case_losses (K, 5) float64: rows loss_cls, loss_bbox[, loss_centerness]
  H_case_g{cls,reg,ctr}_{l}: gradient of the sum of all entries
  H_case_pos (5,): positives per level; H_case_ignored: anchors with
  label_weight 0 (RetinaNet's band between the thresholds)
H: atss (GIoULoss 2.0), retina_l1 (L1Loss, the config), retina_sl1
(SmoothL1Loss(beta=1/9)), retina_giou (reg_decoded_bbox=True, GIoULoss 2.0);
the two side variants run on 'multi' only.

INFER -- H in atss, retina on synthetic.plain_infer_inputs: per rescale r in
0, 1 ``H_r{r}_bboxes_{i}`` / ``_labels_{i}`` (get_bboxes) and, rescale=False,
``H_pre_bboxes_{i}`` / ``_scores_{i}`` [/ ``_factors_{i}``]
(get_bboxes(with_nms=False)).

KEYS -- ``keys_atss`` / ``keys_retina``: state_dict key lists of the heads as
configs/atss/atss_r50_fpn_1x_coco.py and
configs/retinanet/retinanet_r50_fpn_1x_coco.py build them.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'oracle'))
sys.path.insert(0, REPO)

import gen_golden as G  # noqa: E402  (installs ref_shim)
import ref_shim  # noqa: E402

from ld_amd import synthetic as S  # noqa: E402

import mmdet.models.losses.focal_loss as FL  # noqa: E402


def _focal(pred, target, gamma, alpha, weight, reduction):
    onehot = torch.nn.functional.one_hot(
        target, num_classes=pred.shape[1] + 1)[:, :pred.shape[1]]
    return FL.py_sigmoid_focal_loss(pred, onehot, None, gamma, alpha, 'none')


FL._sigmoid_focal_loss = _focal

_np = G._np
ATSS_KEYS = ['loss_cls', 'loss_bbox', 'loss_centerness']
RETINA_KEYS = ['loss_cls', 'loss_bbox']


def _train_cfg(kind):
    if kind == 'atss':
        return ref_shim.ConfigDict(assigner=dict(type='ATSSAssigner', topk=9),
                                   allowed_border=-1, pos_weight=-1,
                                   debug=False)
    return ref_shim.ConfigDict(
        assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.5, neg_iou_thr=0.4,
                      min_pos_iou=0, ignore_iof_thr=-1),
        allowed_border=-1, pos_weight=-1, debug=False)


def _test_cfg(kind, nms_pre=1000):
    return ref_shim.ConfigDict(
        nms_pre=nms_pre, min_bbox_size=0, score_thr=0.05,
        nms=dict(type='nms', iou_threshold=0.6 if kind == 'atss' else 0.5),
        max_per_img=100)


def ref_head(kind, num_classes=S.PLAIN_CLASSES, channels=S.PLAIN_FEAT,
             **over):
    from mmdet.models import build_head
    means, stds = S.PLAIN_CODERS[kind]
    coder = dict(type='DeltaXYWHBBoxCoder', target_means=list(means),
                 target_stds=list(stds))
    focal = dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25,
                 loss_weight=1.0)
    if kind == 'atss':
        cfg = dict(
            type='ATSSHead', num_classes=num_classes, in_channels=channels,
            stacked_convs=4, feat_channels=channels,
            anchor_generator=dict(type='AnchorGenerator', ratios=[1.0],
                                  octave_base_scale=8, scales_per_octave=1,
                                  strides=[8, 16, 32, 64, 128]),
            bbox_coder=coder, loss_cls=focal,
            loss_bbox=dict(type='GIoULoss', loss_weight=2.0),
            loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True,
                                 loss_weight=1.0))
        if channels % 32:
            cfg['norm_cfg'] = dict(type='GN', num_groups=channels,
                                   requires_grad=True)
    else:
        cfg = dict(
            type='RetinaHead', num_classes=num_classes, in_channels=channels,
            stacked_convs=4, feat_channels=channels,
            anchor_generator=dict(type='AnchorGenerator', octave_base_scale=4,
                                  scales_per_octave=3, ratios=[0.5, 1.0, 2.0],
                                  strides=[8, 16, 32, 64, 128]),
            bbox_coder=coder, loss_cls=focal,
            loss_bbox=dict(type='L1Loss', loss_weight=1.0))
    cfg.update(over)
    cfg.update(train_cfg=_train_cfg(kind), test_cfg=_test_cfg(kind))
    return build_head(cfg)


def gen_coder(d):
    from mmdet.core.bbox.coder import DeltaXYWHBBoxCoder
    anchors, gts, deltas = S.delta_coder_rows()
    for name, (means, stds) in S.PLAIN_CODERS.items():
        coder = DeltaXYWHBBoxCoder(target_means=means, target_stds=stds)
        d[f'coder_{name}_enc'] = _np(coder.encode(anchors, gts))
        d[f'coder_{name}_dec'] = _np(coder.decode(anchors, deltas))
        d[f'coder_{name}_dec_clip'] = _np(
            coder.decode(anchors, deltas, max_shape=S.DELTA_MAX_SHAPE))
        assert np.isfinite(d[f'coder_{name}_enc']).all()
        assert np.isfinite(d[f'coder_{name}_dec_clip']).all()
        # the clamp and the clip are exercised
        mr = abs(np.log(16 / 1000))
        dw = deltas[:, 2].numpy() * stds[2]
        assert (dw > mr).any() and (dw < -mr).any()
        assert (d[f'coder_{name}_dec'] != d[f'coder_{name}_dec_clip']).any()


def _target_stats(head, kind, hi, batch):
    """Positives per level and the number of ignored anchors, from the
    reference's own get_targets."""
    sizes = [t.shape[-2:] for t in hi['cls']]
    anchor_list, valid = head.get_anchors(sizes, batch['img_metas'],
                                          device='cpu')
    res = head.get_targets(anchor_list, valid, batch['gt_bboxes'],
                           batch['img_metas'],
                           gt_labels_list=batch['gt_labels'],
                           label_channels=head.cls_out_channels)
    labels, weights = (res[1], res[2]) if kind == 'atss' else (res[0], res[1])
    C = head.num_classes
    pos = np.array([int(((l >= 0) & (l < C)).sum()) for l in labels])
    ignored = sum(int((w == 0).sum()) for w in weights)
    return pos, ignored, labels


def _loss_case(d, tag, kind, head, case):
    keys = ATSS_KEYS if kind == 'atss' else RETINA_KEYS
    batch = S.plain_batch(case)
    hi = S.plain_head_inputs(kind, S.PLAIN_SEEDS[case])
    pos, ignored, labels = _target_stats(head, kind, hi, batch)
    if case == 'multi':
        # the positive whose dw was put beyond the clamp IS a positive
        n, l, y, x, b, _ = S.PLAIN_CLAMP[kind]
        B = 1 if kind == 'atss' else 9
        W = hi['cls'][l].shape[-1]
        lab = labels[l][n, (y * W + x) * B + b]
        assert 0 <= int(lab) < head.num_classes, (tag, int(lab))
    group = ('cls', 'reg', 'ctr') if kind == 'atss' else ('cls', 'reg')
    for k in group:
        for t in hi[k]:
            t.requires_grad_(True)
    outs = [hi[k] for k in group]
    losses = head.loss(*outs, batch['gt_bboxes'], batch['gt_labels'],
                       batch['img_metas'])
    table = np.stack([np.array([float(v.detach()) for v in losses[k]])
                      for k in keys])
    assert np.isfinite(table).all(), (tag, case)
    sum(sum(v) for v in losses.values()).backward()
    key = f'{tag}_{case}'
    d[key + '_losses'] = table.astype(np.float64)
    d[key + '_pos'] = pos
    d[key + '_ignored'] = np.array(ignored)
    for k in group:
        for l, t in enumerate(hi[k]):
            g = t.grad if t.grad is not None else torch.zeros_like(t)
            d[f'{key}_g{k}_{l}'] = _np(g)
    print(f'  {key}: pos/level {pos.tolist()} ignored {ignored} '
          f'losses {table.sum(1)}')
    return pos, ignored


def gen_losses(d):
    atss = ref_head('atss')
    variants = [
        ('retina_l1', {}),
        ('retina_sl1', dict(loss_bbox=dict(type='SmoothL1Loss',
                                           beta=1.0 / 9.0, loss_weight=1.0))),
        ('retina_giou', dict(reg_decoded_bbox=True,
                             loss_bbox=dict(type='GIoULoss',
                                            loss_weight=2.0)))]
    for case in S.PLAIN_CASES:
        pos, _ = _loss_case(d, 'atss', 'atss', atss, case)
        if case == 'multi':
            assert (pos > 0).sum() >= 3, pos
        if case == 'no_pos':
            assert pos.sum() == 0
        for tag, over in variants:
            if tag != 'retina_l1' and case != 'multi':
                continue
            pos, ignored = _loss_case(d, tag, 'retina',
                                      ref_head('retina', **over), case)
            if case == 'multi':
                assert (pos > 0).sum() >= 2 and ignored >= 1, (pos, ignored)
            if case == 'no_pos':
                assert pos.sum() == 0


def gen_infer(d):
    for kind in ('atss', 'retina'):
        head = ref_head(kind)
        hi, metas = S.plain_infer_inputs(kind)
        cfg = _test_cfg(kind, S.PLAIN_INFER['nms_pre'])
        outs = [hi['cls'], hi['reg']] + ([hi['ctr']] if kind == 'atss' else [])
        with torch.no_grad():
            for r in (0, 1):
                res = head.get_bboxes(*outs, metas, cfg=cfg, rescale=bool(r))
                for i, (db, dl) in enumerate(res):
                    d[f'{kind}_r{r}_bboxes_{i}'] = _np(db).astype(np.float32)
                    d[f'{kind}_r{r}_labels_{i}'] = _np(dl).astype(np.int64)
            res = head.get_bboxes(*outs, metas, cfg=cfg, rescale=False,
                                  with_nms=False)
            for i, r_ in enumerate(res):
                d[f'{kind}_pre_bboxes_{i}'] = _np(r_[0]).astype(np.float32)
                d[f'{kind}_pre_scores_{i}'] = _np(r_[1]).astype(np.float32)
                if len(r_) > 2:
                    d[f'{kind}_pre_factors_{i}'] = _np(r_[2]).astype(
                        np.float32)
        n = [int(d[f'{kind}_r0_labels_{i}'].shape[0]) for i in range(2)]
        print(f'  infer {kind}: dets {n}, pre rows '
              f'{d[f"{kind}_pre_bboxes_0"].shape[0]}')
        assert min(n) >= 5


def gen_keys(d):
    for kind in ('atss', 'retina'):
        head = ref_head(kind, num_classes=80, channels=256)
        d[f'keys_{kind}'] = np.array(list(head.state_dict().keys()))


def main():
    torch.manual_seed(0)
    d = {}
    gen_coder(d)
    gen_losses(d)
    gen_infer(d)
    gen_keys(d)
    out = os.path.join(G.OUT, 'plain_heads.npz')
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), 'bytes,', len(d), 'arrays')


if __name__ == '__main__':
    main()
