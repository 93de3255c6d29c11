"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/augtest.npz by EXECUTING THE
REFERENCE's test-time augmentation on CPU in fp32 (the reference package is
imported, unmodified, through oracle/ref_shim.py).  Run from the repo root in
the build container, never on the GPU machine:

    python tools/gen_golden_augtest.py

Reference entry points exercised (file:line under the reference tree):
  mmdet/models/dense_heads/dense_test_mixins.py:38-100  aug_test_bboxes
      (-> get_bboxes(with_nms=False) per view, merge_aug_bboxes,
       multiclass_nms with score_factors, bbox2result)
  mmdet/core/bbox/transforms.py:5-55                    bbox_flip / bbox_mapping_back
  mmdet/datasets/pipelines/test_time_aug.py:83-112      MultiScaleFlipAug view order

The head's ``forward`` is replaced by a lookup of seeded per-view maps
(ld_amd.synthetic.aug_view_outs), so only the seeds and the reference outputs
are stored.
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

from ld_amd import synthetic  # noqa: E402

HEADS = {'gfl': G._ld_head, 'gfl_clustered': G._ld_head, 'v2': G._ldv2_head,
         'atss': G._ld_atss_head, 'fcos': G._ld_fcos_head,
         'retina': G._ld_retina_head}


def _np(t):
    return t.detach().cpu().numpy()


def gen_cases(d):
    import mmcv
    from mmdet.models.dense_heads import dense_test_mixins as DTM
    captured = {}
    orig_b2r = DTM.bbox2result

    def b2r(bboxes, labels, num_classes):
        captured['dets'], captured['labels'] = bboxes, labels
        return orig_b2r(bboxes, labels, num_classes)

    DTM.bbox2result = b2r
    for case in synthetic.AUG_CASES:
        name, kind, views, seed, nms_pre, cs, sh, nms_type, store = case
        head = HEADS[kind]()
        head.eval()
        head.test_cfg = mmcv.ConfigDict(dict(
            nms_pre=nms_pre, min_bbox_size=0, score_thr=0.05,
            nms=dict(type=nms_type, iou_threshold=0.6), max_per_img=100))
        head.forward = lambda v, _c=case: synthetic.aug_view_outs(_c, v)
        orig_merge = head.merge_aug_bboxes

        def merge(aug_bboxes, aug_scores, img_metas, _o=orig_merge):
            captured['pre'] = [b.clone() for b in aug_bboxes]
            captured['pre_scores'] = [s.clone() for s in aug_scores]
            out = _o(aug_bboxes, aug_scores, img_metas)
            captured['merged'] = out[0].clone()
            return out

        head.merge_aug_bboxes = merge
        metas = synthetic.aug_view_metas(case)
        for rescale in (False, True):
            with torch.no_grad():
                res = head.aug_test_bboxes(list(range(len(views))), metas,
                                           rescale=rescale)
            tag = f'{name}_r{int(rescale)}'
            d[f'{tag}_bboxes'] = _np(captured['dets']).astype(np.float32)
            d[f'{tag}_labels'] = _np(captured['labels']).astype(np.int64)
            d[f'{tag}_per_class'] = np.array([len(a) for a in res])
        scores = torch.cat([s[:, :-1] for s in captured['pre_scores']])
        d[f'{name}_candidates'] = np.array(int((scores > 0.05).sum()))
        d[f'{name}_pre_counts'] = np.array([b.shape[0]
                                            for b in captured['pre']])
        if store:
            for v, b in enumerate(captured['pre']):
                d[f'{name}_pre_bboxes_{v}'] = _np(b).astype(np.float32)
            d[f'{name}_merged_bboxes'] = _np(captured['merged']).astype(
                np.float32)
        print(f'[augtest] {name}: views {len(views)}, merged rows '
              f'{int(sum(d[f"{name}_pre_counts"]))}, candidates '
              f'{int(d[f"{name}_candidates"])}, dets '
              f'{d[f"{name}_r0_labels"].shape[0]}', flush=True)
    DTM.bbox2result = orig_b2r


def gen_view_order(d):
    """MultiScaleFlipAug with a pass-through inner transform: the (scale,
    flip, flip_direction) of every view it emits."""
    from mmdet.datasets.pipelines.test_time_aug import MultiScaleFlipAug
    scales = [(1333, 800), (666, 400)]
    aug = MultiScaleFlipAug(transforms=[], img_scale=scales, flip=True)
    out = aug(dict(filename='x'))
    d['order_img_scale'] = np.array(scales, dtype=np.int64)
    d['order_scale'] = np.array(out['scale'], dtype=np.int64)
    d['order_flip'] = np.array(out['flip'], dtype=bool)
    d['order_flip_direction'] = np.array(
        [str(x) for x in out['flip_direction']])
    print('[augtest] MultiScaleFlipAug order:',
          list(zip(out['scale'], out['flip'], out['flip_direction'])))


def main():
    d = {}
    gen_view_order(d)
    gen_cases(d)
    np.savez_compressed(os.path.join(REPO, 'tests', 'golden', 'augtest.npz'),
                        **d)


if __name__ == '__main__':
    main()
