"""Plain numpy / Python restatement of the ``useCats = 0`` path of pycocotools'
COCOeval and of the glue in the reference's CocoDataset.evaluate for
``metric='proposal'`` / ``'proposal_fast'`` (mmdet/datasets/coco.py:233-243,
311-333, 425-434, 474-488), on top of tests/_cocoeval_oracle.py.

With ``useCats = 0`` COCOeval
  * does not make ``catIds`` unique or sorted (evaluate), and loads the
    annotations of the images whatever their category (_prepare);
  * evaluates one cell per image, whose GTs / detections are those of every
    category of ``p.catIds``, category-major in that order, in annotation /
    result order inside a category (computeIoU, evaluateImg);
  * accumulates over the single category ``-1``.
The per-cell code (evaluateImg, accumulate, summarize) is the oracle's own.

One deliberate difference from the reference's glue: ``_proposal2json`` gives
every proposal category id 1, so the reference scores array results only when
1 is one of the dataset's category ids.  ``proposal2json`` below takes the
category id as an argument and ``evaluate_proposal`` passes the first of
``cat_ids``; the scores do not depend on which category of ``cat_ids`` it is.
"""
import copy
from collections import OrderedDict, defaultdict

import numpy as np

import _cocoeval_oracle as O


class COCOevalNoCats(O.COCOeval):

    def __init__(self, cocoGt, cocoDt):
        super().__init__(cocoGt, cocoDt, 'bbox')
        self.params.useCats = 0

    def _prepare(self):
        p = self.params
        every = _Everything()
        gts = self.cocoGt.annsFor(p.imgIds, every)
        dts = self.cocoDt.annsFor(p.imgIds, every)
        for gt in gts:
            gt['ignore'] = gt['ignore'] if 'ignore' in gt else 0
            gt['ignore'] = 'iscrowd' in gt and gt['iscrowd']
        by_gt, by_dt = defaultdict(list), defaultdict(list)
        for gt in gts:
            by_gt[gt['image_id'], gt['category_id']].append(gt)
        for dt in dts:
            by_dt[dt['image_id'], dt['category_id']].append(dt)
        # computeIoU / evaluateImg: [_ for cId in p.catIds for _ in ...[imgId, cId]]
        self._gts, self._dts = defaultdict(list), defaultdict(list)
        for imgId in p.imgIds:
            self._gts[imgId, -1] = [g for c in self._cat_ids
                                    for g in by_gt[imgId, c]]
            self._dts[imgId, -1] = [d for c in self._cat_ids
                                    for d in by_dt[imgId, c]]

    def evaluate(self):
        p = self.params
        p.imgIds = list(np.unique(p.imgIds))
        p.maxDets = sorted(p.maxDets)
        self._cat_ids = list(p.catIds)  # as given: not unique, not sorted
        p.catIds = [-1]
        self._prepare()
        self.ious = {(imgId, -1): self.computeIoU(imgId, -1)
                     for imgId in p.imgIds}
        maxDet = p.maxDets[-1]
        self.evalImgs = [self.evaluateImg(imgId, -1, areaRng, maxDet)
                         for areaRng in p.areaRng for imgId in p.imgIds]
        self._paramsEval = copy.deepcopy(self.params)


class _Everything:

    def __contains__(self, item):
        return True


def proposal2json(results, img_ids, cat_id):
    """CocoDataset._proposal2json (coco.py:233-243) + xyxy2xywh."""
    out = []
    for idx in range(len(img_ids)):
        bboxes = results[idx]
        for i in range(bboxes.shape[0]):
            b = bboxes[i].tolist()
            out.append(dict(image_id=img_ids[idx],
                            bbox=[b[0], b[1], b[2] - b[0], b[3] - b[1]],
                            score=float(bboxes[i][4]), category_id=cat_id))
    return out


PROPOSAL_ITEMS = ['AR@100', 'AR@300', 'AR@1000', 'AR_s@1000', 'AR_m@1000',
                  'AR_l@1000']


def evaluate_proposal(dataset, results, classes=None,
                      proposal_nums=(100, 300, 1000), iou_thrs=None,
                      metric_items=None):
    """CocoDataset(ann_file, classes).evaluate(results, metric='proposal')
    restated -> (eval_results, cocoEval or None).  ``results[i]`` a (k, 5)
    array, or a list of per-class arrays (``_det2json``)."""
    coco = O.COCO(copy.deepcopy(dataset))
    cat_ids = coco.getCatIds(catNms=classes or ())
    img_ids = coco.getImgIds()
    if iou_thrs is None:
        iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1,
                               endpoint=True)
    iou_thrs = np.asarray(iou_thrs, dtype=np.float64)
    if metric_items is not None and not isinstance(metric_items, list):
        metric_items = [metric_items]
    eval_results = OrderedDict()
    if len(results) and isinstance(results[0], list):
        anns = O.det2json(results, img_ids, cat_ids)
    else:
        anns = proposal2json(results, img_ids, cat_ids[0])
    try:
        cocoDt = coco.loadRes(anns)
    except IndexError:
        return eval_results, None
    cocoEval = COCOevalNoCats(coco, cocoDt)
    cocoEval.params.catIds = cat_ids
    cocoEval.params.imgIds = img_ids
    cocoEval.params.maxDets = list(proposal_nums)
    cocoEval.params.iouThrs = iou_thrs
    if metric_items is not None:
        for item in metric_items:
            if item not in O.COCO_METRIC_NAMES:
                raise KeyError(f'metric item {item} is not supported')
    cocoEval.evaluate()
    cocoEval.accumulate()
    cocoEval.summarize()
    if metric_items is None:
        metric_items = PROPOSAL_ITEMS
    for item in metric_items:
        eval_results[item] = float(
            f'{cocoEval.stats[O.COCO_METRIC_NAMES[item]]:.3f}')
    return eval_results, cocoEval
