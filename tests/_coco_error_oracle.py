"""Plain numpy / Python restatement of the reference's
tools/analysis_tools/coco_error_analysis.py (analyze_results and
analyze_individual_category, without the plotting), on top of the COCOeval
restatement in _cocoeval_oracle.py.  It keeps the reference's structure:
1 + 2 K COCOeval passes over deep copies, the relabel done in place on the
copied annotations (so imgToAnns order is kept), and the fill of ps row by
row, category by category."""
import copy
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cocoeval_oracle as O  # noqa: E402

TYPES = ['C75', 'C50', 'Loc', 'Sim', 'Oth', 'BG', 'FN']
AREA_NAMES = ['allarea', 'small', 'medium', 'large']


class COCO(O.COCO):
    """pycocotools' getCatIds with supNms."""

    def getCatIds(self, catNms=(), supNms=()):
        cats = self.dataset.get('categories', [])
        if len(catNms):
            cats = [c for c in cats if c['name'] in catNms]
        if len(supNms):
            cats = [c for c in cats if c['supercategory'] in supNms]
        return [c['id'] for c in cats]


def analyze_individual_category(k, cocoDt, cocoGt, catId):
    ps_ = {}
    dt = copy.deepcopy(cocoDt)
    nm = cocoGt.loadCats(catId)[0]
    imgIds = cocoGt.getImgIds()
    dt.dataset['annotations'] = [a for a in dt.dataset['annotations']
                                 if a['category_id'] == catId]
    dt.__init__(dt.dataset)  # createIndex
    gt = copy.deepcopy(cocoGt)
    child_catIds = gt.getCatIds(supNms=[nm['supercategory']])
    for idx, ann in enumerate(gt.dataset['annotations']):
        if ann['category_id'] in child_catIds and ann['category_id'] != catId:
            gt.dataset['annotations'][idx]['ignore'] = 1
            gt.dataset['annotations'][idx]['iscrowd'] = 1
            gt.dataset['annotations'][idx]['category_id'] = catId
    ps_['ps_supercategory'] = _pass(gt, dt, imgIds, k)
    gt = copy.deepcopy(cocoGt)
    for idx, ann in enumerate(gt.dataset['annotations']):
        if ann['category_id'] != catId:
            gt.dataset['annotations'][idx]['ignore'] = 1
            gt.dataset['annotations'][idx]['iscrowd'] = 1
            gt.dataset['annotations'][idx]['category_id'] = catId
    ps_['ps_allcategory'] = _pass(gt, dt, imgIds, k)
    return k, ps_


def _pass(gt, dt, imgIds, k):
    cocoEval = O.COCOeval(gt, copy.deepcopy(dt), 'bbox')
    cocoEval.params.imgIds = imgIds
    cocoEval.params.maxDets = [100]
    cocoEval.params.iouThrs = [.1]
    cocoEval.params.useCats = 1
    cocoEval.evaluate()
    cocoEval.accumulate()
    return cocoEval.eval['precision'][0, :, k, :, :]


def analyze_results(dataset, res_anns):
    """-> (ps (7, R, K, 4, 1) after the fill, raw (5, R, K, 4, 1) before it,
    recThrs).  ``dataset`` a COCO annotation dict, ``res_anns`` a results
    list (loadRes)."""
    cocoGt = COCO(copy.deepcopy(dataset))
    cocoDt = cocoGt.loadRes(res_anns)
    imgIds = cocoGt.getImgIds()
    cocoEval = O.COCOeval(copy.deepcopy(cocoGt), copy.deepcopy(cocoDt), 'bbox')
    cocoEval.params.imgIds = imgIds
    cocoEval.params.iouThrs = [.75, .5, .1]
    cocoEval.params.maxDets = [100]
    cocoEval.evaluate()
    cocoEval.accumulate()
    ps = cocoEval.eval['precision']
    ps = np.vstack([ps, np.zeros((4, *ps.shape[1:]))])
    raw = ps[:5].copy()
    catIds = cocoGt.getCatIds()
    recThrs = cocoEval.params.recThrs
    results = [analyze_individual_category(k, cocoDt, cocoGt, catId)
               for k, catId in enumerate(catIds)]
    for k, catId in enumerate(catIds):
        assert results[k][0] == k
        raw[3, :, k] = results[k][1]['ps_supercategory']
        raw[4, :, k] = results[k][1]['ps_allcategory']
        ps[3, :, k, :, :] = results[k][1]['ps_supercategory']
        ps[4, :, k, :, :] = results[k][1]['ps_allcategory']
        ps[ps == -1] = 0
        ps[5, :, k, :, :] = (ps[4, :, k, :, :] > 0)
        ps[6, :, k, :, :] = 1.0
    return ps, raw, recThrs


def area_aps(ps):
    """makeplot's ``aps`` per area: {area: {type: mean}}."""
    out = {}
    for i in range(len(AREA_NAMES)):
        area_ps = ps[..., i, 0]
        aps = [ps_.mean() for ps_ in area_ps]
        out[AREA_NAMES[i]] = dict(zip(TYPES, [float(a) for a in aps]))
    return out


def aps_table(ps, class_names):
    table = {nm: area_aps(ps[:, :, k]) for k, nm in enumerate(class_names)}
    table['allclass'] = area_aps(ps)
    return table
