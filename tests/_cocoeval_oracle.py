"""Plain numpy / Python restatement of pycocotools' COCO + COCOeval
(iouType='bbox', useCats=1) and of the glue in the reference's
CocoDataset.evaluate (mmdet/datasets/coco.py:216-231, 363-545).

pycocotools is not installed anywhere this project is built or tested, so this
file is the executable form of the contract in ld_amd/coco_eval.py: it keeps the
structure of ``evaluateImg`` / ``accumulate`` / ``summarize`` line by line,
including their quirks (maxDets=100 for stats[0], ``dtm == 0`` reading a match
to annotation id 0 as unmatched, ``ignore`` overwritten by ``iscrowd``).  The
CPU tests check it against hand-derived known answers before the GPU tests
trust it.
"""
import copy
import itertools
from collections import OrderedDict, defaultdict

import numpy as np


class COCO:
    """The parts of pycocotools.coco.COCO that COCOeval and coco.py use."""

    def __init__(self, dataset=None):
        self.dataset = dataset if dataset is not None else {}
        self.anns, self.cats, self.imgs = {}, {}, {}
        self.imgToAnns = defaultdict(list)
        self.catToImgs = defaultdict(list)
        for ann in self.dataset.get('annotations', []):
            self.imgToAnns[ann['image_id']].append(ann)
            self.anns[ann['id']] = ann
        for img in self.dataset.get('images', []):
            self.imgs[img['id']] = img
        for cat in self.dataset.get('categories', []):
            self.cats[cat['id']] = cat
        for ann in self.dataset.get('annotations', []):
            self.catToImgs[ann['category_id']].append(ann['image_id'])

    def getImgIds(self):
        return list(self.imgs.keys())

    def getCatIds(self, catNms=()):
        cats = self.dataset.get('categories', [])
        if len(catNms):
            cats = [c for c in cats if c['name'] in catNms]
        return [c['id'] for c in cats]

    def loadCats(self, ids):
        return [self.cats[i] for i in (ids if isinstance(ids, list) else [ids])]

    def annsFor(self, imgIds, catIds):
        lists = [self.imgToAnns[i] for i in imgIds if i in self.imgToAnns]
        return [a for a in itertools.chain.from_iterable(lists)
                if a['category_id'] in catIds]

    def loadRes(self, anns):
        res = COCO()
        res.dataset['images'] = [img for img in self.dataset['images']]
        anns = copy.deepcopy(anns)
        assert 'bbox' in anns[0]  # IndexError on an empty list, as upstream
        annsImgIds = [ann['image_id'] for ann in anns]
        assert set(annsImgIds) == (set(annsImgIds) & set(self.getImgIds()))
        res.dataset['categories'] = copy.deepcopy(self.dataset['categories'])
        for id, ann in enumerate(anns):
            bb = ann['bbox']
            ann['area'] = bb[2] * bb[3]
            ann['id'] = id + 1
            ann['iscrowd'] = 0
        res.dataset['annotations'] = anns
        res.__init__(res.dataset)
        return res


def bb_iou(dt, gt, iscrowd):
    """maskApi bbIou, float64, (D, G)."""
    o = np.zeros((len(dt), len(gt)))
    for g, G in enumerate(gt):
        ga = G[2] * G[3]
        crowd = bool(iscrowd[g])
        for d, D in enumerate(dt):
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if crowd else da + ga - i
            o[d, g] = i / u
    return o


class Params:

    def __init__(self):
        self.imgIds, self.catIds = [], []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05))
                                   + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01))
                                   + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2],
                        [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ['all', 'small', 'medium', 'large']
        self.useCats = 1


class COCOeval:

    def __init__(self, cocoGt, cocoDt, iouType='bbox'):
        assert iouType == 'bbox'
        self.cocoGt, self.cocoDt = cocoGt, cocoDt
        self.params = Params()
        self.params.imgIds = sorted(cocoGt.getImgIds())
        self.params.catIds = sorted(cocoGt.getCatIds())
        self.eval = {}

    def _prepare(self):
        p = self.params
        gts = self.cocoGt.annsFor(p.imgIds, p.catIds)
        dts = self.cocoDt.annsFor(p.imgIds, p.catIds)
        for gt in gts:
            gt['ignore'] = gt['ignore'] if 'ignore' in gt else 0
            gt['ignore'] = 'iscrowd' in gt and gt['iscrowd']
        self._gts, self._dts = defaultdict(list), defaultdict(list)
        for gt in gts:
            self._gts[gt['image_id'], gt['category_id']].append(gt)
        for dt in dts:
            self._dts[dt['image_id'], dt['category_id']].append(dt)

    def evaluate(self):
        p = self.params
        p.imgIds = list(np.unique(p.imgIds))
        p.catIds = list(np.unique(p.catIds))
        p.maxDets = sorted(p.maxDets)
        self._prepare()
        self.ious = {(imgId, catId): self.computeIoU(imgId, catId)
                     for imgId in p.imgIds for catId in p.catIds}
        maxDet = p.maxDets[-1]
        self.evalImgs = [self.evaluateImg(imgId, catId, areaRng, maxDet)
                         for catId in p.catIds for areaRng in p.areaRng
                         for imgId in p.imgIds]
        self._paramsEval = copy.deepcopy(self.params)

    def computeIoU(self, imgId, catId):
        p = self.params
        gt, dt = self._gts[imgId, catId], self._dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return []
        inds = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[i] for i in inds]
        if len(dt) > p.maxDets[-1]:
            dt = dt[0:p.maxDets[-1]]
        if len(gt) == 0 or len(dt) == 0:
            return []
        return bb_iou([d['bbox'] for d in dt], [g['bbox'] for g in gt],
                      [int(o['iscrowd']) for o in gt])

    def evaluateImg(self, imgId, catId, aRng, maxDet):
        p = self.params
        gt, dt = self._gts[imgId, catId], self._dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return None
        for g in gt:
            if g['ignore'] or (g['area'] < aRng[0] or g['area'] > aRng[1]):
                g['_ignore'] = 1
            else:
                g['_ignore'] = 0
        gtind = np.argsort([g['_ignore'] for g in gt], kind='mergesort')
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[i] for i in dtind[0:maxDet]]
        iscrowd = [int(o['iscrowd']) for o in gt]
        ious = self.ious[imgId, catId][:, gtind] \
            if len(self.ious[imgId, catId]) > 0 else self.ious[imgId, catId]
        T, G, D = len(p.iouThrs), len(gt), len(dt)
        gtm, dtm = np.zeros((T, G)), np.zeros((T, D))
        gtIg = np.array([g['_ignore'] for g in gt])
        dtIg = np.zeros((T, D))
        if not len(ious) == 0:
            for tind, t in enumerate(p.iouThrs):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gt):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dtIg[tind, dind] = gtIg[m]
                    dtm[tind, dind] = gt[m]['id']
                    gtm[tind, m] = d['id']
        a = np.array([d['area'] < aRng[0] or d['area'] > aRng[1]
                      for d in dt]).reshape((1, len(dt)))
        dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {'image_id': imgId, 'category_id': catId, 'aRng': aRng,
                'maxDet': maxDet, 'dtIds': [d['id'] for d in dt],
                'gtIds': [g['id'] for g in gt], 'dtMatches': dtm,
                'gtMatches': gtm, 'dtScores': [d['score'] for d in dt],
                'gtIgnore': gtIg, 'dtIgnore': dtIg}

    def accumulate(self):
        p = self.params
        T, R, K = len(p.iouThrs), len(p.recThrs), len(p.catIds)
        A, M = len(p.areaRng), len(p.maxDets)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        scores = -np.ones((T, R, K, A, M))
        _pe = self._paramsEval
        setK, setM = set(_pe.catIds), set(_pe.maxDets)
        setA, setI = set(map(tuple, _pe.areaRng)), set(_pe.imgIds)
        k_list = [n for n, k in enumerate(p.catIds) if k in setK]
        m_list = [m for n, m in enumerate(p.maxDets) if m in setM]
        a_list = [n for n, a in enumerate(map(lambda x: tuple(x), p.areaRng))
                  if a in setA]
        i_list = [n for n, i in enumerate(p.imgIds) if i in setI]
        I0, A0 = len(_pe.imgIds), len(_pe.areaRng)
        for k, k0 in enumerate(k_list):
            Nk = k0 * A0 * I0
            for a, a0 in enumerate(a_list):
                Na = a0 * I0
                for m, maxDet in enumerate(m_list):
                    E = [self.evalImgs[Nk + Na + i] for i in i_list]
                    E = [e for e in E if e is not None]
                    if len(E) == 0:
                        continue
                    dtScores = np.concatenate([e['dtScores'][0:maxDet]
                                               for e in E])
                    inds = np.argsort(-dtScores, kind='mergesort')
                    dtScoresSorted = dtScores[inds]
                    dtm = np.concatenate([e['dtMatches'][:, 0:maxDet]
                                          for e in E], axis=1)[:, inds]
                    dtIg = np.concatenate([e['dtIgnore'][:, 0:maxDet]
                                           for e in E], axis=1)[:, inds]
                    gtIg = np.concatenate([e['gtIgnore'] for e in E])
                    npig = np.count_nonzero(gtIg == 0)
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dtIg))
                    fps = np.logical_and(np.logical_not(dtm),
                                         np.logical_not(dtIg))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                    fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                        tp, fp = np.array(tp), np.array(fp)
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        q, ss = np.zeros((R, )), np.zeros((R, ))
                        recall[t, k, a, m] = rc[-1] if nd else 0
                        pr, q = pr.tolist(), q.tolist()
                        for i in range(nd - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        inds = np.searchsorted(rc, p.recThrs, side='left')
                        try:
                            for ri, pi in enumerate(inds):
                                q[ri] = pr[pi]
                                ss[ri] = dtScoresSorted[pi]
                        except IndexError:
                            pass
                        precision[t, :, k, a, m] = np.array(q)
                        scores[t, :, k, a, m] = np.array(ss)
        self.eval = {'counts': [T, R, K, A, M], 'precision': precision,
                     'recall': recall, 'scores': scores}

    def summarize(self):
        def _summarize(ap=1, iouThr=None, areaRng='all', maxDets=100):
            p = self.params
            aind = [i for i, aRng in enumerate(p.areaRngLbl) if aRng == areaRng]
            mind = [i for i, mDet in enumerate(p.maxDets) if mDet == maxDets]
            if ap == 1:
                s = self.eval['precision']
                if iouThr is not None:
                    t = np.where(iouThr == p.iouThrs)[0]
                    s = s[t]
                s = s[:, :, :, aind, mind]
            else:
                s = self.eval['recall']
                if iouThr is not None:
                    t = np.where(iouThr == p.iouThrs)[0]
                    s = s[t]
                s = s[:, :, aind, mind]
            if len(s[s > -1]) == 0:
                mean_s = -1
            else:
                mean_s = np.mean(s[s > -1])
            return mean_s

        m = self.params.maxDets
        stats = np.zeros((12, ))
        stats[0] = _summarize(1)
        stats[1] = _summarize(1, iouThr=.5, maxDets=m[2])
        stats[2] = _summarize(1, iouThr=.75, maxDets=m[2])
        stats[3] = _summarize(1, areaRng='small', maxDets=m[2])
        stats[4] = _summarize(1, areaRng='medium', maxDets=m[2])
        stats[5] = _summarize(1, areaRng='large', maxDets=m[2])
        stats[6] = _summarize(0, maxDets=m[0])
        stats[7] = _summarize(0, maxDets=m[1])
        stats[8] = _summarize(0, maxDets=m[2])
        stats[9] = _summarize(0, areaRng='small', maxDets=m[2])
        stats[10] = _summarize(0, areaRng='medium', maxDets=m[2])
        stats[11] = _summarize(0, areaRng='large', maxDets=m[2])
        self.stats = stats


# ------------------------------------------------------------ coco.py glue ---
def det2json(results, img_ids, cat_ids):
    """CocoDataset._det2json (coco.py:216-231) + xyxy2xywh."""
    out = []
    for idx in range(len(img_ids)):
        for label in range(len(results[idx])):
            bboxes = results[idx][label]
            for i in range(bboxes.shape[0]):
                b = bboxes[i].tolist()
                out.append(dict(image_id=img_ids[idx],
                                bbox=[b[0], b[1], b[2] - b[0], b[3] - b[1]],
                                score=float(bboxes[i][4]),
                                category_id=cat_ids[label]))
    return out


COCO_METRIC_NAMES = {
    'mAP': 0, 'mAP_50': 1, 'mAP_75': 2, 'mAP_s': 3, 'mAP_m': 4, 'mAP_l': 5,
    'AR@100': 6, 'AR@300': 7, 'AR@1000': 8, 'AR_s@1000': 9, 'AR_m@1000': 10,
    'AR_l@1000': 11
}


def evaluate(dataset, results, classes=None, classwise=False,
             proposal_nums=(100, 300, 1000), iou_thrs=None, metric_items=None):
    """CocoDataset(ann_file, classes).evaluate(results, metric='bbox', ...)
    restated -> (eval_results, cocoEval or None, classwise rows)."""
    coco = COCO(copy.deepcopy(dataset))
    cat_ids = coco.getCatIds(catNms=classes or ())
    img_ids = coco.getImgIds()
    if iou_thrs is None:
        iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1,
                               endpoint=True)
    # a list would make summarize's `iouThr == p.iouThrs` one plain bool
    # (numpy-version dependent); the evaluator takes an array, and so does this
    iou_thrs = np.asarray(iou_thrs, dtype=np.float64)
    if metric_items is not None and not isinstance(metric_items, list):
        metric_items = [metric_items]
    eval_results = OrderedDict()
    try:
        cocoDt = coco.loadRes(det2json(results, img_ids, cat_ids))
    except IndexError:
        return eval_results, None, None
    cocoEval = COCOeval(coco, cocoDt, 'bbox')
    cocoEval.params.catIds = cat_ids
    cocoEval.params.imgIds = img_ids
    cocoEval.params.maxDets = list(proposal_nums)
    cocoEval.params.iouThrs = iou_thrs
    if metric_items is not None:
        for item in metric_items:
            if item not in COCO_METRIC_NAMES:
                raise KeyError(f'metric item {item} is not supported')
    cocoEval.evaluate()
    cocoEval.accumulate()
    cocoEval.summarize()
    rows = None
    if classwise:
        precisions = cocoEval.eval['precision']
        rows = []
        for idx, catId in enumerate(cat_ids):
            nm = coco.loadCats(catId)[0]
            precision = precisions[:, :, idx, 0, -1]
            precision = precision[precision > -1]
            ap = np.mean(precision) if precision.size else float('nan')
            rows.append((f'{nm["name"]}', f'{float(ap):0.3f}'))
    if metric_items is None:
        metric_items = ['mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l']
    for item in metric_items:
        eval_results[f'bbox_{item}'] = float(
            f'{cocoEval.stats[COCO_METRIC_NAMES[item]]:.3f}')
    ap = cocoEval.stats[:6]
    eval_results['bbox_mAP_copypaste'] = (
        f'{ap[0]:.3f} {ap[1]:.3f} {ap[2]:.3f} {ap[3]:.3f} '
        f'{ap[4]:.3f} {ap[5]:.3f}')
    return eval_results, cocoEval, rows


def match_bits(cocoEval, dets_json_len):
    """Per detection of the det2json list (1-based id - 1): the uint64
    matched (dtm != 0) / ignored masks, bit t * A + a, and whether it was kept
    (rank < maxDets[-1]) -> (match, ign, kept)."""
    p = cocoEval.params
    T, A = len(p.iouThrs), len(p.areaRng)
    match = np.zeros(dets_json_len, np.uint64)
    ign = np.zeros(dets_json_len, np.uint64)
    kept = np.zeros(dets_json_len, bool)
    I0 = len(p.imgIds)
    for e_idx, e in enumerate(cocoEval.evalImgs):
        if e is None:
            continue
        a = (e_idx // I0) % A
        for j, did in enumerate(e['dtIds']):
            kept[did - 1] = True
            for t in range(T):
                bit = np.uint64(1) << np.uint64(t * A + a)
                if e['dtMatches'][t, j] != 0:
                    match[did - 1] |= bit
                if e['dtIgnore'][t, j]:
                    ign[did - 1] |= bit
    return match, ign, kept


def npig(cocoEval):
    """Non-ignored GTs per (category, area): (K, A)."""
    p = cocoEval.params
    K, A, I0 = len(p.catIds), len(p.areaRng), len(p.imgIds)
    out = np.zeros((K, A), np.int64)
    for e_idx, e in enumerate(cocoEval.evalImgs):
        if e is None:
            continue
        k, a = e_idx // (A * I0), (e_idx // I0) % A
        out[k, a] += np.count_nonzero(e['gtIgnore'] == 0)
    return out
