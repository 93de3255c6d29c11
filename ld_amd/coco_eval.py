"""COCO-style bbox evaluation on the device: pycocotools' ``COCOeval``
(iouType='bbox') as the reference's ``CocoDataset.evaluate(metric='bbox')``
drives it (datasets/coco.py:363-545), run by the coco_eval.hip kernels.

``CocoGroundTruth`` holds an annotation set (a COCO json file, or mmdet-style
annotation dicts) on the device, grouped by (image, category).
``CocoEvaluator`` takes the detections where the heads leave them -- device
``(n, 5)`` + ``(n,)`` from ``get_bboxes`` / ``aug_test`` -- batch after batch
(``ld_coco_match``: evaluateImg for every cell of the batch), keeps one record
per detection on the device, and accumulates every category at once
(``ld_coco_accumulate``).  ``summarize`` runs here in numpy over the device
``precision`` / ``recall``.  ``coco_evaluate`` is the reference's
list-of-per-class-arrays interface on top of it.

Numerics follow pycocotools: boxes [x1, y1, x2 - x1, y2 - y1] and areas in
float64 of the fp32 values, IoU (maskApi bbIou) and rc / pr in float64, every
threshold passed as a host float64.
"""
import itertools
import json
import logging
from collections import OrderedDict

import numpy as np
import torch

from . import lib as L
from .eval_common import (ADD_STEP, RecordBuffers, as_boxes, as_labels,
                          check_one_rank, eval_device, eval_logger, pack_rows)
from .lossblock import workspace

__all__ = ['CocoGroundTruth', 'CocoEvaluator', 'coco_evaluate']

_LOG = logging.getLogger(__name__)

# pycocotools Params.setDetParams / coco.py:446-452
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2],
            [96 ** 2, 1e5 ** 2]]
AREA_LBL = ['all', 'small', 'medium', 'large']
METRIC_NAMES = {
    'mAP': 0, 'mAP_50': 1, 'mAP_75': 2, 'mAP_s': 3, 'mAP_m': 4, 'mAP_l': 5,
    'AR@100': 6, 'AR@300': 7, 'AR@1000': 8, 'AR_s@1000': 9, 'AR_m@1000': 10,
    'AR_l@1000': 11
}


def default_iou_thrs():
    return np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1,
                       endpoint=True)


def default_rec_thrs():
    return np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1,
                       endpoint=True)


class CocoGroundTruth:
    """An annotation set: ``img_ids`` (dataset index order), ``cat_ids``
    (label ``i`` is category ``cat_ids[i]``), ``cat_names``, and per GT its
    image / category id, xywh box, area, iscrowd and annotation id (float64 /
    int64 host arrays).  ``to(device)`` puts it on the device once, grouped by
    (image rank, category index) in sorted id order, annotation order inside a
    cell."""

    def __init__(self, img_ids, cat_ids, cat_names, gt_img_ids, gt_cat_ids,
                 boxes, areas, iscrowd, ids, supercategories=None):
        self.img_ids = [int(i) for i in img_ids]
        self.cat_ids = [int(c) for c in cat_ids]
        self.cat_names = list(cat_names)
        # one per category (cat_ids order) or None; read by the error analysis
        self.supercategories = None if supercategories is None else \
            list(supercategories)
        if self.supercategories is not None and \
                len(self.supercategories) != len(self.cat_ids):
            raise ValueError('CocoGroundTruth: one supercategory per category')
        if len(set(self.img_ids)) != len(self.img_ids):
            raise ValueError('CocoGroundTruth: duplicate image ids')
        self.gt_img_ids = np.asarray(gt_img_ids, np.int64).reshape(-1)
        self.gt_cat_ids = np.asarray(gt_cat_ids, np.int64).reshape(-1)
        self.boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
        self.areas = np.asarray(areas, np.float64).reshape(-1)
        self.iscrowd = np.asarray(iscrowd, np.int64).reshape(-1)
        self.ids = np.asarray(ids, np.int64).reshape(-1)
        n = len(self.gt_img_ids)
        if not all(len(x) == n for x in (self.gt_cat_ids, self.boxes,
                                          self.areas, self.iscrowd, self.ids)):
            raise ValueError('CocoGroundTruth: GT fields differ in length')
        # COCOeval.evaluate: np.unique of imgIds / catIds
        self.sorted_img_ids = np.unique(np.asarray(self.img_ids, np.int64))
        self.sorted_cat_ids = np.unique(np.asarray(self.cat_ids, np.int64))
        self._dev = {}

    @classmethod
    def from_json(cls, ann_file, classes=None):
        """A COCO annotation json.  ``img_ids`` in file order (get_img_ids);
        ``cat_ids`` the categories whose name is in ``classes`` (all when
        None), in the order of ``categories`` (get_cat_ids(cat_names=...)).
        ``supercategories`` when every category has one."""
        if isinstance(ann_file, dict):
            data = ann_file
        else:
            with open(ann_file) as f:
                data = json.load(f)
        img_ids = [im['id'] for im in data.get('images', [])]
        cats = data.get('categories', [])
        if classes is not None:
            names = set(classes)
            cats = [c for c in cats if c['name'] in names]
        cat_ids = [c['id'] for c in cats]
        anns = data.get('annotations', [])
        sup = [c['supercategory'] for c in cats] \
            if all('supercategory' in c for c in cats) else None
        return cls(img_ids, cat_ids, [c['name'] for c in cats],
                   [a['image_id'] for a in anns],
                   [a['category_id'] for a in anns],
                   np.array([a['bbox'] for a in anns],
                            np.float64).reshape(-1, 4),
                   [a['area'] for a in anns],
                   [a.get('iscrowd', 0) for a in anns],
                   [a['id'] for a in anns], sup)

    @classmethod
    def from_annotations(cls, annotations, num_classes=None, classes=None,
                         supercategories=None):
        """mmdet-style ``annotations[i]``: xyxy ``bboxes`` / ``labels``, and
        ``bboxes_ignore`` / ``labels_ignore`` taken as crowd GTs.  Image ids
        are 0..N-1, category ids 0..C-1, areas w * h, annotation ids from 1
        (each image's GTs, then its crowd GTs).  ``supercategories``: one
        name per class, for the error analysis."""
        if classes is not None:
            num_classes = len(classes)
        if num_classes is None:
            labs = [np.asarray(a['labels']).reshape(-1) for a in annotations]
            labs += [np.asarray(a['labels_ignore']).reshape(-1)
                     for a in annotations
                     if a.get('labels_ignore', None) is not None]
            num_classes = int(max([x.max() + 1 for x in labs if len(x)] +
                                  [1]))
        names = list(classes) if classes is not None else \
            [str(i) for i in range(num_classes)]
        gi, gc, boxes, crowd = [], [], [], []
        for i, a in enumerate(annotations):
            parts = [(a['bboxes'], a['labels'], 0)]
            if a.get('labels_ignore', None) is not None:
                parts.append((a['bboxes_ignore'], a['labels_ignore'], 1))
            for b, lab, cr in parts:
                b = np.asarray(b, np.float32).reshape(-1, 4).astype(np.float64)
                lab = np.asarray(lab).reshape(-1)
                gi += [i] * len(lab)
                gc += [int(x) for x in lab]
                boxes.append(np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0],
                                       b[:, 3] - b[:, 1]], 1))
                crowd += [cr] * len(lab)
        boxes = np.concatenate(boxes) if boxes else np.zeros((0, 4))
        return cls(range(len(annotations)), range(num_classes), names, gi, gc,
                   boxes, boxes[:, 2] * boxes[:, 3], crowd,
                   np.arange(1, len(gi) + 1), supercategories)

    def _cells(self):
        """GT order grouped by (image rank, category index), stable; cell
        offsets; GTs of images / categories outside the sets are dropped."""
        I, K = len(self.sorted_img_ids), len(self.sorted_cat_ids)
        ri = np.searchsorted(self.sorted_img_ids, self.gt_img_ids)
        rk = np.searchsorted(self.sorted_cat_ids, self.gt_cat_ids)
        ri_c, rk_c = np.minimum(ri, max(I - 1, 0)), np.minimum(rk, max(K - 1, 0))
        keep = (ri < I) & (rk < K)
        if I and K:
            keep &= (self.sorted_img_ids[ri_c] == self.gt_img_ids) & \
                (self.sorted_cat_ids[rk_c] == self.gt_cat_ids)
        else:
            keep[:] = False
        cell = ri_c * K + rk_c
        idx = np.nonzero(keep)[0]
        idx = idx[np.argsort(cell[idx], kind='stable')]
        off = np.zeros(I * K + 1, np.int64)
        np.cumsum(np.bincount(cell[idx], minlength=I * K), out=off[1:])
        return idx, off

    def to(self, device):
        device = torch.device(device)
        d = self._dev.get(device)
        if d is not None:
            return d
        if device.type != 'cuda':
            raise L.LdError(f'CocoGroundTruth: device {device} is not a HIP '
                            'device (there is no CPU path)')
        idx, off = self._cells()
        max_cell = int(np.diff(off).max()) if len(off) > 1 else 0
        if max_cell > L.LD_COCO_MAX_CELL_GTS:
            raise L.LdError(f'CocoGroundTruth: {max_cell} GTs in one (image, '
                            f'category) cell; at most '
                            f'{L.LD_COCO_MAX_CELL_GTS} are supported')

        def put(x, dt):
            return torch.from_numpy(np.ascontiguousarray(x, dt)).to(device)

        d = dict(box=put(self.boxes[idx], np.float64).reshape(-1, 4),
                 area=put(self.areas[idx], np.float64),
                 crowd=put(self.iscrowd[idx] != 0, np.int32),
                 id=put(self.ids[idx], np.int64),
                 cell_off=put(off, np.int32), max_cell=max_cell)
        self._dev[device] = d
        return d


class _CocoStream:
    """The streaming half that CocoEvaluator and CocoErrorAnalysis share:
    the label map, one record per detection kept on the device, ``add`` and
    the images never added.  A subclass sets ``gt``, ``iou_thrs``,
    ``max_dets``, ``rec_thrs`` and ``area_rng``, calls ``_setup`` and provides
    ``_match`` (its matching kernel over one batch)."""

    def _setup(self, gt, device):
        name = type(self).__name__
        if len(gt.img_ids) == 0 or len(gt.cat_ids) == 0:
            raise ValueError(f'{name}: the ground truth has no images '
                             'or no categories')
        self.device = eval_device(device, name)
        self.num_imgs = len(gt.img_ids)
        self.K = len(gt.sorted_cat_ids)
        self._img_rank = np.searchsorted(gt.sorted_img_ids,
                                         np.asarray(gt.img_ids, np.int64))
        lut = np.searchsorted(gt.sorted_cat_ids,
                              np.asarray(gt.cat_ids, np.int64)).astype(np.int32)
        self._label_cat = torch.from_numpy(lut).to(self.device)
        self.npig = torch.zeros(self.K * len(self.area_rng), dtype=torch.int32,
                                device=self.device)
        self._seen = np.zeros(self.num_imgs, bool)
        self.num_dets = 0  # detection rows added (scored or not)
        self._rec = RecordBuffers(
            dict(score=torch.float32, cat=torch.int32, pos=torch.int32,
                 match=torch.int64, ign=torch.int64), self.device, 1 << 12)

    def _pack(self, indices, dets, labels):
        """One batch as the match kernels read it -> (dets (N, 5), labels,
        det_off, image ranks (device), per-image counts, N)."""
        dev = self.device
        d, det_off, counts = pack_rows(dets, dev, type(self).__name__)
        lab = torch.cat(labels).contiguous()
        ranks = torch.from_numpy(
            self._img_rank[np.asarray(indices, np.int64)].astype(
                np.int32)).to(dev)
        return d, lab, det_off, ranks, counts, d.shape[0]

    def add(self, indices, dets, labels):
        """One batch: ``indices`` (dataset indices into ``gt.img_ids``) and,
        per image, detections (n, 5) [x1 y1 x2 y2 score] with labels (n,) --
        device tensors as ``get_bboxes`` / ``aug_test`` return them, no host
        copy.  Label ``c`` is category ``gt.cat_ids[c]``; other labels are
        not scored.  An image may be added once."""
        name = type(self).__name__
        indices = [int(i) for i in indices]
        B = len(indices)
        if not len(dets) == len(labels) == B:
            raise ValueError(f'{name}.add: indices, dets and labels need '
                             'one entry per image')
        if B == 0:
            return
        ix = np.asarray(indices, np.int64)
        if ix.min() < 0 or ix.max() >= self.num_imgs:
            raise IndexError(f'{name}.add: image index out of range')
        if len(np.unique(ix)) != B or self._seen[ix].any():
            raise ValueError(f'{name}.add: an image was added twice')
        dev = self.device
        d = [as_boxes(x, dev, 5) for x in dets]
        lab = [as_labels(x, dev) for x in labels]
        for x, y in zip(d, lab):
            if x.shape[0] != y.shape[0]:
                raise ValueError(f'{name}.add: detections and labels '
                                 'differ in length')
        N = sum(x.shape[0] for x in d)
        rec = self._rec
        rec.reserve(N)
        self._match(indices, d, lab, self.npig, rec.views(rec.n, rec.n + N))
        self._seen[ix] = True
        rec.n += N
        self.num_dets += N

    def records(self):
        """The records written so far, in the order they were added (image
        after image, detections in their input order) -> host dict of
        ``cat`` (category index, K when not scored), ``pos`` (image rank *
        maxDets[-1] + rank in its cell), ``score``, ``match`` / ``ign``
        (uint64 masks, bit t * A + a)."""
        out = {k: v.cpu().numpy() for k, v in self._rec.views().items()}
        out['pos'] = out['pos'].view(np.uint32)
        out['match'] = out['match'].view(np.uint64)
        out['ign'] = out['ign'].view(np.uint64)
        return out

    def _npig_all(self):
        """npig with the images never added counted as images without
        detections (their GTs still count)."""
        dev = self.device
        npig = self.npig.clone()
        missing = np.nonzero(~self._seen)[0]
        if len(missing):
            empty = torch.zeros((0, 5), dtype=torch.float32, device=dev)
            none = torch.zeros(0, dtype=torch.int64, device=dev)
            self._match(missing.tolist(), [empty] * len(missing),
                        [none] * len(missing), npig, None)
        return npig

    def _accumulate(self, npig, num_thrs):
        """ld_coco_accumulate over every record -> device precision / scores
        (T, R, K, A, M) and recall (T, K, A, M)."""
        lib = L.get_lib()
        dev = self.device
        T, R, K = num_thrs, len(self.rec_thrs), self.K
        A, M = len(self.area_rng), len(self.max_dets)
        rec = self._rec
        need = lib.ld_coco_accumulate_workspace_bytes(rec.n, K, T, A, M)
        if need == 0:
            raise L.LdError('ld_coco_accumulate_workspace_bytes: bad sizes')
        ws = workspace(dev, need, 'coco_accumulate')
        precision = torch.empty((T, R, K, A, M), dtype=torch.float64,
                                device=dev)
        scores = torch.empty_like(precision)
        recall = torch.empty((T, K, A, M), dtype=torch.float64, device=dev)
        md = (L.C.c_int32 * M)(*self.max_dets)
        rt = (L.C.c_double * R)(*self.rec_thrs.tolist())
        L.check(lib.ld_coco_accumulate(
            rec.n, L.ptr(rec['score']), L.ptr(rec['cat']), L.ptr(rec['pos']),
            L.ptr(rec['match']), L.ptr(rec['ign']), K,
            len(self.gt.sorted_img_ids), T, A, M,
            L.C.cast(md, L.C.c_void_p), R, L.C.cast(rt, L.C.c_void_p),
            L.ptr(npig), L.ptr(precision), L.ptr(recall), L.ptr(scores),
            L.ptr(ws), ws.numel(), L.stream_ptr(dev)), 'ld_coco_accumulate')
        return precision, recall, scores


class CocoEvaluator(_CocoStream):
    """Streaming COCO bbox evaluation against ``gt`` (a CocoGroundTruth):
    ``add`` batches of images, then ``compute`` / ``evaluate``.

    ``iou_thrs`` (default np.linspace(.5, .95, 10)) and ``proposal_nums``
    (maxDets, default (100, 300, 1000), sorted as COCOeval.evaluate does) are
    the arguments of ``CocoDataset.evaluate``."""

    def __init__(self, gt, iou_thrs=None, proposal_nums=(100, 300, 1000),
                 device=None):
        if not isinstance(gt, CocoGroundTruth):
            raise TypeError('CocoEvaluator: gt must be a CocoGroundTruth')
        self.gt = gt
        if iou_thrs is None:
            iou_thrs = default_iou_thrs()
        self.iou_thrs = np.atleast_1d(np.asarray(iou_thrs, np.float64))
        self.max_dets = sorted(int(m) for m in proposal_nums)
        self.rec_thrs = default_rec_thrs()
        self.area_rng = np.asarray(AREA_RNG, np.float64)
        T, A = len(self.iou_thrs), len(self.area_rng)
        if not 1 <= T <= L.LD_COCO_MAX_THRS:
            raise ValueError(f'CocoEvaluator: 1..{L.LD_COCO_MAX_THRS} IoU '
                             f'thresholds, got {T}')
        if not 3 <= len(self.max_dets) <= L.LD_COCO_MAX_MAXDETS or \
                self.max_dets[0] < 1:
            raise ValueError('CocoEvaluator: proposal_nums needs 3 or 4 '
                             'positive values (summarize reads maxDets[2])')
        self._setup(gt, device)
        self._g = gt.to(self.device)

    def _match(self, indices, dets, labels, npig, records):
        """ld_coco_match over the images ``indices`` (dataset indices)."""
        lib = L.get_lib()
        dev, g = self.device, self._g
        d, lab, det_off, ranks, counts, N = self._pack(indices, dets, labels)
        b = L.CocoBatchT()
        b.dets, b.labels, b.det_off = L.ptr(d).value, L.ptr(lab).value, \
            L.ptr(det_off).value
        b.img_rank, b.label_cat = L.ptr(ranks).value, \
            L.ptr(self._label_cat).value
        b.gt_box, b.gt_area = L.ptr(g['box']).value, L.ptr(g['area']).value
        b.gt_crowd, b.gt_id = L.ptr(g['crowd']).value, L.ptr(g['id']).value
        b.gt_cell_off = L.ptr(g['cell_off']).value
        b.num_imgs, b.num_dets = len(indices), N
        b.num_labels = self._label_cat.numel()
        b.max_img_dets = max(counts) if counts else 0
        b.num_all_imgs, b.num_cats = len(self.gt.sorted_img_ids), self.K
        b.num_gts, b.max_cell_gts = g['box'].shape[0], g['max_cell']
        thr = (L.C.c_double * len(self.iou_thrs))(*self.iou_thrs.tolist())
        ar = (L.C.c_double * self.area_rng.size)(*self.area_rng.ravel().tolist())
        max_det = self.max_dets[-1]
        need = lib.ld_coco_match_workspace_bytes(N, b.max_img_dets, max_det,
                                                 b.max_cell_gts)
        if need == 0:
            raise L.LdError('ld_coco_match_workspace_bytes: bad sizes')
        ws = workspace(dev, need, 'coco_match')
        r = records if records is not None else {}
        L.check(lib.ld_coco_match(
            L.C.byref(b), len(self.iou_thrs), L.C.cast(thr, L.C.c_void_p),
            len(self.area_rng), L.C.cast(ar, L.C.c_void_p), max_det,
            L.ptr(r.get('score')), L.ptr(r.get('cat')), L.ptr(r.get('pos')),
            L.ptr(r.get('match')), L.ptr(r.get('ign')), L.ptr(npig),
            L.ptr(ws), ws.numel(), L.stream_ptr(dev)), 'ld_coco_match')
        return N

    def compute(self):
        """-> dict of ``precision`` / ``scores`` (T, R, K, A, M), ``recall``
        (T, K, A, M) float64 as COCOeval.accumulate leaves them in
        ``eval``, ``npig`` (K, A) and ``stats`` (12,) from summarize.  Images
        never added count as images without detections."""
        check_one_rank('CocoEvaluator.compute')
        npig = self._npig_all()
        precision, recall, scores = self._accumulate(npig, len(self.iou_thrs))
        out = dict(precision=precision.cpu().numpy(),
                   recall=recall.cpu().numpy(), scores=scores.cpu().numpy(),
                   npig=npig.cpu().numpy().reshape(self.K, len(self.area_rng)))
        out['stats'] = summarize(out['precision'], out['recall'],
                                 self.iou_thrs, self.max_dets)
        return out

    def evaluate(self, metric='bbox', classwise=False, metric_items=None,
                 logger=None):
        """CocoDataset.evaluate (datasets/coco.py:363-545) for
        metric='bbox': an OrderedDict of ``bbox_mAP``, ... rounded to 3
        places and ``bbox_mAP_copypaste``."""
        metrics, metric_items = check_metrics(metric, metric_items)
        log = eval_logger(logger, _LOG)
        eval_results = OrderedDict()
        for m in metrics:
            if self.num_dets == 0:  # loadRes([]) -> IndexError -> break
                log.error('The testing results of the whole dataset is empty.')
                break
            if metric_items is not None:
                for item in metric_items:
                    if item not in METRIC_NAMES:
                        raise KeyError(f'metric item {item} is not supported')
            ev = self.compute()
            stats = ev['stats']
            if classwise:
                _classwise_table(ev['precision'], self.gt, log, logger)
            items = metric_items if metric_items is not None else \
                ['mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l']
            for item in items:
                eval_results[f'{m}_{item}'] = float(
                    f'{stats[METRIC_NAMES[item]]:.3f}')
            ap = stats[:6]
            eval_results[f'{m}_mAP_copypaste'] = (
                f'{ap[0]:.3f} {ap[1]:.3f} {ap[2]:.3f} {ap[3]:.3f} '
                f'{ap[4]:.3f} {ap[5]:.3f}')
        return eval_results


def check_metrics(metric, metric_items=None):
    """coco.py:404-412 argument handling -> (metrics, metric_items); only
    'bbox' is implemented."""
    metrics = metric if isinstance(metric, list) else [metric]
    for m in metrics:
        if m not in ('bbox', 'segm', 'proposal', 'proposal_fast'):
            raise KeyError(f'metric {m} is not supported')
        if m != 'bbox':
            raise NotImplementedError(
                f'CocoEvaluator: metric {m!r} is not implemented (bbox only)')
    if metric_items is not None and not isinstance(metric_items, list):
        metric_items = [metric_items]
    return metrics, metric_items


def _classwise_table(precisions, gt, log, logger):
    """coco.py:485-512: per-category AP over precision[:, :, idx, 0, -1] (idx
    in ``cat_ids`` order, as the reference indexes it), nan without values."""
    assert len(gt.cat_ids) == precisions.shape[2]
    rows = []
    for idx, cat_id in enumerate(gt.cat_ids):
        p = precisions[:, :, idx, 0, -1]
        p = p[p > -1]
        ap = np.mean(p) if p.size else float('nan')
        rows.append((f'{gt.cat_names[idx]}', f'{float(ap):0.3f}'))
    if logger == 'silent':
        return rows
    num_columns = min(6, len(rows) * 2)
    flat = list(itertools.chain(*rows))
    table = [['category', 'AP'] * (num_columns // 2)]
    table += [list(r) for r in itertools.zip_longest(
        *[flat[i::num_columns] for i in range(num_columns)])]
    log.info('\n' + '\n'.join(' '.join(f'{str(c or ""):>12}' for c in r)
                              for r in table))
    return rows


def summarize(precision, recall, iou_thrs, max_dets):
    """COCOeval.summarize / _summarizeDets over ``eval['precision']`` and
    ``eval['recall']`` -> stats (12,)."""
    iou_thrs = np.asarray(iou_thrs)

    def _summarize(ap=1, iouThr=None, areaRng='all', maxDets=100):
        aind = [i for i, a in enumerate(AREA_LBL) if a == areaRng]
        mind = [i for i, m in enumerate(max_dets) if m == maxDets]
        if ap == 1:
            s = precision
            if iouThr is not None:
                s = s[np.where(iouThr == iou_thrs)[0]]
            s = s[:, :, :, aind, mind]
        else:
            s = recall
            if iouThr is not None:
                s = s[np.where(iouThr == iou_thrs)[0]]
            s = s[:, :, aind, mind]
        if len(s[s > -1]) == 0:
            return -1
        return np.mean(s[s > -1])

    m = max_dets
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
    return stats


def coco_evaluate(results, gt, metric='bbox', logger=None, classwise=False,
                  proposal_nums=(100, 300, 1000), iou_thrs=None,
                  metric_items=None, device=None):
    """CocoDataset.evaluate's input form: ``results[i][c]`` (k, 5) arrays per
    image (``gt.img_ids`` order) and class, scored on the device."""
    if len(results) != len(gt.img_ids):
        raise ValueError(f'coco_evaluate: {len(results)} results for '
                         f'{len(gt.img_ids)} images')
    ev = CocoEvaluator(gt, iou_thrs, proposal_nums, device)
    dets, labels = [], []
    for res in results:
        if len(res) != len(gt.cat_ids):
            raise ValueError(f'coco_evaluate: {len(res)} class arrays, '
                             f'expected {len(gt.cat_ids)}')
        rows = [np.asarray(r, np.float32).reshape(-1, 5) for r in res]
        dets.append(torch.from_numpy(np.concatenate(rows)))
        labels.append(torch.from_numpy(np.concatenate(
            [np.full(len(r), c, np.int64) for c, r in enumerate(rows)])))
    for i in range(0, len(results), ADD_STEP):
        ev.add(range(i, min(i + ADD_STEP, len(results))),
               dets[i:i + ADD_STEP], labels[i:i + ADD_STEP])
    return ev.evaluate(metric, classwise, metric_items, logger)
