"""Proposal recall on the device: the reference's ``eval_recalls``
(core/evaluation/recall.py), the ``evaluate(metric='recall')`` of its custom /
VOC datasets (datasets/custom.py:313-323, datasets/voc.py:88-100) and the
``proposal_fast`` / ``proposal`` metrics of ``CocoDataset.evaluate``
(datasets/coco.py:311-333, 425-434, 474-488), run by recall.hip
(``ld_eval_recalls_match``, ``ld_eval_recalls_count``) and, for ``proposal``,
by the coco_eval.hip kernels behind ``CocoEvaluator``.

``RecallAccumulator`` takes proposals where the heads leave them -- device
``(k, 5)`` from ``get_bboxes`` / ``aug_test`` -- batch after batch: one launch
per ``add`` orders every image's proposals by score, cuts them to
``proposal_nums[-1]``, computes the fp32 GT x proposal IoUs and runs the
reference's greedy matching for every proposal budget, one workgroup per
image.  The matched IoUs stay in a device table; ``compute`` counts them
against the thresholds in one more launch.

Numerics are the reference's: IoU fp32 in ``bbox_overlaps`` op order, the
threshold comparison in float64 (iterating a numpy array yields ``np.float64``
scalars, which NumPy 2 does not demote), recalls float64.  The cap is
``proposal_nums[-1]``, the last entry and not the largest, as recall.py:96
has it.

Equal scores: the reference orders by ``np.argsort(scores)[::-1]``, which is
not a stable sort, so the order of equal scores is open there.  Here the
proposal with the LATER index comes first (what reversing a stable ascending
sort gives).  ``(k, 4)`` proposals are taken in the given order.

Ragged inputs: the reference's ``np.array(all_ious)`` raises ``ValueError``
under NumPy >= 1.24 unless every image has the same number of GTs and of kept
proposals.  This module has no such limit; it computes what ``_recalls``
returns for the per-image IoU arrays.
"""
import logging
from collections import OrderedDict
from collections.abc import Sequence

import numpy as np
import torch

from . import lib as L
from .coco_eval import (METRIC_NAMES, CocoEvaluator, CocoGroundTruth,
                        default_iou_thrs)
from .eval_common import ADD_STEP, eval_device, eval_logger, pack_rows
from .lossblock import workspace

__all__ = ['set_recall_param', 'RecallAccumulator', 'eval_recalls',
           'print_recall_summary', 'plot_num_recall', 'plot_iou_recall',
           'coco_proposal_evaluate', 'CocoProposalEvaluator']

_LOG = logging.getLogger(__name__)


def _as_array(x, scalar, default=None):
    if x is None:
        return default
    if isinstance(x, scalar):
        return np.array([x])
    return np.array(x) if isinstance(x, Sequence) else x


def set_recall_param(proposal_nums, iou_thrs):
    """The reference's argument rules: an int budget and a float threshold
    become 1-element arrays, a sequence an array, ``None`` thresholds
    ``[0.5]``; anything else (an array, ``None`` budgets) passes through.
    -> (proposal_nums, iou_thrs)"""
    return (_as_array(proposal_nums, int),
            _as_array(iou_thrs, float, np.array([0.5])))


class RecallAccumulator:
    """Streaming ``eval_recalls``: ``add`` batches of images, then ``compute``
    / ``evaluate``.  ``proposal_nums`` and ``iou_thrs`` take what
    ``set_recall_param`` takes."""

    def __init__(self, proposal_nums, iou_thrs=0.5, device=None):
        nums, thrs = set_recall_param(proposal_nums, iou_thrs)
        if nums is None:
            raise ValueError('RecallAccumulator: proposal_nums is required')
        nums = np.atleast_1d(np.asarray(nums))
        if not np.issubdtype(nums.dtype, np.integer):
            raise ValueError('RecallAccumulator: proposal_nums must be ints')
        if not 1 <= nums.size <= L.LD_EVAL_RECALLS_MAX_NUMS or nums.ndim != 1:
            raise ValueError(
                f'RecallAccumulator: 1..{L.LD_EVAL_RECALLS_MAX_NUMS} '
                f'proposal budgets, got {nums.size}')
        if nums.min() < 0 or nums.max() >= 2 ** 31:
            raise ValueError('RecallAccumulator: proposal_nums must be >= 0')
        thrs = np.atleast_1d(np.asarray(thrs, dtype=np.float64))
        if not 1 <= thrs.size <= L.LD_EVAL_MAX_THRS or thrs.ndim != 1:
            raise ValueError(f'RecallAccumulator: 1..{L.LD_EVAL_MAX_THRS} IoU '
                             f'thresholds, got {thrs.size}')
        self.proposal_nums = nums.astype(np.int64)
        self.iou_thrs = thrs
        self.device = eval_device(device, 'recall')
        self._no_lds = False  # tests: every image through the workspace route
        self.num_imgs = 0
        self.total_gt = 0
        P = len(self.proposal_nums)
        self._table = torch.zeros((P, 0), dtype=torch.float32,
                                  device=self.device)

    def _reserve(self, extra):
        need = self.total_gt + extra
        cap = self._table.shape[1]
        if need <= cap:
            return
        cap = max(need, 2 * cap, 1 << 10)
        new = torch.zeros((self._table.shape[0], cap), dtype=torch.float32,
                          device=self.device)
        new[:, :self.total_gt] = self._table[:, :self.total_gt]
        self._table = new

    def add(self, proposals, gt_bboxes):
        """One batch: per image its proposals, ``(k, 5)`` [x1 y1 x2 y2 score]
        or ``(k, 4)`` -- device tensors (no host copy: the ``dets`` that
        ``get_bboxes`` / ``aug_test`` return go in as they are, their labels
        are not used) or numpy arrays -- and its GT boxes ``(n, 4)`` or
        ``None``.  All images of a batch that have proposals have the same
        column count.  One launch."""
        B = len(proposals)
        if len(gt_bboxes) != B:
            raise ValueError('RecallAccumulator.add: proposals and gt_bboxes '
                             'need one entry per image')
        if B == 0:
            return
        dev = self.device
        props = []
        for x in proposals:
            t = torch.as_tensor(x)
            if t.numel() == 0:
                t = t.reshape(0, 5 if t.dim() == 2 and t.shape[1] == 5 else 4)
            if t.dim() != 2 or t.shape[1] not in (4, 5):
                raise ValueError('RecallAccumulator.add: proposals must be '
                                 f'(k, 4) or (k, 5), got {tuple(t.shape)}')
            props.append(t.to(device=dev, dtype=torch.float32))
        cols = {t.shape[1] for t in props if t.shape[0]}
        if len(cols) > 1:
            raise ValueError('RecallAccumulator.add: (k, 4) and (k, 5) '
                             'proposals in one batch')
        cols = cols.pop() if cols else 4
        props = [t if t.shape[0] else t.reshape(0, cols) for t in props]
        gts = []
        for g in gt_bboxes:
            if g is None:
                gts.append(torch.zeros((0, 4), dtype=torch.float32,
                                       device=dev))
                continue
            t = torch.as_tensor(g)
            if t.numel() == 0:
                t = t.reshape(0, 4)
            if t.dim() != 2 or t.shape[1] != 4:
                raise ValueError('RecallAccumulator.add: gt_bboxes must be '
                                 f'(n, 4), got {tuple(t.shape)}')
            gts.append(t.to(device=dev, dtype=torch.float32))

        p, poff_d, pcounts = pack_rows(props, dev, 'RecallAccumulator.add')
        g, goff_d, gcounts = pack_rows(gts, dev, 'RecallAccumulator.add')
        N, G = sum(pcounts), sum(gcounts)
        if G == 0:  # no row of the table belongs to these images
            self.num_imgs += B
            return
        max_k = max(pcounts)
        self._reserve(G)
        lib = L.get_lib()
        P = len(self.proposal_nums)
        nums = (L.C.c_int32 * P)(*self.proposal_nums.tolist())
        need = lib.ld_eval_recalls_workspace_bytes(
            N, G, max_k, int(self.proposal_nums[-1]))
        if need == 0:
            raise L.LdError('ld_eval_recalls_workspace_bytes: bad sizes')
        ws = workspace(dev, need, 'eval_recalls')
        L.check(lib.ld_eval_recalls_match(
            L.ptr(p), cols, L.ptr(poff_d), L.ptr(g), L.ptr(goff_d), B, N, G,
            max_k, P, L.C.cast(nums, L.C.c_void_p),
            L.LD_EVAL_RECALLS_NO_LDS if self._no_lds else 0,
            L.ptr(self._table), self._table.shape[1], self.total_gt,
            L.ptr(ws), ws.numel(), L.stream_ptr(dev)),
            'ld_eval_recalls_match')
        self.num_imgs += B
        self.total_gt += G

    def add_results(self, results, annotations):
        """The reference's forms (custom.py:313-316): ``results[i]`` a
        ``(k, 5)`` / ``(k, 4)`` array, ``annotations[i]`` a dict with
        ``bboxes``."""
        if len(results) != len(annotations):
            raise ValueError('add_results: one annotation per image')
        self.add(results, [ann['bboxes'] for ann in annotations])

    def gt_ious(self):
        """-> device (P, total_gt) float32: row p holds, image after image,
        the IoUs that the greedy matching of budget p recorded round after
        round (``_ious`` of recall.py:15-33, before its sort)."""
        return self._table[:, :self.total_gt]

    def compute(self):
        """-> recalls (P, T) float64 (numpy); NaN without any GT, as the
        reference's division gives."""
        lib = L.get_lib()
        dev = self.device
        P, T = len(self.proposal_nums), len(self.iou_thrs)
        thr = (L.C.c_double * T)(*self.iou_thrs.tolist())
        out = torch.empty((P, T), dtype=torch.float64, device=dev)
        L.check(lib.ld_eval_recalls_count(
            L.ptr(self._table), self._table.shape[1], self.total_gt, P, T,
            L.C.cast(thr, L.C.c_void_p), L.ptr(out), L.stream_ptr(dev)),
            'ld_eval_recalls_count')
        return out.cpu().numpy()

    def evaluate(self, logger=None):
        """The OrderedDict of ``evaluate(metric='recall')``
        (custom.py:313-323): ``recall@{num}@{iou}``, and ``AR@{num}`` with
        more than one threshold."""
        recalls = self.compute()
        print_recall_summary(recalls, self.proposal_nums, self.iou_thrs,
                             logger=logger)
        eval_results = OrderedDict()
        nums = [int(n) for n in self.proposal_nums]
        for i, num in enumerate(nums):
            for j, iou in enumerate(self.iou_thrs.tolist()):
                eval_results[f'recall@{num}@{iou}'] = recalls[i, j]
        if recalls.shape[1] > 1:
            ar = recalls.mean(axis=1)
            for i, num in enumerate(nums):
                eval_results[f'AR@{num}'] = ar[i]
        return eval_results


def eval_recalls(gts, proposals, proposal_nums=None, iou_thrs=0.5,
                 logger=None, device=None):
    """The reference's ``eval_recalls`` (recall.py:64-106) on the device:
    ``gts`` a list of (n, 4) arrays or ``None``, ``proposals`` a list of
    (k, 4) / (k, 5) arrays -> recalls (P, T) float64."""
    img_num = len(gts)
    assert img_num == len(proposals)
    acc = RecallAccumulator(proposal_nums, iou_thrs, device)
    for i in range(0, img_num, ADD_STEP):
        acc.add(proposals[i:i + ADD_STEP], gts[i:i + ADD_STEP])
    recalls = acc.compute()
    print_recall_summary(recalls, acc.proposal_nums, acc.iou_thrs,
                         logger=logger)
    return recalls


def print_recall_summary(recalls, proposal_nums, iou_thrs, row_idxs=None,
                         col_idxs=None, logger=None):
    """Plain-text stand-in for recall.py:109-139 (an AsciiTable there): one
    header row of the IoU thresholds, one row per proposal budget with the
    recalls to 3 places.  Logged at INFO; ``logger='silent'`` logs nothing.
    -> the table text."""
    recalls = np.asarray(recalls)
    nums = np.asarray(proposal_nums, dtype=np.int32)
    thrs = np.asarray(iou_thrs)
    rows = range(nums.size) if row_idxs is None else list(row_idxs)
    cols = np.arange(thrs.size) if col_idxs is None else np.asarray(col_idxs)
    cells = [[''] + [str(t) for t in thrs[cols].tolist()]]
    cells += [[str(int(nums[r]))] + ['%.3f' % v for v in recalls[r, cols]]
              for r in rows]
    widths = [max(len(line[c]) for line in cells)
              for c in range(len(cells[0]))]
    text = '\n'.join(' '.join(cell.rjust(w) for cell, w in zip(line, widths))
                     for line in cells)
    if logger != 'silent':
        eval_logger(logger, _LOG).info('\n' + text)
    return text


def _curve(xs, ys, xlabel, x_from, x_to):
    """One recall curve on the non-interactive Agg backend -> the figure."""
    import matplotlib
    matplotlib.use('Agg')  # never a display
    import matplotlib.pyplot as plt
    fig = plt.figure()
    ax = fig.gca()
    ax.plot(xs, ys)
    ax.set_xlabel(xlabel)
    ax.set_ylabel('Recall')
    ax.set_xlim(x_from, x_to)
    ax.set_ylim(0, 1)
    return fig


def plot_num_recall(recalls, proposal_nums):
    """The proposal_num - recall curve of the reference's ``plot_num_recall``,
    from the origin; arrays or lists of one length.  The figure is returned
    and not shown."""
    nums = np.asarray(proposal_nums).tolist()
    return _curve([0] + nums, [0] + np.asarray(recalls).tolist(),
                  'Proposal num', 0, max(nums))


def plot_iou_recall(recalls, iou_thrs):
    """The IoU - recall curve of the reference's ``plot_iou_recall``, closed
    with recall 0 at IoU 1; as ``plot_num_recall``."""
    thrs = np.asarray(iou_thrs).tolist()
    return _curve(thrs + [1.0], np.asarray(recalls).tolist() + [0.0], 'IoU',
                  min(thrs), 1)


# ------------------------------------------------------------------- COCO ----
PROPOSAL_ITEMS = ['AR@100', 'AR@300', 'AR@1000', 'AR_s@1000', 'AR_m@1000',
                  'AR_l@1000']


def _fast_gt_bboxes(gt):
    """fast_eval_recall's GT list (coco.py:312-328): per image of
    ``gt.img_ids`` every annotation of the image that is not crowd, in
    annotation order, xyxy in float32; (0, 4) without any.  The reference
    also drops an annotation whose json carries a true ``ignore`` key
    (coco.py:320); ``CocoGroundTruth`` keeps no such field (COCOeval
    overwrites it with ``iscrowd``), so that key is NOT honoured here: mark
    such annotations ``iscrowd`` to leave them out."""
    by_img = {}
    for n in np.nonzero(gt.iscrowd == 0)[0]:
        by_img.setdefault(int(gt.gt_img_ids[n]), []).append(n)
    out = []
    for img in gt.img_ids:
        idx = by_img.get(img)
        if not idx:
            out.append(np.zeros((0, 4), np.float32))
            continue
        b = gt.boxes[idx]
        out.append(np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2],
                             b[:, 1] + b[:, 3]], 1).astype(np.float32))
    return out


def _agnostic_gt(gt):
    """The class-agnostic view COCOeval makes with ``useCats = 0``: the GTs of
    the categories in ``gt.cat_ids``, every one mapped to ONE category, ordered
    per image category-major in ``cat_ids`` order and in annotation order
    inside a category (evaluateImg: ``[_ for cId in p.catIds for _ in
    self._gts[imgId, cId]]``)."""
    rank = {c: i for i, c in enumerate(gt.cat_ids)}
    key = np.array([rank.get(int(c), -1) for c in gt.gt_cat_ids], np.int64)
    idx = np.nonzero(key >= 0)[0]
    idx = idx[np.argsort(key[idx], kind='stable')]
    return CocoGroundTruth(gt.img_ids, [1], ['object'], gt.gt_img_ids[idx],
                           np.ones(len(idx), np.int64), gt.boxes[idx],
                           gt.areas[idx], gt.iscrowd[idx], gt.ids[idx])


def _image_dets(res):
    """One image's result -> (k, 5) rows in ``_det2json`` order: an array as
    it is, a list of per-class arrays concatenated in class order, the bbox
    part of a ``(bbox, segm)`` tuple."""
    if isinstance(res, tuple):
        res = res[0]
    if isinstance(res, (list, tuple)):
        rows = [torch.as_tensor(r).reshape(-1, 5) for r in res]
        return torch.cat(rows) if rows else torch.zeros((0, 5))
    return torch.as_tensor(res).reshape(-1, 5)


class CocoProposalEvaluator:
    """Streaming ``proposal_fast`` / ``proposal`` of ``CocoDataset.evaluate``
    against ``gt`` (a CocoGroundTruth): ``add`` batches of images, then
    ``evaluate``.

    ``proposal_fast`` is ``eval_recalls`` of the non-crowd GTs
    (coco.py:311-333) through a ``RecallAccumulator``; it needs the images
    added in ``gt.img_ids`` order, every image once.  ``proposal`` is COCOeval
    with ``useCats = 0`` (coco.py:474-488) through a ``CocoEvaluator`` over a
    class-agnostic view of ``gt``, every detection with label 0; an image with
    more than ``LD_COCO_MAX_CELL_GTS`` GTs is refused as ``CocoGroundTruth``
    refuses it.  (The reference's ``_proposal2json`` writes category id 1 for
    every proposal, so its ``proposal`` scores them only when 1 is one of the
    dataset's category ids; here they are always scored.)"""

    def __init__(self, gt, metric='proposal_fast', proposal_nums=(100, 300,
                                                                  1000),
                 iou_thrs=None, device=None):
        if not isinstance(gt, CocoGroundTruth):
            raise TypeError('CocoProposalEvaluator: gt must be a '
                            'CocoGroundTruth')
        self.metrics = metric if isinstance(metric, list) else [metric]
        for m in self.metrics:
            if m not in ('proposal', 'proposal_fast'):
                raise KeyError(f'metric {m} is not supported')
        self.gt = gt
        self.proposal_nums = proposal_nums
        self.iou_thrs = default_iou_thrs() if iou_thrs is None else iou_thrs
        self.device = eval_device(device, 'recall')
        self._fast = self._coco = None
        self._next = 0
        if 'proposal_fast' in self.metrics:
            self._fast = RecallAccumulator(proposal_nums, self.iou_thrs,
                                           self.device)
            self._fast_gts = _fast_gt_bboxes(gt)
        if 'proposal' in self.metrics:
            self._coco = CocoEvaluator(_agnostic_gt(gt), self.iou_thrs,
                                       proposal_nums, self.device)

    def add(self, indices, dets):
        """One batch: ``indices`` (dataset indices into ``gt.img_ids``) and
        per image its proposals / detections ``(k, 5)`` -- device tensors or
        arrays; labels are not needed."""
        indices = [int(i) for i in indices]
        if len(dets) != len(indices):
            raise ValueError('CocoProposalEvaluator.add: one entry per image')
        if not indices:
            return
        d = [torch.as_tensor(x).reshape(-1, 5) for x in dets]
        if self._fast is not None:
            if indices != list(range(self._next, self._next + len(indices))):
                raise ValueError(
                    'CocoProposalEvaluator.add: proposal_fast needs the '
                    'images in dataset order, every image once')
            self._fast.add(d, [self._fast_gts[i] for i in indices])
        if self._coco is not None:
            dev = self.device
            self._coco.add(indices, d, [
                torch.zeros(x.shape[0], dtype=torch.int64, device=dev)
                for x in d])
        self._next += len(indices)

    def evaluate(self, metric_items=None, logger=None):
        """-> OrderedDict: ``AR@{num}`` of ``proposal_fast``
        (``recalls.mean(axis=1)``, not rounded, coco.py:425-434), then the
        items of ``proposal`` rounded to 3 places (coco.py:468-488; default
        ``AR@100 ... AR_l@1000``)."""
        if metric_items is not None and not isinstance(metric_items, list):
            metric_items = [metric_items]
        log = eval_logger(logger, _LOG)
        eval_results = OrderedDict()
        for m in self.metrics:
            if m == 'proposal_fast':
                if self._next != len(self.gt.img_ids):
                    raise ValueError(
                        f'proposal_fast: {self._next} of '
                        f'{len(self.gt.img_ids)} images were added')
                ar = self._fast.compute().mean(axis=1)
                msg = []
                for i, num in enumerate(self.proposal_nums):
                    eval_results[f'AR@{num}'] = ar[i]
                    msg.append(f'\nAR@{num}\t{ar[i]:.4f}')
                if logger != 'silent':
                    log.info(''.join(msg))
                continue
            if self._coco.num_dets == 0:  # loadRes([]) -> IndexError -> break
                log.error('The testing results of the whole dataset is empty.')
                break
            if metric_items is not None:
                for item in metric_items:
                    if item not in METRIC_NAMES:
                        raise KeyError(f'metric item {item} is not supported')
            stats = self._coco.compute()['stats']
            if metric_items is None:  # kept for later metrics, as there
                metric_items = list(PROPOSAL_ITEMS)
            for item in metric_items:
                eval_results[item] = float(f'{stats[METRIC_NAMES[item]]:.3f}')
        return eval_results


def coco_proposal_evaluate(results, gt, metric='proposal_fast',
                           proposal_nums=(100, 300, 1000), iou_thrs=None,
                           metric_items=None, logger=None, device=None):
    """``CocoDataset.evaluate(results, metric='proposal' | 'proposal_fast')``
    on the device.  ``results[i]`` is image i's (``gt.img_ids`` order)
    ``(k, 5)`` proposal array.  A list of per-class ``(k, 5)`` arrays (a
    detector's result) is concatenated in class order, which is ``_det2json``
    order; the reference scores such results under ``proposal`` but crashes on
    them under ``proposal_fast`` (``eval_recalls`` reads ``.ndim`` of a
    list)."""
    if len(results) != len(gt.img_ids):
        raise ValueError(f'coco_proposal_evaluate: {len(results)} results '
                         f'for {len(gt.img_ids)} images')
    ev = CocoProposalEvaluator(gt, metric, proposal_nums, iou_thrs, device)
    dets = [_image_dets(r) for r in results]
    for i in range(0, len(dets), ADD_STEP):
        ev.add(range(i, min(i + ADD_STEP, len(dets))), dets[i:i + ADD_STEP])
    return ev.evaluate(metric_items, logger)
