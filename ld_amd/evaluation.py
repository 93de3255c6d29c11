"""Detection mAP on the device: the reference's ``eval_map`` (core/evaluation/
mean_ap.py:267-402) and the ``evaluate(metric='mAP')`` of its datasets
(datasets/custom.py:297-312), run by the eval.hip kernels.

``MapAccumulator`` takes the detections where the heads leave them -- device
``(n, 5)`` + ``(n,)`` from ``get_bboxes`` / ``aug_test`` -- batch after batch,
keeps one TP/FP record per (detection, IoU threshold) on the device, and
finalizes every class at once (``ld_eval_ap``).  ``eval_map`` is the
reference's list-of-per-class-arrays interface on top of it.

Numerics follow the reference: IoU, areas and the IoU / area-range
comparisons in fp32, recall float64, precision fp32 (exact TP / FP counts
below 2**24), AP summed in float64 and stored as float32.  Detections with
equal scores in one class are ordered by (image, position in the class array),
i.e. a stable sort; the reference's ``np.argsort`` leaves that order open.
"""
import logging
from collections import OrderedDict

import numpy as np
import torch

from . import lib as L
from .eval_common import (RecordBuffers, check_one_rank, eval_batch,
                          eval_device, eval_logger, pack_det_gt_batch,
                          results_to_lists)
from .lossblock import workspace

__all__ = ['eval_map', 'MapAccumulator']

_LOG = logging.getLogger(__name__)


def _refuse_tpfp(dataset, tpfp_fn):
    if tpfp_fn is not None:
        raise NotImplementedError(
            'eval_map: a custom tpfp_fn is not supported; TP/FP are computed '
            'on the device with tpfp_default semantics')
    if dataset in ('det', 'vid'):
        raise NotImplementedError(
            f'eval_map: dataset={dataset!r} needs tpfp_imagenet, which ld_amd '
            'does not implement')


def eval_tpfp(batch, num_classes, area_ranges, iou_thrs, rec_score, rec_seg,
              rec_bits, num_gts):
    """ld_eval_tpfp on packed device tensors (see include/ld_hip.h).
    ``batch``: dict of dets / det_labels / det_off, gts / gt_labels / gt_off,
    ign / ign_labels / ign_off; the record tensors are views of the slots to
    fill (num_dets * len(iou_thrs) each)."""
    lib = L.get_lib()
    dev = batch['det_off'].device
    b = eval_batch(batch)
    S = 1 if area_ranges is None else len(area_ranges)
    ar = None
    if area_ranges is not None:
        ar = (L.C.c_float * (2 * S))(
            *[float(v) for rg in area_ranges for v in rg])
    thr = (L.C.c_float * len(iou_thrs))(*[float(t) for t in iou_thrs])
    need = lib.ld_eval_tpfp_workspace_bytes(b.num_dets)
    ws = workspace(dev, need, 'eval_tpfp')
    L.check(lib.ld_eval_tpfp(
        L.C.byref(b), int(num_classes), S,
        L.C.cast(ar, L.C.c_void_p) if ar is not None else None, len(iou_thrs),
        L.C.cast(thr, L.C.c_void_p), L.ptr(rec_score), L.ptr(rec_seg),
        L.ptr(rec_bits), L.ptr(num_gts), L.ptr(ws), ws.numel(),
        L.stream_ptr(dev)), 'ld_eval_tpfp')


def eval_ap(rec_score, rec_seg, rec_bits, num_classes, num_thrs, num_scales,
            num_gts, eleven_points):
    """ld_eval_ap over R records -> (seg_start (T*C+1,), recall (S, R) f64,
    precision (S, R) f32, ap (T*C, S) f32), device tensors."""
    lib = L.get_lib()
    dev = num_gts.device
    R = rec_score.numel()
    segs = num_thrs * num_classes
    need = lib.ld_eval_ap_workspace_bytes(R, num_scales)
    if need == 0:
        raise L.LdError('eval_ap: bad record count / scale count')
    ws = workspace(dev, need, 'eval_ap')
    seg_start = torch.empty(segs + 1, dtype=torch.int32, device=dev)
    recall = torch.empty((num_scales, R), dtype=torch.float64, device=dev)
    precision = torch.empty((num_scales, R), dtype=torch.float32, device=dev)
    ap = torch.empty((segs, num_scales), dtype=torch.float32, device=dev)
    L.check(lib.ld_eval_ap(
        R, L.ptr(rec_score), L.ptr(rec_seg), L.ptr(rec_bits), int(num_classes),
        int(num_thrs), int(num_scales), L.ptr(num_gts),
        L.LD_EVAL_11POINTS if eleven_points else 0, L.ptr(seg_start),
        L.ptr(recall), L.ptr(precision), L.ptr(ap), L.ptr(ws), ws.numel(),
        L.stream_ptr(dev)), 'ld_eval_ap')
    return seg_start, recall, precision, ap


class MapAccumulator:
    """Streaming mAP: ``add`` batches of images, then ``compute`` /
    ``evaluate``.

    ``iou_thrs``: the IoU thresholds to score at once (one ``eval_map`` result
    each); ``scale_ranges``: ``[(min, max), ...]`` scale bounds (areas are
    their squares) or None; ``dataset='voc07'`` selects 11-point AP."""

    def __init__(self, num_classes, iou_thrs=(0.5, ), scale_ranges=None,
                 dataset=None, device=None):
        _refuse_tpfp(dataset, None)
        if isinstance(iou_thrs, (int, float)):
            iou_thrs = (iou_thrs, )
        self.iou_thrs = tuple(float(t) for t in iou_thrs)
        if not 1 <= len(self.iou_thrs) <= L.LD_EVAL_MAX_THRS:
            raise ValueError(f'MapAccumulator: 1..{L.LD_EVAL_MAX_THRS} IoU '
                             f'thresholds, got {len(self.iou_thrs)}')
        self.num_classes = int(num_classes)
        if self.num_classes < 1:
            raise ValueError('MapAccumulator: num_classes must be >= 1')
        self.scale_ranges = None if scale_ranges is None else \
            [tuple(rg) for rg in scale_ranges]
        if self.scale_ranges is not None and not \
                1 <= len(self.scale_ranges) <= L.LD_EVAL_MAX_SCALES:
            raise ValueError(f'MapAccumulator: 1..{L.LD_EVAL_MAX_SCALES} '
                             'scale ranges')
        # mean_ap.py:301-302; the comparisons are against their fp32 values
        self.area_ranges = None if self.scale_ranges is None else \
            [(np.float32(rg[0]**2), np.float32(rg[1]**2))
             for rg in self.scale_ranges]
        self.dataset = dataset
        self.device = eval_device(device, 'MapAccumulator')
        S = 1 if self.scale_ranges is None else len(self.scale_ranges)
        self.num_scales = S
        self.num_gts = torch.zeros(self.num_classes * S, dtype=torch.int32,
                                   device=self.device)
        self.num_imgs = 0
        self._rec = RecordBuffers(
            dict(score=torch.float32, seg=torch.int32, bits=torch.int32),
            self.device, 1 << 12)

    def add(self, dets, labels, gt_bboxes, gt_labels, gt_bboxes_ignore=None,
            gt_labels_ignore=None):
        """One batch: lists (one entry per image) of detections (n, 5) with
        labels (n,) -- device tensors as the heads return them, no host copy
        -- and GTs (g, 4) / (g,), optionally ignored GTs (k, 4) / (k,).  Boxes
        are compared in fp32.  Detection labels outside [0, num_classes) are
        not scored."""
        batch = pack_det_gt_batch(
            'MapAccumulator.add', ('dets', 'labels'), dets, labels, gt_bboxes,
            gt_labels, gt_bboxes_ignore, gt_labels_ignore, self.device)
        if batch is None:
            return
        rec = self._rec
        R = batch['dets'].shape[0] * len(self.iou_thrs)
        rec.reserve(R)
        new = rec.views(rec.n, rec.n + R)
        eval_tpfp(batch, self.num_classes, self.area_ranges, self.iou_thrs,
                  new['score'], new['seg'], new['bits'], self.num_gts)
        rec.n += R
        self.num_imgs += batch['det_off'].numel() - 1

    def add_results(self, det_results, annotations):
        """The reference's form: ``det_results[i][c]`` (k, 5) arrays per image
        and class, ``annotations[i]`` dicts of ``bboxes`` / ``labels`` and
        optional ``bboxes_ignore`` / ``labels_ignore`` (numpy or tensors)."""
        self.add(*results_to_lists(det_results, annotations,
                                   self.num_classes))

    def records(self):
        """The TP/FP records written so far, in the order they were added
        (image after image, detections in their input order, thresholds
        innermost) -> host (threshold (R,), class (R,), score (R,), tp (S, R),
        fp (S, R)); class -1 marks a label outside [0, num_classes)."""
        C_, S = self.num_classes, self.num_scales
        rec = self._rec.views()
        seg = rec['seg'].cpu().numpy().astype(np.int64)
        bits = rec['bits'].cpu().numpy().view(np.uint32)
        valid = seg < len(self.iou_thrs) * C_
        k = np.arange(S, dtype=np.uint32)[:, None]
        tp = ((bits[None] >> k) & 1).astype(np.uint8)
        fp = ((bits[None] >> (k + 16)) & 1).astype(np.uint8)
        return (np.where(valid, seg // C_, -1), np.where(valid, seg % C_, -1),
                rec['score'].cpu().numpy(), tp, fp)

    def compute(self, logger=None):
        """-> one ``(mean_ap, eval_results)`` per IoU threshold, shaped as the
        reference's ``eval_map`` returns them."""
        check_one_rank('MapAccumulator.compute')
        T, C_, S = len(self.iou_thrs), self.num_classes, self.num_scales
        rec = self._rec.views()
        seg_start, recall, precision, ap = eval_ap(
            rec['score'], rec['seg'], rec['bits'], C_, T, S, self.num_gts,
            self.dataset == 'voc07')
        seg_start = seg_start.cpu().numpy().astype(np.int64)
        recall, precision = recall.cpu().numpy(), precision.cpu().numpy()
        ap = ap.cpu().numpy()
        num_gts = self.num_gts.cpu().numpy().astype(int).reshape(C_, S)
        out = []
        for t, thr in enumerate(self.iou_thrs):
            eval_results = []
            for c in range(C_):
                s = t * C_ + c
                lo, hi = seg_start[s], seg_start[s + 1]
                r = {'num_gts': num_gts[c].copy(), 'num_dets': int(hi - lo),
                     'recall': recall[:, lo:hi].copy(),
                     'precision': precision[:, lo:hi].copy(),
                     'ap': ap[s].copy()}
                if self.scale_ranges is None:  # mean_ap.py:345-348
                    r['recall'], r['precision'] = r['recall'][0], \
                        r['precision'][0]
                    r['num_gts'] = r['num_gts'].item()
                    r['ap'] = r['ap'][0]
                eval_results.append(r)
            mean_ap = _mean_ap(eval_results, self.scale_ranges)
            _summary(mean_ap, eval_results, thr, self.area_ranges, logger)
            out.append((mean_ap, eval_results))
        return out

    def evaluate(self, logger=None):
        """CustomDataset.evaluate(metric='mAP', iou_thr=self.iou_thrs)
        (datasets/custom.py:297-312): ``AP50``, ... rounded to 3 places and the
        unrounded mean over thresholds as ``mAP``."""
        if self.scale_ranges is not None:
            raise ValueError('evaluate: with scale_ranges the mean AP is a list '
                             'per scale; use compute()')
        res = OrderedDict()
        mean_aps = []
        for thr, (mean_ap, _) in zip(self.iou_thrs, self.compute(logger)):
            mean_aps.append(mean_ap)
            res[f'AP{int(thr * 100):02d}'] = round(mean_ap, 3)
        res['mAP'] = sum(mean_aps) / len(mean_aps)
        return res


def _mean_ap(eval_results, scale_ranges):
    """mean_ap.py:379-393: mean over the classes with GTs."""
    if scale_ranges is not None:
        all_ap = np.vstack([r['ap'] for r in eval_results])
        all_num_gts = np.vstack([r['num_gts'] for r in eval_results])
        mean_ap = []
        for i in range(len(scale_ranges)):
            if np.any(all_num_gts[:, i] > 0):
                mean_ap.append(all_ap[all_num_gts[:, i] > 0, i].mean())
            else:
                mean_ap.append(0.0)
        return mean_ap
    aps = [r['ap'] for r in eval_results if r['num_gts'] > 0]
    return np.array(aps).mean().item() if aps else 0.0


def _summary(mean_ap, eval_results, iou_thr, area_ranges, logger):
    """Plain-text stand-in for print_map_summary (mean_ap.py:405-470)."""
    if logger == 'silent':
        return
    log = eval_logger(logger, _LOG)
    S = 1 if area_ranges is None else len(area_ranges)
    lines = [f'mAP @ IoU {iou_thr}']
    for k in range(S):
        if area_ranges is not None:
            lines.append(f'area range [{area_ranges[k][0]}, '
                         f'{area_ranges[k][1]})')
        lines.append(f'{"class":>6} {"gts":>7} {"dets":>8} {"recall":>7} '
                     f'{"ap":>7}')
        for c, r in enumerate(eval_results):
            ng = np.atleast_1d(r['num_gts'])[k]
            rec = np.atleast_2d(r['recall'])[k] if r['num_dets'] else []
            ap = np.atleast_1d(r['ap'])[k]
            lines.append(f'{c:>6} {int(ng):>7} {r["num_dets"]:>8} '
                         f'{(rec[-1] if len(rec) else 0.0):>7.3f} '
                         f'{float(ap):>7.3f}')
        m = mean_ap if area_ranges is None else mean_ap[k]
        lines.append(f'{"mAP":>6} {"":>7} {"":>8} {"":>7} {float(m):>7.3f}')
    log.info('\n'.join(lines))


def eval_map(det_results, annotations, scale_ranges=None, iou_thr=0.5,
             dataset=None, logger=None, tpfp_fn=None, nproc=4):
    """The reference's eval_map (mean_ap.py:267-402) on the device: same
    arguments, ``(mean_ap, [{num_gts, num_dets, recall, precision, ap}, ...])``
    with its dtypes and shapes.  ``nproc`` is accepted and ignored;
    ``tpfp_fn`` and ``dataset in ('det', 'vid')`` (tpfp_imagenet) are refused.
    The per-class summary goes to ``logging`` (``logger``: a Logger, a logger
    name, 'silent' or None)."""
    _refuse_tpfp(dataset, tpfp_fn)
    assert len(det_results) == len(annotations)
    if not det_results:
        raise ValueError('eval_map: no images')
    acc = MapAccumulator(len(det_results[0]), (iou_thr, ), scale_ranges,
                         dataset)
    acc.add_results(det_results, annotations)
    return acc.compute(logger)[0]
