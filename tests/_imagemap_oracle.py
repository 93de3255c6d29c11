"""A numpy restatement of the reference's per-image mAP
(tools/analysis_tools/analyze_results.py:13-45: ``bbox_map_eval``, i.e. eval_map
of a one-image dataset at ten IoU thresholds, averaged), written from its
behaviour, not copied from it.  Test-side checker and the host side of
tools/bench_analyze_results.py; ``ld_amd`` never imports it.

Contract restated (see also tests/_evalmap_oracle.py, whose IoU this uses):
  * per class: IoU fp32 against [GTs; ignored GTs] of the class, first maximum;
    greedy over descending score, equal scores by position (stable):
    ``f64(ious_max) >= thr`` with thr an np.float64 -- NumPy 2 promotion makes
    the reference's fp32-vs-float64 comparison a float64 one -- on a real GT
    -> TP if not yet covered else FP; on an ignored GT -> neither; else FP.
  * recall = f64(ctp) / max(f64(num_gts), f64(eps_f32)); precision = f32(ctp) /
    max(f32(ctp) + f32(cfp), eps_f32).
  * AP (mean_ap.py:34-43): mrec = [0, recall, 1], mpre = [0, precision, 0]
    in float64, running maximum from the right, np.sum over the indices where
    mrec steps, stored as float32.
  * mean_ap (mean_ap.py:392-396): float32 np.mean of the APs of the classes
    with num_gts > 0, as a Python float; 0.0 without such a class.
  * mAP (analyze_results.py:45): sum(mean_aps) / len(mean_aps) in float64.

``np_sum_model`` restates the order in which np.sum / np.mean add a contiguous
vector (what eval_image.hip reproduces); the host tests hold it to numpy.
"""
import numpy as np

import _evalmap_oracle as O

EPS32 = np.float32(np.finfo(np.float32).eps)


def default_iou_thrs():
    return np.linspace(
        .5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)


def np_sum_model(a):
    """np.add.reduce of a contiguous 1-D array, in a's dtype."""
    dt = a.dtype.type
    n = len(a)
    if n < 8:
        res = dt(0)
        for x in a:
            res = dt(res + x)
        return res
    if n <= 128:
        r = [dt(a[j]) for j in range(8)]
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] = dt(r[j] + a[i + j])
            i += 8
        res = dt(dt(dt(r[0] + r[1]) + dt(r[2] + r[3])) +
                 dt(dt(r[4] + r[5]) + dt(r[6] + r[7])))
        while i < n:
            res = dt(res + a[i])
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return dt(np_sum_model(a[:n2]) + np_sum_model(a[n2:]))


def np_mean_model(a):
    """np.mean of a float32 vector: the float32 sum, one float32 divide."""
    return np.float32(np_sum_model(a) / np.float32(len(a)))


def class_ap(dets, gts, ign, thrs, use_model=False):
    """-> (ap (T,) float32, num_gts) of one class of one image."""
    dets = np.asarray(dets, np.float32).reshape(-1, 5)
    gts = np.asarray(gts, np.float32).reshape(-1, 4)
    ign = np.asarray(ign, np.float32).reshape(-1, 4)
    n, ng = dets.shape[0], gts.shape[0]
    allg = np.concatenate([gts, ign])
    if allg.shape[0] and n:
        ious = O.iou_matrix(dets[:, :4], allg)
        best, arg = ious.max(1).astype(np.float64), ious.argmax(1)
    else:
        best, arg = np.full(n, -1.0), np.full(n, -1)
    order = np.argsort(-dets[:, 4], kind='stable')
    aps = np.zeros(len(thrs), np.float32)
    for t, thr in enumerate(thrs):
        tp, fp = np.zeros(n, np.int64), np.zeros(n, np.int64)
        taken = set()
        for i in order:
            if arg[i] >= 0 and best[i] >= np.float64(thr):
                if arg[i] >= ng:
                    continue
                if arg[i] in taken:
                    fp[i] = 1
                else:
                    taken.add(arg[i])
                    tp[i] = 1
            else:
                fp[i] = 1
        ctp, cfp = np.cumsum(tp[order]), np.cumsum(fp[order])
        rec = ctp / np.maximum(np.float64(ng), np.float64(EPS32))
        ftp = ctp.astype(np.float32)
        prec = ftp / np.maximum(ftp + cfp.astype(np.float32), EPS32)
        mrec = np.concatenate([[0.0], rec, [1.0]])
        mpre = np.concatenate([[0.0], prec.astype(np.float64), [0.0]])
        env = np.maximum.accumulate(mpre[::-1])[::-1]
        ind = np.nonzero(mrec[1:] != mrec[:-1])[0]
        terms = (mrec[ind + 1] - mrec[ind]) * env[ind + 1]
        aps[t] = np_sum_model(terms) if use_model else np.sum(terms)
    return aps, ng


def image_map(det_result, annotation, thrs=None, use_model=False):
    """-> (mAP float, mean_ap (T,) float64, ap (T, C) float32, has_gt (C,)
    uint8) of one image."""
    if isinstance(det_result, tuple):
        det_result = det_result[0]
    thrs = default_iou_thrs() if thrs is None else thrs
    C = len(det_result)
    labels = np.asarray(annotation['labels']).reshape(-1)
    boxes = np.asarray(annotation['bboxes'], np.float32).reshape(-1, 4)
    if annotation.get('labels_ignore', None) is not None:
        il = np.asarray(annotation['labels_ignore']).reshape(-1)
        ib = np.asarray(annotation['bboxes_ignore'], np.float32).reshape(-1, 4)
    else:
        il, ib = np.zeros(0, np.int64), np.zeros((0, 4), np.float32)
    ap = np.zeros((len(thrs), C), np.float32)
    has_gt = np.zeros(C, np.uint8)
    for c in range(C):
        ap[:, c], ng = class_ap(det_result[c], boxes[labels == c],
                                ib[il == c], thrs, use_model)
        has_gt[c] = ng > 0
    mean_ap = np.zeros(len(thrs), np.float64)
    sel = has_gt.astype(bool)
    if sel.any():
        for t in range(len(thrs)):
            v = np.ascontiguousarray(ap[t, sel])
            mean_ap[t] = (np_mean_model(v) if use_model else v.mean()).item()
    return sum(mean_ap.tolist()) / len(thrs), mean_ap, ap, has_gt


def bbox_map_eval(det_result, annotation):
    return image_map(det_result, annotation)[0]


def rank(maps, topk):
    """analyze_results.py:107-129 -> (good, bad) index lists."""
    n = len(maps)
    if topk * 2 > n:
        topk = n // 2
    order = sorted(range(n), key=lambda i: maps[i])  # stable
    return order[-topk:], order[:topk]
