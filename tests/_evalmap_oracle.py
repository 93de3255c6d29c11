"""A numpy restatement of the reference's VOC-style mAP, written from its
behaviour (mmdet/core/evaluation/, file:line below), not copied from it.

Differences from the reference are deliberate and only where it leaves the
answer open: detections with equal scores are ordered stably -- by image, then
by position in the class array -- inside an image (mean_ap.py:206, an unstable
np.argsort there) and across a class (mean_ap.py:333, likewise).

Contract restated:
  * IoU (bbox_overlaps.py:28-45): fp32, overlap = max(xe - xs, 0) *
    max(ye - ys, 0), union = max(area_d + area_g - overlap, fp32(1e-6)).
  * per (image, class) (mean_ap.py:176-237, get_cls_results :240-264): IoU
    against [GTs; ignored GTs] of that class, first maximum; greedy over
    descending score: ious_max >= fp32(thr) on a GT that is neither ignored nor
    out of the area range -> TP if not yet covered else FP; a matched ignored or
    out-of-range GT -> neither; unmatched -> FP if the detection's own area is in
    range (always without ranges).  No GT at all: the same unmatched rule.
  * areas compared in fp32 against fp32(lo**2), fp32(hi**2) (mean_ap.py:301).
  * num_gts (mean_ap.py:320-330): non-ignored GTs in range.
  * recall = f64(tp) / max(f64(num_gts), f64(eps_f32)); precision = f32(tp) /
    max(f32(tp) + f32(fp), eps_f32) over the class's cumulative counts
    (mean_ap.py:336-342).
  * AP 'area' (mean_ap.py:32-43): sum over recall steps of the step times the
    running maximum of precision from the right; '11points' (:44-50): the mean
    of the best precision at recall >= 0, 0.1, ... 1.0, where the division by 11
    runs once per scale that follows (inclusive) -- the reference divides the
    whole array inside its per-scale loop.
  * mean (mean_ap.py:379-393): over classes with num_gts > 0.
"""
import numpy as np

EPS32 = np.float32(np.finfo(np.float32).eps)


def _areas(b):
    b = np.asarray(b, np.float32).reshape(-1, 4)
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def iou_matrix(d, g):
    d = np.asarray(d, np.float32).reshape(-1, 4)
    g = np.asarray(g, np.float32).reshape(-1, 4)
    ad, ag = _areas(d)[:, None], _areas(g)[None, :]
    w = np.maximum(np.minimum(d[:, None, 2], g[None, :, 2]) -
                   np.maximum(d[:, None, 0], g[None, :, 0]), np.float32(0))
    h = np.maximum(np.minimum(d[:, None, 3], g[None, :, 3]) -
                   np.maximum(d[:, None, 1], g[None, :, 1]), np.float32(0))
    ov = w * h
    return ov / np.maximum(ad + ag - ov, np.float32(1e-6))


def _in_range(a, rng):
    if rng is None:
        return np.ones(a.shape, bool)
    return (a >= rng[0]) & (a < rng[1])


def tpfp(dets, gts, ign, iou_thr, area_ranges):
    """-> (tp, fp) uint8 (S, n) in the detections' own order."""
    dets = np.asarray(dets, np.float32).reshape(-1, 5)
    n = dets.shape[0]
    ranges = [None] if area_ranges is None else \
        [(np.float32(lo), np.float32(hi)) for lo, hi in area_ranges]
    tp = np.zeros((len(ranges), n), np.uint8)
    fp = np.zeros((len(ranges), n), np.uint8)
    allg = np.concatenate([np.asarray(gts, np.float32).reshape(-1, 4),
                           np.asarray(ign, np.float32).reshape(-1, 4)])
    n_real = np.asarray(gts).reshape(-1, 4).shape[0]
    det_area = _areas(dets[:, :4])
    thr = np.float32(iou_thr)
    if allg.shape[0]:
        ious = iou_matrix(dets[:, :4], allg)
        best = ious.max(1) if n else np.zeros(0, np.float32)
        arg = ious.argmax(1) if n else np.zeros(0, int)
        matched = best >= thr
    else:
        arg = np.full(n, -1)
        matched = np.zeros(n, bool)
    gt_area = _areas(allg)
    order = np.argsort(-dets[:, 4], kind='stable')
    for k, rng in enumerate(ranges):
        taken = set()
        usable = (np.arange(allg.shape[0]) < n_real) & _in_range(gt_area, rng)
        for i in order:
            if matched[i]:
                g = arg[i]
                if not usable[g]:
                    continue
                if g in taken:
                    fp[k, i] = 1
                else:
                    taken.add(g)
                    tp[k, i] = 1
            elif _in_range(det_area[i:i + 1], rng)[0]:
                fp[k, i] = 1
    return tp, fp


def average_precision(rec, prec, mode, scale_index=0, num_scales=1):
    if mode == 'area':
        if rec.size == 0:
            return np.float32(0)
        env = np.maximum.accumulate(prec[::-1].astype(np.float64))[::-1]
        step = np.diff(np.concatenate([[0.0], rec]))
        return np.float32(np.sum(step[step != 0] * env[step != 0]))
    acc = np.float32(0)
    for j in range(11):
        sel = prec[rec >= j * 0.1]
        if sel.size:
            acc = np.float32(acc + sel.max())
    for _ in range(num_scales - scale_index):
        acc = np.float32(acc / np.float32(11))
    return acc


def eval_map(det_results, annotations, scale_ranges=None, iou_thr=0.5,
             dataset=None):
    """-> (mean_ap, results, tp, fp): results as the reference's eval_map;
    tp / fp (S, total) uint8 of every class (class-major, image order)."""
    C = len(det_results[0])
    area_ranges = None if scale_ranges is None else \
        [(lo**2, hi**2) for lo, hi in scale_ranges]
    S = 1 if scale_ranges is None else len(scale_ranges)
    mode = '11points' if dataset == 'voc07' else 'area'
    results, all_tp, all_fp = [], [], []
    for c in range(C):
        tps, fps, scores, ng = [], [], [], np.zeros(S, int)
        for res, ann in zip(det_results, annotations):
            dets = np.asarray(res[c], np.float32).reshape(-1, 5)
            labels = np.asarray(ann['labels']).reshape(-1)
            gts = np.asarray(ann['bboxes'], np.float32).reshape(-1, 4)[
                labels == c]
            if ann.get('labels_ignore', None) is not None:
                il = np.asarray(ann['labels_ignore']).reshape(-1)
                ign = np.asarray(ann['bboxes_ignore'], np.float32).reshape(
                    -1, 4)[il == c]
            else:
                ign = np.zeros((0, 4), np.float32)
            t, f = tpfp(dets, gts, ign, iou_thr, area_ranges)
            tps.append(t)
            fps.append(f)
            scores.append(dets[:, 4])
            ga = _areas(gts)
            for k in range(S):
                rng = None if area_ranges is None else \
                    (np.float32(area_ranges[k][0]),
                     np.float32(area_ranges[k][1]))
                ng[k] += int(_in_range(ga, rng).sum())
        tp, fp = np.hstack(tps), np.hstack(fps)
        all_tp.append(tp)
        all_fp.append(fp)
        sc = np.concatenate(scores)
        order = np.argsort(-sc, kind='stable')
        ctp = np.cumsum(tp[:, order], 1, dtype=np.int64)
        cfp = np.cumsum(fp[:, order], 1, dtype=np.int64)
        rec = ctp / np.maximum(ng[:, None].astype(np.float64),
                               np.float64(EPS32))
        ftp = ctp.astype(np.float32)
        prec = ftp / np.maximum(ftp + cfp.astype(np.float32), EPS32)
        ap = np.array([average_precision(rec[k], prec[k], mode, k, S)
                       for k in range(S)], np.float32)
        r = {'num_gts': ng, 'num_dets': int(sc.size), 'recall': rec,
             'precision': prec, 'ap': ap}
        if scale_ranges is None:
            r = {'num_gts': int(ng[0]), 'num_dets': int(sc.size),
                 'recall': rec[0], 'precision': prec[0], 'ap': ap[0]}
        results.append(r)
    if scale_ranges is None:
        aps = [r['ap'] for r in results if r['num_gts'] > 0]
        mean_ap = float(np.mean(np.array(aps, np.float32))) if aps else 0.0
    else:
        all_ap = np.stack([r['ap'] for r in results])
        all_ng = np.stack([r['num_gts'] for r in results])
        mean_ap = [all_ap[all_ng[:, k] > 0, k].mean() if
                   (all_ng[:, k] > 0).any() else 0.0 for k in range(S)]
    return mean_ap, results, np.hstack(all_tp), np.hstack(all_fp)


def flatten(results, S):
    """results -> (num_gts (C, S), num_dets (C,), recall (S, total),
    precision (S, total), ap (C, S)) in the golden file's layout."""
    ng = np.array([np.atleast_1d(r['num_gts']) for r in results], np.int64)
    nd = np.array([r['num_dets'] for r in results], np.int64)
    rec = np.hstack([np.asarray(r['recall']).reshape(S, -1) for r in results])
    prec = np.hstack([np.asarray(r['precision']).reshape(S, -1)
                      for r in results])
    ap = np.array([np.atleast_1d(r['ap']) for r in results], np.float32)
    return ng, nd, rec, prec, ap
