"""COCO error analysis on the device: the reference's
``tools/analysis_tools/coco_error_analysis.py`` (``analyze_results``,
``analyze_individual_category``, ``makeplot``; bbox only), the per-category
breakdown of precision into C75 / C50 / Loc / Sim / Oth / BG / FN.

The reference runs 1 + 2 K full COCOeval passes.  Here one
``ld_coco_match_errors`` call per batch of images writes every row's match
bits: C75 / C50 / Loc (IoU .75 / .5 / .1), then Sim and Oth at IoU .1, where
the image's GTs of the other categories of the same supercategory (Sim) or of
every other category (Oth) act as ignored crowd GTs of the detection's
category.  One ``ld_coco_accumulate`` (5 thresholds, maxDets [100]) then gives
``precision`` rows 0-4 of every category, and the host applies the
reference's fill: -1 -> 0, BG = (Oth > 0), FN = 1.

Kept from the reference, on purpose:
- a relabelled GT's overlap is intersection / detection area (crowd), it is
  never consumed, and it never changes npig;
- the GTs of a cell are in annotation order within the image, so equal
  overlaps are resolved as pycocotools' stable sort resolves them;
- categories without GTs count as 0 (BG, and 1 for FN) in the all-class mean.
Refused: category ids not listed in ascending order (the reference indexes
``precision`` by file order), a ground truth without supercategories, and
``'segm'``.
"""
import json
import os
from collections import OrderedDict

import numpy as np
import torch

from . import lib as L
from .coco_eval import (AREA_RNG, CocoGroundTruth, _CocoStream,
                        default_rec_thrs)
from .eval_common import ADD_STEP, check_one_rank
from .lossblock import workspace

__all__ = ['CocoErrorAnalysis', 'coco_error_analysis', 'TYPES', 'AREA_NAMES']

TYPES = ['C75', 'C50', 'Loc', 'Sim', 'Oth', 'BG', 'FN']
AREA_NAMES = ['allarea', 'small', 'medium', 'large']
MAIN_THRS = [.75, .5, .1]  # rows 0-2: cocoEval.params.iouThrs
ERR_THR = .1  # rows 3-4: analyze_individual_category's iouThrs
MAX_DET = 100


def check_analysable(gt, name='CocoErrorAnalysis'):
    """The reference's preconditions on the annotation set."""
    if not isinstance(gt, CocoGroundTruth):
        raise TypeError(f'{name}: gt must be a CocoGroundTruth')
    if gt.supercategories is None:
        raise ValueError(f'{name}: the ground truth has no supercategories '
                         '(the Sim row needs them)')
    ids = np.asarray(gt.cat_ids, np.int64)
    if np.any(np.diff(ids) <= 0):
        raise ValueError(f'{name}: category ids must be listed in ascending '
                         'order (the reference indexes precision by file '
                         'order)')


def fill(raw):
    """analyze_results' post-processing of the device rows (5, R, K, A, 1):
    stack 2 zero rows, -1 -> 0, BG = (Oth > 0), FN = 1 -> (7, R, K, A, 1)."""
    ps = np.vstack([raw, np.zeros((2, *raw.shape[1:]))])
    ps[ps == -1] = 0
    ps[5] = ps[4] > 0
    ps[6] = 1.0
    return ps


def _area_aps(ps):
    """makeplot's legend numbers: per area, the mean of each type over every
    axis but the area's (``ps`` (7, R, [K,] A, 1))."""
    out = OrderedDict()
    for i, area in enumerate(AREA_NAMES):
        area_ps = ps[..., i, 0]
        out[area] = OrderedDict(
            (t, float(ps_.mean())) for t, ps_ in zip(TYPES, area_ps))
    return out


def aps_table(ps, class_names):
    """{class name: {area: {type: ap}}} for every category (figures
    ``{class}-{area}``), then ``'allclass'``."""
    table = OrderedDict()
    for k, nm in enumerate(class_names):
        table[nm] = _area_aps(ps[:, :, k])
    table['allclass'] = _area_aps(ps)
    return table


class CocoErrorAnalysis(_CocoStream):
    """Streaming error analysis against ``gt`` (a CocoGroundTruth with
    supercategories, category ids ascending): ``add`` batches as for
    CocoEvaluator (device ``(n, 5)`` + ``(n,)`` from ``get_bboxes`` /
    ``aug_test``), then ``compute``."""

    def __init__(self, gt, device=None):
        check_analysable(gt)
        self.gt = gt
        self.iou_thrs = np.asarray(MAIN_THRS, np.float64)
        self.max_dets = [MAX_DET]
        self.rec_thrs = default_rec_thrs()
        self.area_rng = np.asarray(AREA_RNG, np.float64)
        self._setup(gt, device)
        self._g = self._upload(gt)

    def _upload(self, gt):
        """The GTs grouped by image rank only, annotation order inside an
        image; the category index (-1 outside the set) and each category's
        supercategory index."""
        I = len(gt.sorted_img_ids)
        ri = np.searchsorted(gt.sorted_img_ids, gt.gt_img_ids)
        ri_c = np.minimum(ri, I - 1)
        keep = (ri < I) & (gt.sorted_img_ids[ri_c] == gt.gt_img_ids)
        idx = np.nonzero(keep)[0]
        idx = idx[np.argsort(ri_c[idx], kind='stable')]
        off = np.zeros(I + 1, np.int64)
        np.cumsum(np.bincount(ri_c[idx], minlength=I), out=off[1:])
        max_img = int(np.diff(off).max())
        if max_img > L.LD_COCO_MAX_CELL_GTS:
            raise L.LdError(f'CocoErrorAnalysis: {max_img} GTs in one image; '
                            f'at most {L.LD_COCO_MAX_CELL_GTS} are supported')
        K = len(gt.sorted_cat_ids)
        rk = np.searchsorted(gt.sorted_cat_ids, gt.gt_cat_ids[idx])
        rk_c = np.minimum(rk, K - 1)
        cat = np.where((rk < K) & (gt.sorted_cat_ids[rk_c] ==
                                   gt.gt_cat_ids[idx]), rk_c, -1)
        names = {}
        # cat_ids ascending: file order is the sorted-id order
        sup = [names.setdefault(s, len(names)) for s in gt.supercategories]
        dev = self.device

        def put(x, dt):
            return torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)

        return dict(box=put(gt.boxes[idx], np.float64).reshape(-1, 4),
                    area=put(gt.areas[idx], np.float64),
                    crowd=put(gt.iscrowd[idx] != 0, np.int32),
                    id=put(gt.ids[idx], np.int64), cat=put(cat, np.int32),
                    img_off=put(off, np.int32), cat_sup=put(sup, np.int32),
                    max_img=max_img)

    def _match(self, indices, dets, labels, npig, records):
        """ld_coco_match_errors over the images ``indices``."""
        lib = L.get_lib()
        dev, g = self.device, self._g
        d, lab, det_off, ranks, counts, N = self._pack(indices, dets, labels)
        b = L.CocoErrBatchT()
        b.dets, b.labels, b.det_off = L.ptr(d).value, L.ptr(lab).value, \
            L.ptr(det_off).value
        b.img_rank, b.label_cat = L.ptr(ranks).value, \
            L.ptr(self._label_cat).value
        b.gt_box, b.gt_area = L.ptr(g['box']).value, L.ptr(g['area']).value
        b.gt_crowd, b.gt_id = L.ptr(g['crowd']).value, L.ptr(g['id']).value
        b.gt_cat, b.gt_img_off = L.ptr(g['cat']).value, \
            L.ptr(g['img_off']).value
        b.cat_sup = L.ptr(g['cat_sup']).value
        b.num_imgs, b.num_dets = len(indices), N
        b.num_labels = self._label_cat.numel()
        b.max_img_dets = max(counts) if counts else 0
        b.num_all_imgs, b.num_cats = len(self.gt.sorted_img_ids), self.K
        b.num_gts, b.max_img_gts = g['box'].shape[0], g['max_img']
        thr = (L.C.c_double * len(self.iou_thrs))(*self.iou_thrs.tolist())
        ar = (L.C.c_double * self.area_rng.size)(*self.area_rng.ravel().tolist())
        need = lib.ld_coco_match_errors_workspace_bytes(
            N, b.max_img_dets, MAX_DET, b.max_img_gts)
        if need == 0:
            raise L.LdError('ld_coco_match_errors_workspace_bytes: bad sizes')
        ws = workspace(dev, need, 'coco_match')
        r = records if records is not None else {}
        L.check(lib.ld_coco_match_errors(
            L.C.byref(b), len(self.iou_thrs), L.C.cast(thr, L.C.c_void_p),
            ERR_THR, len(self.area_rng), L.C.cast(ar, L.C.c_void_p), MAX_DET,
            L.ptr(r.get('score')), L.ptr(r.get('cat')), L.ptr(r.get('pos')),
            L.ptr(r.get('match')), L.ptr(r.get('ign')), L.ptr(npig),
            L.ptr(ws), ws.numel(), L.stream_ptr(dev)), 'ld_coco_match_errors')
        return N

    def compute(self):
        """-> dict of ``ps`` (7, R, K, 4, 1) float64 as analyze_results
        leaves it (rows C75 C50 Loc Sim Oth BG FN), ``raw`` (5, R, K, 4, 1):
        rows 0-4 before the fill (-1 where a category and area have no
        non-ignored GT), ``aps`` (aps_table), ``rec_thrs`` and ``npig``
        (K, 4).  Images never added count as images without detections."""
        check_one_rank('CocoErrorAnalysis.compute')
        npig = self._npig_all()
        precision, _, _ = self._accumulate(npig, len(self.iou_thrs) + 2)
        raw = precision.cpu().numpy()
        ps = fill(raw)
        return dict(ps=ps, raw=raw, aps=aps_table(ps, self.gt.cat_names),
                    rec_thrs=self.rec_thrs,
                    npig=npig.cpu().numpy().reshape(self.K,
                                                    len(self.area_rng)))


# ------------------------------------------------------ the tool's entry ---
def _results_from_json(anns, gt):
    """COCO.loadRes's rules over a results list -> per image (gt.img_ids
    order) fp32 [x1, y1, x2, y2, score] rows and labels, in file order.  Image
    ids outside the ground truth are refused; a category outside it is not
    scored.  Boxes and scores go to fp32, the detectors' type: exact for the
    files det2json writes, rounded for float64 boxes from elsewhere."""
    if isinstance(anns, (str, os.PathLike)):
        with open(anns) as f:
            anns = json.load(f)
    if len(anns) == 0:
        raise ValueError('coco_error_analysis: the results are empty')
    if 'bbox' not in anns[0]:
        raise ValueError('coco_error_analysis: only bbox results are supported')
    img_index = {i: n for n, i in enumerate(gt.img_ids)}
    bad = {a['image_id'] for a in anns} - set(img_index)
    if bad:
        raise ValueError(f'coco_error_analysis: {len(bad)} result image ids '
                         'are not in the annotation file')
    lab_of = {c: n for n, c in enumerate(gt.cat_ids)}
    img = np.array([img_index[a['image_id']] for a in anns], np.int64)
    bb = np.array([a['bbox'] for a in anns], np.float64).reshape(-1, 4)
    rows = np.stack([bb[:, 0], bb[:, 1], bb[:, 0] + bb[:, 2],
                     bb[:, 1] + bb[:, 3],
                     np.array([a['score'] for a in anns], np.float64)], 1)
    rows = rows.astype(np.float32)
    lab = np.array([lab_of.get(a['category_id'], -1) for a in anns], np.int64)
    order = np.argsort(img, kind='stable')
    cuts = np.searchsorted(img[order], np.arange(len(gt.img_ids) + 1))
    return ([rows[order[cuts[i]:cuts[i + 1]]] for i in range(len(gt.img_ids))],
            [lab[order[cuts[i]:cuts[i + 1]]] for i in range(len(gt.img_ids))])


def _results_from_arrays(results, gt):
    if len(results) != len(gt.img_ids):
        raise ValueError(f'coco_error_analysis: {len(results)} results for '
                         f'{len(gt.img_ids)} images')
    dets, labels = [], []
    for res in results:
        if len(res) != len(gt.cat_ids):
            raise ValueError(f'coco_error_analysis: {len(res)} class arrays, '
                             f'expected {len(gt.cat_ids)}')
        rows = [np.asarray(r, np.float32).reshape(-1, 5) for r in res]
        dets.append(np.concatenate(rows))
        labels.append(np.concatenate(
            [np.full(len(r), c, np.int64) for c, r in enumerate(rows)]))
    return dets, labels


def makeplot(rs, ps, out_dir, class_name, iou_type):
    """The reference's figures: one per area, ``{iou_type}-{class_name}-
    {area}.png``, the types stacked as filled PR curves."""
    from matplotlib.figure import Figure
    cs = np.vstack([np.ones((2, 3)), np.array([.31, .51, .74]),
                    np.array([.75, .31, .30]), np.array([.36, .90, .38]),
                    np.array([.50, .39, .64]), np.array([1, .6, 0])])
    for i, area in enumerate(AREA_NAMES):
        area_ps = ps[..., i, 0]
        figure_tile = f'{iou_type}-{class_name}-{area}'
        aps = [ps_.mean() for ps_ in area_ps]
        ps_curve = [ps_.mean(axis=1) if ps_.ndim > 1 else ps_
                    for ps_ in area_ps]
        ps_curve.insert(0, np.zeros(ps_curve[0].shape))
        fig = Figure()
        ax = fig.add_subplot(111)
        for k in range(len(TYPES)):
            ax.plot(rs, ps_curve[k + 1], color=[0, 0, 0], linewidth=0.5)
            ax.fill_between(rs, ps_curve[k], ps_curve[k + 1], color=cs[k],
                            label=f'[{aps[k]:.3f}]' + TYPES[k])
        ax.set_xlabel('recall')
        ax.set_ylabel('precision')
        ax.set_xlim(0, 1.)
        ax.set_ylim(0, 1.)
        ax.set_title(figure_tile)
        ax.legend()
        fig.savefig(os.path.join(out_dir, f'{figure_tile}.png'))


def coco_error_analysis(results, gt, out_dir=None, types=('bbox', ),
                        device=None, plot=True):
    """analyze_results: ``results`` a COCO results json (path or loaded
    list, COCO.loadRes rules) or ``results[i][c]`` (k, 5) arrays per image
    (``gt.img_ids`` order) and class; ``gt`` a CocoGroundTruth or an
    annotation json (path or dict).  With ``out_dir``, writes
    ``out_dir/bbox/aps.json`` and, when matplotlib imports and ``plot``, the
    reference's PNGs under ``out_dir/bbox/``.  -> CocoErrorAnalysis.compute's
    dict."""
    for t in types:
        if t not in ('bbox', 'segm'):
            raise ValueError(f'coco_error_analysis: unknown result type {t!r}')
        if t != 'bbox':
            raise NotImplementedError(
                f'coco_error_analysis: result type {t!r} is not implemented '
                '(bbox only)')
    if not isinstance(gt, CocoGroundTruth):
        gt = CocoGroundTruth.from_json(gt)
    check_analysable(gt, 'coco_error_analysis')
    is_json = isinstance(results, (str, os.PathLike)) or (
        len(results) > 0 and isinstance(results[0], dict))
    if is_json:
        dets, labels = _results_from_json(results, gt)
    else:
        dets, labels = _results_from_arrays(results, gt)
    ev = CocoErrorAnalysis(gt, device)
    for i in range(0, len(dets), ADD_STEP):
        j = min(len(dets), i + ADD_STEP)
        ev.add(range(i, j), [torch.from_numpy(x) for x in dets[i:j]],
               [torch.from_numpy(x) for x in labels[i:j]])
    out = ev.compute()
    if out_dir is not None:
        res_dir = os.path.join(out_dir, 'bbox')
        os.makedirs(res_dir, exist_ok=True)
        with open(os.path.join(res_dir, 'aps.json'), 'w') as f:
            json.dump(out['aps'], f, indent=1)
        if plot:
            try:
                import matplotlib  # noqa: F401
            except ImportError:
                plot = False
        if plot:
            ps, rs = out['ps'], out['rec_thrs']
            for k, nm in enumerate(gt.cat_names):
                makeplot(rs, ps[:, :, k], res_dir, nm, 'bbox')
            makeplot(rs, ps, res_dir, 'allclass', 'bbox')
    return out
