"""CPU-side checks of the proposal recall: the golden fixture
(tests/golden/recall.npz, tools/gen_golden_recall.py), the argument handling
and refusals of ld_amd.recall, its summary table and plots, the numpy
restatement of COCOeval's useCats = 0 path (tests/_proposal_oracle.py) against
hand-derived known answers, and the C ABI's declarations and host-side
validation."""
import ctypes
import logging
import os
import re
import sys

import numpy as np
import pytest

from ld_amd import synthetic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cocoeval_oracle as O  # noqa: E402
import _proposal_oracle as PO  # noqa: E402

GOLD = os.path.join(REPO, 'tests', 'golden', 'recall.npz')


def _lib():
    from ld_amd import lib as L
    if not L.lib_available():
        import __graft_entry__
        __graft_entry__.build()
    return L, L.get_lib()


# ------------------------------------------------------------------ golden ---
def test_golden_loads_and_is_interior():
    gold = np.load(GOLD)
    runs = synthetic.recall_cases()
    assert {r[0] for r in runs} == {
        'mixed', 'unsorted_nums', 'ties', 'noscore', 'equal',
        'equal_int_float', 'equal_none', 'big', 'nogt'}
    for tag, gts, props, nums, thrs, whole, interior in runs:
        rec, table = gold[f'{tag}_recalls'], gold[f'{tag}_gt_ious']
        assert rec.dtype == np.float64 and table.dtype == np.float32
        P = len(np.atleast_1d(nums))
        T = 1 if thrs is None else len(np.atleast_1d(thrs))
        total = sum(0 if g is None else len(g) for g in gts)
        assert rec.shape == (P, T) and table.shape == (P, total)
        for p, g in zip(props, gts):  # pairwise distinct scores
            if p.shape[1] == 5:
                assert len(np.unique(p[:, 4])) == len(p)
        if interior:
            assert synthetic.recall_is_interior(rec), tag
    assert np.isnan(gold['nogt_recalls']).all()
    # the edges the cases exist for
    assert (gold['mixed_gt_ious'] == -1).any()      # proposals used up
    assert (gold['ties_gt_ious'] == 1).any()        # a proposal equal to a GT
    assert (gold['ties_gt_ious'] == 0).any()        # a GT nothing overlaps
    by = {c[0]: c for c in synthetic.RECALL_CASES}
    assert max(by['big'][3]) > 1024 and max(by['big'][2]) * 1000 > 12288


def test_recall_is_interior_rule():
    assert not synthetic.recall_is_interior(np.zeros((3, 10)))
    assert not synthetic.recall_is_interior(np.ones((3, 10)))
    assert synthetic.recall_is_interior([[0.5]])
    assert not synthetic.recall_is_interior([[0.5, 0.25, 1.0, 0.0]])


# ------------------------------------------------------------- python side ---
def test_set_recall_param():
    from ld_amd.recall import set_recall_param
    n, t = set_recall_param(100, None)
    assert n.tolist() == [100] and t.tolist() == [0.5]
    n, t = set_recall_param((12, 3, 8), 0.75)
    assert n.tolist() == [12, 3, 8] and t.tolist() == [0.75]
    n, t = set_recall_param([5], [0.5, 0.6])
    assert n.tolist() == [5] and t.tolist() == [0.5, 0.6]
    arr, thr = np.array([1, 2]), np.linspace(.5, .95, 10)
    n, t = set_recall_param(arr, thr)
    assert n is arr and t is thr


def test_cpu_is_refused():
    from ld_amd import lib as L
    from ld_amd.recall import RecallAccumulator, eval_recalls
    with pytest.raises(L.LdError, match='no CPU path'):
        RecallAccumulator((5, 10), device='cpu')
    with pytest.raises(L.LdError, match='no CPU path'):
        eval_recalls([np.zeros((1, 4), np.float32)],
                     [np.zeros((1, 5), np.float32)], 5, device='cpu')


def test_bad_arguments():
    from ld_amd.recall import CocoProposalEvaluator, RecallAccumulator
    with pytest.raises(ValueError):
        RecallAccumulator(None, device='cpu')
    with pytest.raises(ValueError):
        RecallAccumulator((5, -1), device='cpu')
    with pytest.raises(ValueError):
        RecallAccumulator(tuple(range(17)), device='cpu')
    with pytest.raises(ValueError):
        RecallAccumulator(5, np.linspace(0, 1, 17), device='cpu')
    from ld_amd.coco_eval import CocoGroundTruth
    gt = CocoGroundTruth([0], [1], ['a'], [], [], np.zeros((0, 4)), [], [],
                         [])
    with pytest.raises(KeyError):
        CocoProposalEvaluator(gt, 'bbox', device='cpu')


def test_check_metrics_still_refuses_proposal():
    from ld_amd import coco_eval as CE
    for m in ('proposal', 'proposal_fast'):
        with pytest.raises(NotImplementedError):
            CE.check_metrics(m)


def test_summary_table_text(caplog):
    from ld_amd.recall import print_recall_summary
    rec = np.array([[0.5, 0.25], [1.0, 0.123456]])
    with caplog.at_level(logging.INFO, logger='ld_amd.recall'):
        text = print_recall_summary(rec, (100, 1000), [0.5, 0.75])
    assert text.splitlines() == ['       0.5  0.75',
                                 ' 100 0.500 0.250',
                                 '1000 1.000 0.123']
    assert text in caplog.text
    caplog.clear()
    with caplog.at_level(logging.INFO, logger='ld_amd.recall'):
        sub = print_recall_summary(rec, (100, 1000), [0.5, 0.75],
                                   row_idxs=np.array([1]),
                                   col_idxs=np.array([0]), logger='silent')
    assert sub.splitlines() == ['       0.5', '1000 1.000']
    assert caplog.text == ''


def test_plots_return_a_figure_under_agg():
    import matplotlib
    from matplotlib.figure import Figure
    from ld_amd.recall import plot_iou_recall, plot_num_recall
    f = plot_num_recall(np.array([0.2, 0.5, 0.9]), np.array([100, 300, 1000]))
    assert isinstance(f, Figure)
    assert matplotlib.get_backend().lower() == 'agg'
    (line, ) = f.axes[0].lines
    assert line.get_xdata().tolist() == [0, 100, 300, 1000]
    assert line.get_ydata().tolist() == [0, 0.2, 0.5, 0.9]
    assert f.axes[0].get_xlim() == (0, 1000)
    g = plot_iou_recall([0.9, 0.5], [0.5, 0.75])
    assert isinstance(g, Figure)
    (line, ) = g.axes[0].lines
    assert line.get_xdata().tolist() == [0.5, 0.75, 1.0]
    assert line.get_ydata().tolist() == [0.9, 0.5, 0.0]
    assert g.axes[0].get_xlim() == (0.5, 1)
    import matplotlib.pyplot as plt
    plt.close(f)
    plt.close(g)


# ------------------------------------------- the useCats = 0 restatement ----
def _ds(gts, img_ids=(0, ), cats=((0, 'car'), )):
    """gts: (image_id, category_id, xywh, area, iscrowd, id) tuples."""
    return dict(
        images=[dict(id=i, width=640, height=640) for i in img_ids],
        categories=[dict(id=c, name=n) for c, n in cats],
        annotations=[dict(image_id=i, category_id=c, bbox=list(b), area=a,
                          iscrowd=cr, id=k) for i, c, b, a, cr, k in gts])


def _arr(rows):
    return np.asarray(rows, np.float32).reshape(-1, 5)


def test_kat_categories_do_not_matter():
    """Each detection sits on the GT of the OTHER category: nothing under
    'bbox', everything under 'proposal'."""
    ds = _ds([(0, 3, (0, 0, 10, 10), 100, 0, 1),
              (0, 7, (100, 100, 50, 50), 2500, 0, 2)],
             cats=((3, 'a'), (7, 'b')))
    res = [[_arr([[100, 100, 150, 150, 0.9]]), _arr([[0, 0, 10, 10, 0.8]])]]
    ev, _, _ = O.evaluate(ds, res)
    assert ev['bbox_mAP'] == 0.0
    ev, ce = PO.evaluate_proposal(ds, res)
    assert list(ev) == PO.PROPOSAL_ITEMS
    assert ev['AR@100'] == ev['AR@300'] == ev['AR@1000'] == 1.0
    assert ev['AR_s@1000'] == 1.0 and ev['AR_m@1000'] == 1.0
    assert ev['AR_l@1000'] == -1.0
    assert ce.eval['recall'].shape == (10, 1, 4, 3)
    # the same boxes as one (k, 5) array per image
    ev2, _ = PO.evaluate_proposal(ds, [np.concatenate(res[0])])
    assert ev2 == ev


def test_kat_budget_and_crowd():
    """The only hit is ranked 150th: outside AR@100, inside AR@300.  A crowd
    GT is not counted, and a hit at IoU 0.72 counts at 5 of 10 thresholds."""
    fps = [[300 + i, 300, 310 + i, 310, 1.0 - 0.001 * i] for i in range(149)]
    ds = _ds([(0, 0, (0, 0, 10, 10), 100, 0, 1),
              (0, 0, (400, 400, 100, 100), 10000, 1, 2)])
    ev, _ = PO.evaluate_proposal(ds, [_arr(fps + [[0, 0, 10, 10, 0.5]])])
    assert ev['AR@100'] == 0.0 and ev['AR@300'] == 1.0
    assert ev['AR@1000'] == 1.0 and ev['AR_s@1000'] == 1.0
    assert ev['AR_m@1000'] == -1.0 and ev['AR_l@1000'] == -1.0
    ev, ce = PO.evaluate_proposal(ds, [_arr([[0, 0, 10, 7.2, 0.9]])],
                                  metric_items=['AR@100', 'mAP_50'])
    assert ev == {'AR@100': 0.5, 'mAP_50': 1.0}
    assert abs(ce.stats[6] - 0.5) < 1e-12
    assert PO.evaluate_proposal(ds, [np.zeros((0, 5), np.float32)]) == \
        ({}, None)


def test_kat_gt_order_is_category_major_in_cat_ids_order():
    """Two equal GTs of different categories and one detection on them: the
    later GT of the cell takes the match (``ious < iou`` does not skip an
    equal IoU), and the cell lists the categories in ``cat_ids`` (file)
    order, not in sorted or annotation order."""
    gts = [(0, 3, (0, 0, 10, 10), 100, 0, 11), (0, 7, (0, 0, 10, 10), 100, 0, 12)]
    det = [_arr([[0, 0, 10, 10, 0.9]])]
    _, ce = PO.evaluate_proposal(_ds(gts, cats=((3, 'a'), (7, 'b'))), det)
    assert ce.evalImgs[0]['gtIds'] == [11, 12]
    assert ce.evalImgs[0]['dtMatches'][0, 0] == 12
    _, ce = PO.evaluate_proposal(_ds(gts, cats=((7, 'b'), (3, 'a'))), det)
    assert ce.evalImgs[0]['gtIds'] == [12, 11]
    assert ce.evalImgs[0]['dtMatches'][0, 0] == 11
    # a GT of a category outside the class list is not in the cell
    _, ce = PO.evaluate_proposal(_ds(gts, cats=((7, 'b'), (3, 'a'))), det,
                                 classes=('a', ))
    assert ce.evalImgs[0]['gtIds'] == [11]


def test_agnostic_view_orders_gts_like_the_restatement():
    from ld_amd import recall as R
    from ld_amd.coco_eval import CocoGroundTruth
    case = {c[0]: c for c in synthetic.COCO_CASES}['base']
    ds, _, classes, _ = synthetic.coco_eval_inputs(case)
    gt = CocoGroundTruth.from_json(ds, classes)
    view = R._agnostic_gt(gt)
    assert view.cat_ids == [1] and view.img_ids == gt.img_ids
    rank = {c: i for i, c in enumerate(gt.cat_ids)}
    for img in gt.img_ids[:10]:
        want = sorted((a for a in ds['annotations'] if a['image_id'] == img),
                      key=lambda a: rank[a['category_id']])
        got = view.ids[view.gt_img_ids == img]
        assert got.tolist() == [a['id'] for a in want]
    fast = R._fast_gt_bboxes(gt)
    assert len(fast) == len(gt.img_ids)
    n_real = sum(1 for a in ds['annotations'] if not a['iscrowd'])
    assert sum(len(b) for b in fast) == n_real
    assert all(b.dtype == np.float32 and b.shape[1] == 4 for b in fast)


# -------------------------------------------------------------------- ABI ----
def test_recall_symbols_declared_and_bound():
    L, _ = _lib()
    src = open(os.path.join(REPO, 'include', 'ld_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(ld_[a-z0-9_]+)\s*\(', src))
    names = {'ld_eval_recalls_workspace_bytes', 'ld_eval_recalls_match',
             'ld_eval_recalls_count'}
    assert names <= declared and names <= set(L.SIGNATURES)
    so = ctypes.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(so, n), n
    assert re.search(r'#define\s+LD_EVAL_RECALLS_MAX_NUMS\s+16\b', src)
    assert re.search(r'#define\s+LD_EVAL_RECALLS_NO_LDS\s+1\b', src)
    assert L.LD_EVAL_RECALLS_MAX_NUMS == 16 and L.LD_EVAL_RECALLS_NO_LDS == 1
    import ld_amd
    for n in ('RecallAccumulator', 'eval_recalls', 'set_recall_param',
              'print_recall_summary', 'plot_num_recall', 'plot_iou_recall',
              'coco_proposal_evaluate', 'CocoProposalEvaluator'):
        assert hasattr(ld_amd, n), n


def test_recall_abi_validates_on_the_host():
    """Malformed arguments are refused before anything reaches the device."""
    L, lib = _lib()
    C = ctypes
    wsb = lib.ld_eval_recalls_workspace_bytes
    assert wsb(-1, 0, 0, 0) == 0 and wsb(10, 10, 10, -1) == 0
    # the tile is num_gts x min(max_img_props, cap) floats
    assert wsb(3000, 140, 1500, 1000) >= 140 * 1000 * 4
    assert wsb(3000, 140, 1500, 1000) < wsb(3000, 140, 1500, 1500)
    vp = lambda a: C.cast(a, C.c_void_p)  # noqa: E731
    nums = (C.c_int32 * 17)(*([5] * 17))
    neg = (C.c_int32 * 2)(5, -1)
    one = (C.c_int32 * 2)(0, 0)
    buf = (C.c_float * 8)()
    m = lib.ld_eval_recalls_match

    def call(cols=5, num_nums=2, pn=nums, flags=0, stride=4, base=0,
             num_gts=1, ws=None, ws_bytes=0, max_k=0):
        return m(vp(buf), cols, vp(one), vp(buf), vp(one), 1, 0, num_gts,
                 max_k, num_nums, vp(pn), flags, vp(buf), stride, base, ws,
                 ws_bytes, None)

    assert call(cols=3) == -1
    assert call(num_nums=0) == -1 and call(num_nums=17) == -1
    assert call(pn=neg) == -1
    assert call(flags=2) == -1
    assert call(max_k=1) == -1            # more than num_props
    assert call(stride=4, base=4) == -1   # the batch does not fit the table
    assert call() == -2                   # no workspace
    assert call(num_gts=0) == 0           # nothing to do
    big = (C.c_char * 4096)()             # a workspace that is not 4-aligned
    odd = C.c_void_p(C.addressof(big) + 1)
    assert call(ws=odd, ws_bytes=4000) == -1
    c = lib.ld_eval_recalls_count
    thr = (C.c_double * 17)(*([0.5] * 17))
    out = (C.c_double * 4)()
    assert c(vp(buf), 8, 8, 0, 1, vp(thr), vp(out), None) == -1
    assert c(vp(buf), 8, 8, 17, 1, vp(thr), vp(out), None) == -1
    assert c(vp(buf), 8, 8, 1, 17, vp(thr), vp(out), None) == -1
    assert c(vp(buf), 4, 8, 1, 1, vp(thr), vp(out), None) == -1
    assert c(None, 8, 8, 1, 1, vp(thr), vp(out), None) == -1
    assert c(vp(buf), 1 << 32, 1 << 31, 1, 1, vp(thr), vp(out), None) == -3
