"""CPU checks of the COCO bbox evaluation: the numpy restatement of COCOeval
(tests/_cocoeval_oracle.py) against hand-derived known answers, the golden
file it wrote (tests/golden/coco_eval.npz), the json / annotation loaders of
ld_amd.coco_eval, its refusals, and the new C ABI (declared, exported,
host-side argument validation)."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

from ld_amd import synthetic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _cocoeval_oracle as O  # noqa: E402

GOLD = os.path.join(REPO, 'tests', 'golden', 'coco_eval.npz')


def _ds(gts, img_ids=(0, ), cats=((0, 'car'), )):
    """gts: (image_id, category_id, xywh, area, iscrowd, id) tuples."""
    return dict(
        images=[dict(id=i, width=640, height=640) for i in img_ids],
        categories=[dict(id=c, name=n) for c, n in cats],
        annotations=[dict(image_id=i, category_id=c, bbox=list(b), area=a,
                          iscrowd=cr, id=k) for i, c, b, a, cr, k in gts])


def _res(*per_img):
    return [[np.asarray(r, np.float32).reshape(-1, 5) for r in img]
            for img in per_img]


def test_kat_reference_dataset_test():
    """tests/test_data/test_dataset.py:23-120 of the reference, as data."""
    ds = _ds([(0, 0, (50, 60, 20, 20), 400, 0, 1),
              (0, 0, (100, 120, 30, 30), 900, 0, 2),
              (0, 0, (150, 160, 40, 40), 1600, 0, 3),
              (0, 0, (250, 260, 100, 100), 10000, 0, 4)])
    res = _res([[[50, 60, 70, 80, 1.0], [100, 120, 130, 150, 0.98],
                 [150, 160, 190, 200, 0.96], [250, 260, 350, 360, 0.95]]])
    ev, _, rows = O.evaluate(ds, res, ('car', ), classwise=True)
    assert ev['bbox_mAP'] == ev['bbox_mAP_50'] == ev['bbox_mAP_75'] == 1
    assert rows == [('car', '1.000')]


def test_kat_iou_072():
    ds = _ds([(0, 0, (0, 0, 10, 10), 100, 0, 1)])
    ev, ce, _ = O.evaluate(ds, _res([[[0, 0, 10, 7.2, 0.9]]]))
    assert abs(ce.stats[0] - 0.5) < 1e-12
    assert ev['bbox_mAP'] == 0.5 and ev['bbox_mAP_50'] == 1.0
    assert ev['bbox_mAP_75'] == 0.0
    assert ev['bbox_mAP_s'] == 0.5 and ev['bbox_mAP_m'] == -1.0


def test_kat_crowd_ignores_a_detection():
    real = (0, 0, (0, 0, 10, 10), 100, 0, 1)
    crowd = (0, 0, (100, 100, 50, 50), 2500, 1, 2)
    dets = _res([[[110, 110, 120, 120, 0.9], [0, 0, 10, 10, 0.8]]])
    ev, _, _ = O.evaluate(_ds([real, crowd]), dets)
    assert ev['bbox_mAP'] == 1.0  # the top detection sits in the crowd box
    ev, _, _ = O.evaluate(_ds([real]), dets)
    assert ev['bbox_mAP'] == 0.5  # without it, an FP ranked first


def test_kat_json_area_decides_the_range():
    """Box area 1200 would be 'medium'; the json area 900 makes it 'small'."""
    ds = _ds([(0, 0, (0, 0, 40, 30), 900, 0, 1)])
    ev, ce, _ = O.evaluate(ds, _res([[[0, 0, 40, 30, 0.9]]]))
    assert ev['bbox_mAP_s'] == 1.0
    assert ev['bbox_mAP_m'] == -1.0 and ev['bbox_mAP_l'] == -1.0
    assert O.npig(ce).tolist() == [[1, 1, 0, 0]]


def test_kat_stats0_reads_max_dets_100():
    """The only TP is ranked 150th of its image: inside maxDets[2] = 1000,
    outside the 100 that stats[0] (``_summarize(1)``) reads."""
    fps = [[300 + i, 300, 310 + i, 310, 1.0 - 0.001 * i] for i in range(149)]
    dets = _res([fps + [[0, 0, 10, 10, 0.5]]])
    ev, ce, _ = O.evaluate(_ds([(0, 0, (0, 0, 10, 10), 100, 0, 1)]), dets)
    assert ce.stats[0] == 0.0 and ev['bbox_mAP'] == 0.0
    assert abs(ce.stats[1] - 1 / 150) < 1e-12  # AP50 at maxDets 1000
    assert ev['bbox_mAP_50'] == 0.007
    ev, ce, _ = O.evaluate(_ds([(0, 0, (0, 0, 10, 10), 100, 0, 1)]), dets,
                           proposal_nums=(1, 10, 50))
    assert ce.stats[0] == -1  # no maxDets == 100 at all


def test_kat_annotation_id_0_reads_unmatched():
    dets = _res([[[0, 0, 10, 10, 0.9]]])
    ev, ce, _ = O.evaluate(_ds([(0, 0, (0, 0, 10, 10), 100, 0, 5)]), dets)
    assert ev['bbox_mAP'] == 1.0
    ev, ce, _ = O.evaluate(_ds([(0, 0, (0, 0, 10, 10), 100, 0, 0)]), dets)
    assert ev['bbox_mAP'] == 0.0  # dtm == 0: a false positive
    match, ign, kept = O.match_bits(ce, 1)
    assert kept.all() and match[0] == 0
    # unmatched (dtm == 0) and out of 'medium' / 'large': ignored there only
    want = sum(1 << (t * 4 + a) for t in range(10) for a in (2, 3))
    assert int(ign[0]) == want


def test_kat_ignore_key_is_overwritten_by_iscrowd():
    ds = _ds([(0, 0, (0, 0, 10, 10), 100, 0, 1)])
    ds['annotations'][0]['ignore'] = 1
    ev, _, _ = O.evaluate(ds, _res([[[0, 0, 10, 10, 0.9]]]))
    assert ev['bbox_mAP'] == 1.0


def test_kat_empty_results():
    ds = _ds([(0, 0, (0, 0, 10, 10), 100, 0, 1)])
    ev, ce, _ = O.evaluate(ds, _res([[]]))
    assert ev == {} and ce is None


def test_restatement_reproduces_golden():
    gold = np.load(GOLD)
    for case in synthetic.COCO_CASES:
        name = case[0]
        ds, res, classes, kw = synthetic.coco_eval_inputs(case)
        ev, ce, rows = O.evaluate(ds, res, classes, classwise=True, **kw)
        assert json.dumps(ev) == str(gold[f'{name}_eval'])
        assert json.dumps(rows) == str(gold[f'{name}_classwise'])
        for k in ('precision', 'recall', 'scores'):
            assert ce.eval[k].tobytes() == gold[f'{name}_{k}'].tobytes()
        np.testing.assert_array_equal(O.npig(ce), gold[f'{name}_npig'])


def test_golden_covers_the_edges():
    gold = np.load(GOLD)
    # category id 4 (K index 1 of sorted ids 2, 4, 9) has no GTs
    assert (gold['ties_npig'][1] == 0).all()
    assert (gold['ties_precision'][:, :, 1] == -1).all()
    assert (~gold['maxdet_kept']).any()  # cells truncated at maxDets[-1]
    assert gold['maxdet_stats'][0] == -1  # maxDets (3, 8, 12): no 100
    assert gold['thrs_precision'].shape[0] == 3
    ds, res, _, _ = synthetic.coco_eval_inputs(synthetic.COCO_CASES[1])
    assert any(a['id'] == 0 for a in ds['annotations'])
    assert any(a['iscrowd'] for a in ds['annotations'])


def test_from_json_orderings(tmp_path):
    from ld_amd import coco_eval as CE
    ds = _ds([(7, 5, (0, 0, 4, 4), 16, 0, 3), (3, 2, (1, 1, 4, 4), 16, 1, 1),
              (7, 2, (2, 2, 4, 4), 16, 0, 2), (7, 5, (3, 3, 4, 4), 9, 0, 4),
              (3, 9, (0, 0, 1, 1), 1, 0, 5)],
             img_ids=(7, 3, 11), cats=((5, 'b'), (2, 'a'), (9, 'c')))
    f = tmp_path / 'a.json'
    f.write_text(json.dumps(ds))
    gt = CE.CocoGroundTruth.from_json(str(f))
    assert gt.img_ids == [7, 3, 11] and gt.cat_ids == [5, 2, 9]
    assert gt.sorted_img_ids.tolist() == [3, 7, 11]
    assert gt.sorted_cat_ids.tolist() == [2, 5, 9]
    gt = CE.CocoGroundTruth.from_json(str(f), classes=('c', 'b'))
    assert gt.cat_ids == [5, 9] and gt.cat_names == ['b', 'c']
    idx, off = gt._cells()
    # cells (image rank, category index): (3, 9) -> 1; (7, 5) -> 3, 4
    assert gt.ids[idx].tolist() == [5, 3, 4]
    assert off.tolist() == [0, 0, 1, 3, 3, 3, 3]
    assert gt.areas[idx].tolist() == [1.0, 16.0, 9.0]


def test_from_annotations():
    from ld_amd import coco_eval as CE
    anns = [dict(bboxes=np.array([[0, 0, 10, 5]], np.float32),
                 labels=np.array([1]),
                 bboxes_ignore=np.array([[1, 1, 3, 3]], np.float32),
                 labels_ignore=np.array([0])),
            dict(bboxes=np.zeros((0, 4), np.float32), labels=np.zeros(0))]
    gt = CE.CocoGroundTruth.from_annotations(anns)
    assert gt.img_ids == [0, 1] and gt.cat_ids == [0, 1]
    assert gt.ids.tolist() == [1, 2] and gt.iscrowd.tolist() == [0, 1]
    assert gt.boxes.tolist() == [[0, 0, 10, 5], [1, 1, 2, 2]]
    assert gt.areas.tolist() == [50.0, 4.0]


def test_refusals():
    from ld_amd import coco_eval as CE
    from ld_amd.lib import LdError
    gt = CE.CocoGroundTruth.from_annotations(
        [dict(bboxes=np.zeros((0, 4)), labels=np.zeros(0))], num_classes=2)
    with pytest.raises(ValueError):
        CE.CocoEvaluator(gt, iou_thrs=[0.5] * 17, device='cuda:0')
    with pytest.raises(ValueError):
        CE.CocoEvaluator(gt, proposal_nums=(10, 100), device='cuda:0')
    with pytest.raises(LdError, match='no CPU path'):
        CE.CocoEvaluator(gt, device='cpu')
    with pytest.raises(LdError, match='no CPU path'):
        gt.to('cpu')
    for m in ('segm', 'proposal', 'proposal_fast', ['bbox', 'segm']):
        with pytest.raises(NotImplementedError):
            CE.check_metrics(m)
    with pytest.raises(KeyError):
        CE.check_metrics('mAP')
    assert CE.check_metrics('bbox', 'mAP') == (['bbox'], ['mAP'])
    with pytest.raises(ValueError):
        CE.coco_evaluate([], gt)
    import ld_amd
    assert ld_amd.CocoEvaluator is CE.CocoEvaluator
    assert ld_amd.coco_evaluate is CE.coco_evaluate


def test_summarize_matches_restatement():
    from ld_amd import coco_eval as CE
    gold = np.load(GOLD)
    for name, md, thrs in (('base', [100, 300, 1000], None),
                           ('maxdet', [3, 8, 12], None),
                           ('thrs', [100, 300, 1000], [0.5, 0.75, 0.6])):
        thrs = CE.default_iou_thrs() if thrs is None else np.asarray(thrs)
        st = CE.summarize(gold[f'{name}_precision'], gold[f'{name}_recall'],
                          thrs, md)
        assert st.tobytes() == gold[f'{name}_stats'].tobytes()


def _lib():
    from ld_amd import lib as L
    if not L.lib_available():
        import __graft_entry__
        __graft_entry__.build()
    return L, L.get_lib()


def test_coco_symbols_declared_and_exported():
    L, _ = _lib()
    src = open(os.path.join(REPO, 'include', 'ld_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(ld_[a-z0-9_]+)\s*\(', src))
    names = {'ld_coco_match', 'ld_coco_match_workspace_bytes',
             'ld_coco_accumulate', 'ld_coco_accumulate_workspace_bytes'}
    assert names <= declared and names <= set(L.SIGNATURES)
    so = ctypes.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(so, n), n
    assert ctypes.sizeof(L.CocoBatchT) == 10 * 8 + 8 * 4


def test_coco_abi_validates_on_the_host():
    """Malformed arguments are refused before anything reaches the device."""
    L, lib = _lib()
    C = ctypes
    assert lib.ld_coco_match_workspace_bytes(-1, 0, 100, 0) == 0
    assert lib.ld_coco_match_workspace_bytes(10, 10, 0, 0) == 0
    assert lib.ld_coco_match_workspace_bytes(10, 10, 100, 1025) == 0
    small = lib.ld_coco_match_workspace_bytes(1000, 100, 100, 10)
    big = lib.ld_coco_match_workspace_bytes(1000, 1000, 1000, 200)
    assert 0 < small < big and big >= 16 * 1000 * 200 * 8
    assert lib.ld_coco_accumulate_workspace_bytes(10, 0, 10, 4, 3) == 0
    assert lib.ld_coco_accumulate_workspace_bytes(10, 3, 17, 4, 3) == 0
    assert lib.ld_coco_accumulate_workspace_bytes(10, 3, 10, 5, 3) == 0
    assert lib.ld_coco_accumulate_workspace_bytes(10, 3, 10, 4, 5) == 0
    assert lib.ld_coco_accumulate_workspace_bytes(1 << 20, 80, 10, 4, 3) > \
        (1 << 20) * 32
    thr = (C.c_double * 17)(*([0.5] * 17))
    ar = (C.c_double * 10)(*([0.0, 1e10] * 5))
    vp = lambda a: C.cast(a, C.c_void_p)  # noqa: E731
    one = C.c_int32(0)
    b = L.CocoBatchT()
    b.num_imgs, b.num_all_imgs, b.num_cats = 1, 1, 1
    b.det_off = b.img_rank = b.gt_cell_off = C.addressof(one)
    m = lib.ld_coco_match
    args = [None] * 7 + [0, None]
    assert m(None, 10, vp(thr), 4, vp(ar), 100, *args) == -1
    assert m(C.byref(b), 17, vp(thr), 4, vp(ar), 100, *args) == -1
    assert m(C.byref(b), 10, vp(thr), 5, vp(ar), 100, *args) == -1
    assert m(C.byref(b), 16, vp(thr), 5, vp(ar), 100, *args) == -1  # T*A > 64
    assert m(C.byref(b), 10, vp(thr), 4, vp(ar), 0, *args) == -1
    npig = C.c_int32(0)
    args = [None] * 5 + [C.addressof(npig), None, 0, None]
    b.max_cell_gts = 1025
    assert m(C.byref(b), 10, vp(thr), 4, vp(ar), 100, *args) == -3
    b.max_cell_gts, b.max_img_dets, b.num_dets = 300, 1000, 5
    assert m(C.byref(b), 10, vp(thr), 4, vp(ar), 100, *args) == -1  # no dets
    b.num_dets = 0
    assert m(C.byref(b), 10, vp(thr), 4, vp(ar), 100, *args) == -2  # no ws
    acc = lib.ld_coco_accumulate
    rec = (C.c_double * 3)(0.0, 0.5, 1.0)
    bad_rec = (C.c_double * 3)(0.0, 1.0, 0.5)
    md = (C.c_int32 * 3)(100, 300, 1000)
    bad_md = (C.c_int32 * 3)(300, 100, 1000)
    out = C.c_double(0)
    o = C.addressof(out)
    tail = [C.addressof(npig), o, o, o, None, 0, None]
    assert acc(0, None, None, None, None, None, 1, 1, 10, 4, 3, vp(md), 3,
               vp(rec), *tail) == -2  # no workspace
    assert acc(0, None, None, None, None, None, 1, 1, 10, 4, 3, vp(bad_md), 3,
               vp(rec), *tail) == -1
    assert acc(0, None, None, None, None, None, 1, 1, 10, 4, 3, vp(md), 3,
               vp(bad_rec), *tail) == -1
    assert acc(0, None, None, None, None, None, 1, 1, 10, 4, 3, vp(md), 129,
               vp(rec), *tail) == -1
    assert acc(5, None, None, None, None, None, 1, 1, 10, 4, 3, vp(md), 3,
               vp(rec), *tail) == -1  # records without pointers
