"""CPU checks of the COCO error analysis: the numpy restatement of the
reference's coco_error_analysis.py (tests/_coco_error_oracle.py) against
hand-derived answers, the module's fill and aps table against it, the
refusals, and the new C entry points' host-side argument checks."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _coco_error_oracle as E  # noqa: E402

from ld_amd import coco_analysis as CA  # noqa: E402
from ld_amd.coco_eval import CocoGroundTruth  # noqa: E402

# categories 1, 2 share supercategory 'S'; 3 is alone in 'T'
CATS = [dict(id=1, name='a', supercategory='S'),
        dict(id=2, name='b', supercategory='S'),
        dict(id=3, name='c', supercategory='T')]
EINVAL, ENOSPACE, EUNSUPPORTED = -1, -2, -3  # include/ld_hip.h
FAR = [300.0, 300.0, 20.0, 20.0]  # an own GT no test detection overlaps


def _ds(anns, cats=CATS, images=(7, )):
    for n, a in enumerate(anns):
        a.setdefault('id', n + 1)
        a.setdefault('image_id', images[0])
        a.setdefault('iscrowd', 0)
        a.setdefault('area', a['bbox'][2] * a['bbox'][3])
    return dict(images=[dict(id=i) for i in images], annotations=anns,
                categories=cats)


def _det(bbox, score, cat=1, img=7):
    return dict(image_id=img, bbox=list(bbox), score=score, category_id=cat)


def _aps(ps, k=0, area=0):
    # rounded: pr = tp / (tp + fp + eps) is one ulp under 1
    return dict(zip(E.TYPES, [round(float(ps[t, :, k, area, 0].mean()), 12)
                              for t in range(7)]))


def _iou_06_box():
    # GT [0, 0, 10, 10], detection [0, 0, 10, 6]: IoU 60 / 100 = .6
    return [0.0, 0.0, 10.0, 10.0], [0.0, 0.0, 10.0, 6.0]


def test_same_supercategory_confusion_is_ignored_in_sim():
    gt_box, det_box = _iou_06_box()
    ds = _ds([dict(bbox=FAR, category_id=1),
              dict(bbox=gt_box, category_id=2)])
    res = [_det(det_box, .9), _det(FAR, .5)]  # FP on the 'b' GT, TP
    ps, _, _ = E.analyze_results(ds, res)
    got = _aps(ps)
    assert got['C75'] == got['C50'] == got['Loc'] == .5
    assert got['Sim'] == got['Oth'] == got['BG'] == got['FN'] == 1.0


def test_other_supercategory_confusion_is_ignored_only_in_oth():
    gt_box, det_box = _iou_06_box()
    ds = _ds([dict(bbox=FAR, category_id=1),
              dict(bbox=gt_box, category_id=3)])
    ps, _, _ = E.analyze_results(ds, [_det(det_box, .9), _det(FAR, .5)])
    got = _aps(ps)
    assert got['C75'] == got['C50'] == got['Loc'] == got['Sim'] == .5
    assert got['Oth'] == got['BG'] == 1.0


def test_poor_localisation_is_a_tp_only_at_loc():
    # IoU([0, 0, 10, 10], [0, 0, 10, 3]) = .3
    ds = _ds([dict(bbox=[0.0, 0.0, 10.0, 10.0], category_id=1)])
    ps, _, _ = E.analyze_results(ds, [_det([0.0, 0.0, 10.0, 3.0], .9)])
    got = _aps(ps)
    assert got['C75'] == got['C50'] == 0.0
    assert got['Loc'] == got['Sim'] == got['Oth'] == 1.0


def test_small_detection_inside_a_large_other_gt_is_ignored_by_ioa():
    big = [0.0, 0.0, 200.0, 200.0]
    small = [50.0, 50.0, 10.0, 10.0]  # IoU 100 / 40000, ioa 1
    ds = _ds([dict(bbox=FAR, category_id=1), dict(bbox=big, category_id=3)])
    ps, _, _ = E.analyze_results(ds, [_det(small, .9), _det(FAR, .5)])
    got = _aps(ps)
    assert got['Loc'] == got['Sim'] == .5
    assert got['Oth'] == 1.0


@pytest.mark.parametrize('relabelled_first, expect', [(True, .5),
                                                      (False, 1.0)])
def test_tie_own_ignored_vs_relabelled_crowd_follows_annotation_order(
        relabelled_first, expect):
    """d1 overlaps the own GT O (IoU .5; json area 2000, so ignored in
    'small') and the 'c' GT R (ioa .5) equally: it takes the later one.  If
    that is O, O is consumed and d2 (inside O only) is a small false
    positive; if it is R, d2 matches O and is ignored."""
    O_ = dict(bbox=[0.0, 0.0, 10.0, 20.0], category_id=1, area=2000.0)
    R = dict(bbox=[5.0, 0.0, 15.0, 10.0], category_id=3)
    S = dict(bbox=FAR, category_id=1, area=100.0)
    anns = [R, O_, S] if relabelled_first else [O_, R, S]
    ds = _ds([dict(a) for a in anns])
    res = [_det([0.0, 0.0, 10.0, 10.0], .9), _det([0.0, 12.0, 8.0, 8.0], .8),
           _det(FAR, .7)]
    ps, _, _ = E.analyze_results(ds, res)
    assert _aps(ps, area=1)['Oth'] == expect  # area 'small'
    assert _aps(ps, area=1)['Sim'] == .5  # R is not relabelled there


def test_category_without_gts_counts_as_zero_and_fill_rows():
    gt_box, det_box = _iou_06_box()
    ds = _ds([dict(bbox=FAR, category_id=1),
              dict(bbox=gt_box, category_id=3)])
    res = [_det(det_box, .9), _det(FAR, .5), _det(FAR, .4, cat=2)]
    ps, raw, _ = E.analyze_results(ds, res)
    assert np.all(raw[:, :, 1] == -1)  # 'b' has no GT
    assert np.all(ps[:6, :, 1] == 0) and np.all(ps[6, :, 1] == 1)
    np.testing.assert_array_equal(ps[5], ps[4] > 0)  # BG
    assert np.all(ps[6] == 1)  # FN
    table = E.aps_table(ps, ['a', 'b', 'c'])
    # 'c' has a GT but no detection: C75 .. Oth 0
    per = [round(table[n]['allarea']['C75'], 12) for n in 'abc']
    assert per == [.5, 0.0, 0.0]
    assert table['allclass']['allarea']['C75'] == pytest.approx(.5 / 3)
    assert table['allclass']['allarea']['FN'] == 1.0


def test_fill_and_table_equal_the_restatement():
    """The module's vectorised fill / aps table equal the reference's loop
    over categories on the same raw rows."""
    gt_box, det_box = _iou_06_box()
    ds = _ds([dict(bbox=FAR, category_id=1), dict(bbox=gt_box, category_id=2),
              dict(bbox=[40.0, 40.0, 90.0, 90.0], category_id=3)])
    res = [_det(det_box, .9), _det(FAR, .5), _det([45.0, 40.0, 90.0, 80.0],
                                                  .6, cat=3),
           _det([0.0, 0.0, 9.0, 9.0], .3, cat=2)]
    ps, raw, _ = E.analyze_results(ds, res)
    mine = CA.fill(raw)
    assert mine.tobytes() == ps.tobytes()
    assert CA.aps_table(mine, ['a', 'b', 'c']) == E.aps_table(ps, 'abc')


def test_refusals():
    ds = _ds([dict(bbox=FAR, category_id=1)])
    gt = CocoGroundTruth.from_json(ds)
    assert gt.supercategories == ['S', 'S', 'T']
    CA.check_analysable(gt)
    unsorted = dict(ds, categories=[CATS[1], CATS[0], CATS[2]])
    with pytest.raises(ValueError, match='ascending'):
        CA.CocoErrorAnalysis(CocoGroundTruth.from_json(unsorted))
    nosup = dict(ds, categories=[dict(id=c['id'], name=c['name'])
                                 for c in CATS])
    gt_nosup = CocoGroundTruth.from_json(nosup)
    assert gt_nosup.supercategories is None
    with pytest.raises(ValueError, match='supercategories'):
        CA.CocoErrorAnalysis(gt_nosup)
    with pytest.raises(NotImplementedError, match='segm'):
        CA.coco_error_analysis([], gt, types=['segm'])
    with pytest.raises(ValueError, match='unknown'):
        CA.coco_error_analysis([], gt, types=['keypoints'])
    with pytest.raises(TypeError):
        CA.CocoErrorAnalysis(ds)
    anns = [dict(bboxes=np.zeros((1, 4), np.float32), labels=np.array([0]))]
    g2 = CocoGroundTruth.from_annotations(anns, num_classes=2,
                                          supercategories=['x', 'y'])
    assert g2.supercategories == ['x', 'y']
    assert CocoGroundTruth.from_annotations(anns).supercategories is None
    with pytest.raises(ValueError, match='one supercategory'):
        CocoGroundTruth.from_annotations(anns, num_classes=2,
                                         supercategories=['x'])


def test_json_results_follow_loadres_rules():
    ds = _ds([dict(bbox=FAR, category_id=1)], images=(7, 9))
    gt = CocoGroundTruth.from_json(ds)
    with pytest.raises(ValueError, match='not in the annotation'):
        CA._results_from_json([_det(FAR, .5, img=8)], gt)
    dets, labels = CA._results_from_json(
        [_det([1.0, 2.0, 3.0, 4.0], .5, img=9), _det(FAR, .25),
         _det(FAR, .75, cat=99, img=9)], gt)
    assert [len(d) for d in dets] == [1, 2]
    np.testing.assert_array_equal(dets[1][0], [1, 2, 4, 6, .5])
    np.testing.assert_array_equal(labels[1], [0, -1])


def test_new_symbols_and_argument_checks():
    from ld_amd import lib as L
    if not L.lib_available():
        import __graft_entry__
        __graft_entry__.build()
    lib = L.get_lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), 'include', 'ld_hip.h')).read()
    for name in ('ld_coco_match_errors', 'ld_coco_match_errors_workspace_bytes'):
        assert name + '(' in src.replace('\n', '')
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert 'ld_coco_err_batch_t' in src
    assert ctypes.sizeof(L.CocoErrBatchT) == 12 * 8 + 8 * 4
    assert lib.ld_coco_match_errors_workspace_bytes(10, 5, 100, 8) > 0
    assert lib.ld_coco_match_errors_workspace_bytes(-1, 5, 100, 8) == 0
    assert lib.ld_coco_match_errors_workspace_bytes(
        10, 5, 100, L.LD_COCO_MAX_CELL_GTS + 1) == 0
    thr = (ctypes.c_double * 3)(.75, .5, .1)
    ar = (ctypes.c_double * 8)(*[0, 1e10] * 4)
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: refused first

    def call(b, T=3, A=4, max_det=100, npig=fake):
        return lib.ld_coco_match_errors(
            ctypes.byref(b), T, ctypes.cast(thr, ctypes.c_void_p), .1, A,
            ctypes.cast(ar, ctypes.c_void_p), max_det, None, None, None, None,
            None, npig, None, 0, None)

    def batch(**kw):
        b = L.CocoErrBatchT()
        b.det_off = b.img_rank = b.gt_img_off = b.cat_sup = fake.value
        b.num_imgs, b.num_all_imgs, b.num_cats = 1, 1, 3
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    assert call(batch(), T=15) == EINVAL  # 17 rows
    assert call(batch(), A=5) == EINVAL
    assert call(batch(), T=0) == EINVAL
    assert call(batch(), max_det=0) == EINVAL
    assert call(batch(), npig=None) == EINVAL
    assert call(batch(num_imgs=0)) == EINVAL
    assert call(batch(cat_sup=None)) == EINVAL
    assert call(batch(num_dets=4)) == EINVAL  # no dets / records
    assert call(batch(num_gts=2)) == EINVAL  # no GT arrays
    assert call(batch(max_img_gts=L.LD_COCO_MAX_CELL_GTS + 1)) == \
        EUNSUPPORTED
    assert call(batch(max_img_gts=4)) == ENOSPACE  # no workspace
