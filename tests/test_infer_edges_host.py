"""The premises of tests/test_gpu_infer_edges.py, on the CPU: every case of
tests/_infer_exact.py is built, run through the numpy oracle and checked to be
still adversarial -- coordinates integer and scores dyadic (so the device can
be held to bit equality), top-k cuts inside runs of equal scores, the best-4096
window really too small, IoU really equal to the threshold.  These asserts are
conditions on the inputs, not measurements of any kernel."""
import numpy as np
import pytest

import _infer_exact as X

F32 = np.float32

# name -> (builder, extra score values the case may hold)
HALVES = tuple(0.5 * v for v in X.DYADIC)
CASES = {
    'three_paths': (X.three_paths, ()),
    'topk_reference_level': (X.topk_reference_level, ()),
    'topk_4500': (X.topk_4500, ()),
    'window': (X.window, ()),
    'keep_limits': (X.keep_limits, ()),
    'iou_half': (X.iou_half, ()),
    'score_thr_edge': (X.score_thr_edge, (X.SCORE_ABOVE_THR, )),
    'zero_area': (X.zero_area, ()),
    'many_images': (X.many_images, ()),
    'ctr_product_ties': (X.ctr_product_ties, HALVES),
    'fcos_points': (X.fcos_points, ()),
    'nine_anchors': (X.nine_anchors, ()),
    'scaled': (X.scaled, ()),
    'voting': (X.voting, ()),
}
CASES.update({n: ((lambda n=n: X.boundary(n)), ()) for n in X.BOUNDARY_LEVELS})


def _is_int(a):
    return bool(np.all(a == np.round(a)))


@pytest.mark.parametrize('name', list(CASES))
def test_coordinates_are_integers_and_scores_dyadic(name):
    build, extra = CASES[name]
    case = build()
    allowed = np.array(X.DYADIC + tuple(extra), F32)
    for m in case.cls:
        assert np.isin(m, allowed).all()
    for pre in case.pre_nms():
        assert _is_int(pre[0]) and pre[0].min() >= 0
        if len(pre) > 2:
            assert np.isin(pre[2], [F32(0.5), F32(1)]).all()
    for dets, labels in case.oracle():
        assert np.isin(dets[:, 4], allowed).all()
        assert np.all(np.diff(dets[:, 4]) <= 0)
        if not case.voting:  # voted boxes are weighted means
            assert _is_int(dets[:, :4])


def _cut(case, l, n, A):
    """(sorted keys, stable order, k) of a level the top-k cuts."""
    key = case.level_keys(l, n)
    assert key.shape == (A, )
    order = np.argsort(-key, kind='stable')
    return key, order, case.settings['nms_pre']


def _assert_cut_inside_tie_run(case, l, n, A):
    key, order, k = _cut(case, l, n, A)
    assert A > k
    kth = key[order[k - 1]]
    assert key[order[k]] == kth, 'the cut does not split a run of equal keys'
    run = np.nonzero(key == kth)[0].astype(np.uint32)
    # the run differs in every index byte the level uses
    nbytes = max(1, (int(A - 1).bit_length() + 7) // 8)
    for b in range(nbytes):
        vals = np.unique((run >> np.uint32(8 * b)) & np.uint32(0xFF))
        assert len(vals) > 1, f'byte {b} is constant inside the tie run'
    if A >= 4096:  # a long run: the low byte takes every value
        assert len(np.unique(run & np.uint32(0xFF))) == 256
    return int((key > kth).sum()), len(run)


CUT_LEVELS = [('topk_reference_level', 0, 0, 4608), ('topk_4500', 0, 0, 4608),
              ('three_paths', 0, 0, 4608), ('three_paths', 0, 1, 4608),
              ('three_paths', 1, 0, 1152), ('three_paths', 1, 1, 1152),
              ('A_eq_k_plus_1', 0, 0, 1152), ('A_4096', 0, 0, 4096),
              ('A_4097', 0, 0, 4097), ('A_4608_long_run', 0, 0, 4608),
              ('ctr_product_ties', 0, 0, 256),
              ('ctr_product_ties', 0, 1, 256), ('fcos_points', 0, 0, 256),
              ('fcos_points', 0, 1, 256), ('scaled', 0, 0, 256),
              ('scaled', 0, 1, 256), ('nine_anchors', 0, 0, 576)]


@pytest.mark.parametrize('name,l,n,A', CUT_LEVELS)
def test_kth_key_lies_inside_a_tie_run(name, l, n, A):
    _assert_cut_inside_tie_run(CASES[name][0](), l, n, A)


def test_three_paths_tie_patterns_differ_per_image():
    case = X.three_paths()
    for l in range(len(case.cls)):
        assert not np.array_equal(case.cls[l][0], case.cls[l][1])
    # unsorted levels too (A <= nms_pre): 288 + 72 + 20 rows are passed through
    assert [m.shape[2] * m.shape[3] for m in case.cls] == \
        [4608, 1152, 288, 72, 20]
    assert case.pre_nms()[0][0].shape[0] == 1000 + 1000 + 288 + 72 + 20


def test_topk_reference_level_closed_form():
    """One 72x64 level, three score values, nms_pre 1000: the cut takes a part
    of the middle value's run, and the oracle's detections are the closed form
    argsort(-score, stable)[:1000] of the cell boxes (nothing overlaps)."""
    case = X.topk_reference_level()
    key, order, k = _cut(case, 0, 0, 4608)
    vals, counts = np.unique(key, return_counts=True)
    assert len(vals) == 3
    above, run = _assert_cut_inside_tie_run(case, 0, 0, 4608)
    assert above == counts[2] and run == counts[1]
    assert 0 < k - above < run  # strictly inside the middle run
    top = order[:k]
    dets, labels = case.oracle()[0]
    x, y = (top % 64).astype(F32) * 8, (top // 64).astype(F32) * 8
    want = np.stack([x, y, x + 8, y + 8, key[top]], 1).astype(F32)
    assert np.array_equal(dets, want)
    rows = case.cls[0][0].reshape(3, -1).T
    assert np.array_equal(labels, rows[top].argmax(1))


def test_boundary_levels_have_the_sizes_named():
    for name, A in (('A_eq_k', 1152), ('A_eq_k_plus_1', 1152),
                    ('A_4096', 4096), ('A_4097', 4097)):
        case = X.boundary(name)
        assert case.level_keys(0).shape == (A, )
    # the keys at or above the k-th score outnumber the 4096-wide LDS sort
    above, run = _assert_cut_inside_tie_run(X.boundary('A_4608_long_run'),
                                            0, 0, 4608)
    assert above + run > 4096 and above < 1000
    assert X.boundary('A_eq_k').settings['nms_pre'] == 1152
    assert X.boundary('A_eq_k_plus_1').settings['nms_pre'] + 1 == 1152
    assert X.topk_4500().settings['nms_pre'] > 4096


def test_window_runs_out_in_production_form():
    """More than 4096 candidates, the window's edge inside a tie run, fewer
    keeps than max_per_img, and fewer still when only the best 4096 are
    offered: a fallback that did not run, or ran on a mis-sorted list, changes
    the count."""
    import ld_oracle as O
    case = X.window()
    s, boxes, labels = case.candidates()
    assert len(s) == 2 * 4608 > 4096
    assert s[4095] == s[4096]
    run = np.nonzero(s == s[4095])[0]
    assert run[0] < 4095 and run[-1] > 4096
    full, full_labels = case.oracle()[0]
    assert full.shape[0] < case.settings['max_per_img'] == 1024
    # one keep per (group, class) pair
    assert full.shape[0] == 2 * (72 * 64 // 16)
    C = case.cls[0].shape[1]
    sc = np.zeros((4096, C), F32)
    sc[np.arange(4096), labels[:4096]] = s[:4096]
    best, _ = O.multiclass_nms(boxes[:4096], sc, 0.05, 0.6, 1024)
    assert 100 < best.shape[0] < full.shape[0]
    # the fast path suffices at max_per_img 100, and gives the same prefix
    d100, l100 = case.oracle(max_per_img=100)[0]
    assert d100.shape[0] == 100
    assert np.array_equal(d100, full[:100]) and \
        np.array_equal(d100, best[:100])
    print('window: keeps', full.shape[0], 'from all', len(s),
          'candidates,', best.shape[0], 'from the best 4096')


def test_iou_equal_to_the_threshold():
    case = X.iou_half()
    both, labels = case.oracle(iou_thr=0.5)[0]
    assert np.array_equal(both[:, :4], np.array(
        [[0, 0, 16, 16], [0, 0, 16, 8]], F32))
    assert labels.tolist() == [1, 1]  # not label 0: the class shift is in play
    assert F32(X.IOU_THR_BELOW_HALF) < F32(0.5)
    one, _ = case.oracle(iou_thr=X.IOU_THR_BELOW_HALF)[0]
    assert np.array_equal(one, both[:1])


def test_score_equal_to_the_threshold():
    case = X.score_thr_edge()
    assert case.settings['score_thr'] == 0.25
    flat = case.cls[0].reshape(-1)
    assert (flat == F32(0.25)).sum() == 3
    assert (flat == F32(X.SCORE_ABOVE_THR)).sum() == 3
    assert F32(X.SCORE_ABOVE_THR) > F32(0.25)
    dets, _ = case.oracle()[0]
    assert dets.shape[0] == int((flat > F32(0.25)).sum()) == 5
    assert (dets[:, 4] == F32(X.SCORE_ABOVE_THR)).sum() == 3


def test_zero_area_boxes_are_kept():
    dets, labels = X.zero_area().oracle()[0]
    area = (dets[:, 2] - dets[:, 0]) * (dets[:, 3] - dets[:, 1])
    assert dets.shape[0] == 5 and (area == 0).sum() == 4
    # two identical zero-area boxes of one class: 0 / 0, nothing suppressed
    same = [(i, j) for i in range(5) for j in range(i + 1, 5)
            if labels[i] == labels[j] and area[i] == 0 and area[j] == 0 and
            np.array_equal(dets[i, :4], dets[j, :4])]
    assert same


def test_many_images_counts():
    case = X.many_images()
    res = case.oracle()
    assert len(res) == 65 > 64
    counts = [d.shape[0] for d, _ in res]
    assert counts == [X.many_images_count(n) for n in range(65)]
    assert counts[0] == 0 and counts[8] == 56 and counts[9] == 0
    # the images differ: every non-empty one has its own detections
    assert len({d.tobytes() for d, _ in res}) == 1 + sum(c > 0 for c in counts)


def test_keep_limits_premise():
    case = X.keep_limits()
    s, _, _ = case.candidates()
    assert len(s) >= 1100
    full, _ = case.oracle(max_per_img=1024)[0]
    assert full.shape[0] == 1024
    # ties straddle the 256-wide NMS chunks and every keep limit used
    for edge in (255, 256, 257, 511, 512, 767, 768):
        assert s[edge - 1] == s[edge] or s[edge] == s[edge + 1]


def test_centerness_product_ties():
    case = X.ctr_product_ties()
    thr = F32(X.CTR_SCORE_THR)
    for n in range(2):
        pre = case.pre_nms()[n]
        sc, fac = pre[1].max(1), pre[2]
        prod = (sc * fac).astype(F32)
        # equal products from different (score, factor) pairs, both selected
        assert ((prod == F32(0.5)) & (fac == F32(0.5))).any()
        assert ((prod == F32(0.5)) & (fac == F32(1))).any()
        # score above the threshold, product below: still a detection
        assert ((sc > thr) & (prod < thr)).any()
        dets, _ = case.oracle()[n]
        assert (dets[:, 4] < thr).any()
        assert dets.shape[0] == int((pre[1] > thr).sum())


def test_nine_anchor_ties_inside_a_cell():
    case = X.nine_anchors()
    key = case.level_keys(0).reshape(64, 9)
    live = key > 0
    assert (live.sum(1) >= 8).all() and not live.all()
    assert all(len(np.unique(k[m])) == 1 for k, m in zip(key, live))
    # base anchors of one cell with one label (suppressed duplicates) and with
    # different labels (all kept)
    lab = case.cls[0][0].reshape(9, 3, 64).argmax(1).T
    assert any(len(set(r)) < len(r) for r in lab.tolist())
    dets, _ = case.oracle()[0]
    assert 0 < dets.shape[0] < case.settings['nms_pre']


def test_scaled_and_points_geometry():
    res = X.scaled().oracle()
    assert res[0][0][:, :4].max() > 128 and res[1][0][:, :4].max() <= 64
    d = X.fcos_points().oracle()[0][0]
    assert np.all(d[:, :2] % 8 == 4)  # centres (x, y) * 8 + 4, bins 0 / 1


def test_voting_premise():
    case = X.voting()
    s, _, _ = case.candidates()
    assert len(s) == 2 * 36 * 32  # dense matrix: 2304^2 fp32, about 20 MB
    dets, labels = case.oracle()[0]
    assert dets.shape[0] == 100 and set(labels.tolist()) == {0, 1}


def test_aug_views_duplicate_each_other():
    import ld_oracle as O
    views, boxes, scores = X.aug_views()
    K = views[0]['boxes'].shape[0]
    assert _is_int(boxes) and np.array_equal(boxes[:K], boxes[K:])
    assert not np.array_equal(views[0]['boxes'], views[1]['boxes'])
    for v in views:
        assert np.log2(v['scale_factor']).tolist() == \
            np.round(np.log2(v['scale_factor'])).tolist()
    s = X.AUG_SETTINGS
    dets, labels = O.multiclass_nms(boxes, scores, s['score_thr'],
                                    s['iou_thr'], s['max_per_img'])
    # view 0's row wins every tie with its duplicate in view 1; the rows of
    # view 1 that moved to another class survive
    moved = int(X.aug_moved(K).sum())
    assert 0 < moved < K and dets.shape[0] == K + moved < s['max_per_img']
    first, fl = O.multiclass_nms(boxes[:K], scores[:K], s['score_thr'],
                                 s['iou_thr'], s['max_per_img'])
    # ... behind every view-0 row of their score (view-major tie order)
    for v in np.unique(dets[:, 4]):
        run = dets[:, 4] == v
        n0 = int((first[:, 4] == v).sum())
        assert np.array_equal(dets[run][:n0], first[first[:, 4] == v])
        assert np.array_equal(labels[run][:n0], fl[first[:, 4] == v])
