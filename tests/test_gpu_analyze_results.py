"""GPU parity (-m gpu) of the per-image mAP ranking (eval_image.hip:
ld_eval_image_map / ld_draw_boxes, eval.hip: ld_rank_images) through
ld_amd.analyze_results, against
 (1) the REFERENCE's bbox_map_eval outputs (tests/golden/analyze_results.npz),
 (2) this repository's eval_map run on one image at a time,
 (3) the numpy restatement (tests/_imagemap_oracle.py) where the fixture does
     not reach (more than 128 recall steps / classes with GTs).
Bars: ap, has_gt and map bit-exact (assert_array_equal); rankings and painted
images exact."""
import os
import sys

import numpy as np
import pytest
import torch

from ld_amd import synthetic

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _imagemap_oracle as IO  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden', 'analyze_results.npz')
CASES = synthetic.image_map_cases()
IDS = [c[0] for c in CASES]


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def _analyze(results, anns, C, no_lds=False, chunk=None):
    from ld_amd import analyze_results as A
    acc = A.ImageMapAnalyzer(C)
    acc._no_lds = no_lds
    step = chunk or max(len(results), 1)
    for i in range(0, len(results), step):
        acc.add_results(results[i:i + step], anns[i:i + step])
    return acc


def _host(acc):
    m, ap = acc.compute()
    return m.cpu().numpy(), ap.cpu().numpy(), acc.has_gt().cpu().numpy()


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_image_map_vs_reference_golden(gold, case):
    name = case[0]
    results, anns, C = synthetic.image_map_inputs(case)
    m, ap, has_gt = _host(_analyze(results, anns, C))
    assert m.dtype == np.float64 and ap.dtype == np.float32
    assert has_gt.dtype == np.uint8
    assert gold[f'{name}_valid'].all()  # no cell is excluded for ties
    np.testing.assert_array_equal(ap, gold[f'{name}_ap'])
    np.testing.assert_array_equal(has_gt, gold[f'{name}_has_gt'])
    np.testing.assert_array_equal(m, gold[f'{name}_map'])


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_batches_and_forms_agree(case):
    """add in one batch == several batches == add_results == device lists."""
    from ld_amd import analyze_results as A
    results, anns, C = synthetic.image_map_inputs(case)
    one = _host(_analyze(results, anns, C))
    for chunk in (1, 7):
        many = _host(_analyze(results, anns, C, chunk=chunk))
        for a, b in zip(one, many):
            assert a.tobytes() == b.tobytes()
    dev = torch.device('cuda:0')
    lists = A._results_to_lists(results, anns, C)
    acc = A.ImageMapAnalyzer(C, device=dev)
    acc.add(*[[torch.from_numpy(x).to(dev) for x in col] for col in lists])
    assert len(acc) == len(results)
    for a, b in zip(one, _host(acc)):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_topk_vs_reference_golden(gold, case):
    name = case[0]
    results, anns, C = synthetic.image_map_inputs(case)
    acc = _analyze(results, anns, C)
    n = len(results)
    for tag, k in (('3', 3), ('all', n)):
        good, bad = acc.topk(k)
        assert [i for i, _ in good] == gold[f'{name}_good{tag}'].tolist()
        assert [i for i, _ in bad] == gold[f'{name}_bad{tag}'].tolist()
        for i, v in good + bad:
            assert isinstance(i, int) and v == gold[f'{name}_map'][i]
    good, bad = acc.topk(n)
    assert len(good) == len(bad) == n // 2


def test_rank_images_is_stable():
    """Few distinct values, -0.0 among the zeros: equal scores keep index
    order, as sorted() on the reference's dict items does."""
    from ld_amd import analyze_results as A
    rng = np.random.RandomState(1)
    # 4096 is one tile of the sort: one tile exactly, one over, two tiles
    for n in (1, 2, 255, 4095, 4096, 4097, 5000, 8192, 8193, 9000):
        s = rng.randint(0, 7, size=n) / 6.0
        s[::5] = -0.0
        order, out = A.rank_images(torch.from_numpy(s).cuda())
        want = np.argsort(s, kind='stable')
        np.testing.assert_array_equal(order.cpu().numpy(), want)
        np.testing.assert_array_equal(out.cpu().numpy(), s[want])


@pytest.mark.parametrize('name', ['base', 'ignore', 'crowd'])
def test_per_image_path_equals_eval_map_of_one_image(name):
    """map[i] is eval_map of this repository on image i alone at each
    threshold, averaged as bbox_map_eval averages: the new kernel against the
    merged one.  eval_map compares fp32 IoUs with the fp32 threshold, so the
    per-image path is given the fp32 thresholds here (widened exactly)."""
    from ld_amd import analyze_results as A
    from ld_amd import evaluation as E
    case = {c[0]: c for c in CASES}[name]
    results, anns, C = synthetic.image_map_inputs(case)
    thrs32 = IO.default_iou_thrs().astype(np.float32)
    acc = A.ImageMapAnalyzer(C, iou_thrs=thrs32.astype(np.float64))
    acc.add_results(results, anns)
    m, ap = acc.compute()
    m, ap = m.cpu().numpy(), ap.cpu().numpy()
    has_gt = acc.has_gt().cpu().numpy()
    picks = [0, 1, 2, len(results) // 2, len(results) - 1]
    if name == 'crowd':
        picks = [1, 3, 7]  # above the LDS route, and 12 classes with GTs
    for i in picks:
        means = []
        for t, thr in enumerate(thrs32):
            mean_ap, res = E.eval_map([results[i]], [anns[i]],
                                      iou_thr=float(thr), logger='silent')
            means.append(mean_ap)
            for c, r in enumerate(res):
                assert (r['num_gts'] > 0) == bool(has_gt[i, c])
                if r['num_gts'] > 0:
                    assert np.float32(r['ap']) == ap[i, t, c], (i, t, c)
        # eval_map's mean over classes is np.mean as well
        assert m[i] == sum(means) / len(means), i


def test_workspace_route_equals_lds_route():
    """The same images through LDS and, with LD_EVAL_IMAGE_NO_LDS, through the
    global-memory workspace; 'crowd' also mixes both routes in one launch."""
    for name in ('base', 'ignore', 'crowd'):
        case = {c[0]: c for c in CASES}[name]
        results, anns, C = synthetic.image_map_inputs(case)
        a = _host(_analyze(results, anns, C))
        b = _host(_analyze(results, anns, C, no_lds=True))
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), name
    # the small images of 'crowd' alone (all LDS) == inside the mixed launch
    results, anns, C = synthetic.image_map_inputs(CASES[-1])
    small = [i for i, r in enumerate(results) if sum(map(len, r)) <= 256
             and len(anns[i]['bboxes']) + len(anns[i]['bboxes_ignore']) <= 128]
    assert 0 < len(small) < len(results)
    sub = _host(_analyze([results[i] for i in small],
                         [anns[i] for i in small], C))
    np.testing.assert_array_equal(sub[0], a[0][small])
    np.testing.assert_array_equal(sub[1], a[1][small])


def test_beyond_the_fixture_vs_restatement():
    """More than 128 recall steps in one class (numpy's recursive split of the
    float64 sum) and more than 128 classes with GTs (the same for the float32
    mean), and equal scores (stable order), against the numpy restatement."""
    rng = np.random.RandomState(9)
    C = 140
    gts = synthetic._eval_boxes(rng, 300, lo=10.0, hi=30.0)
    gl = np.zeros(300, np.int64)
    gl[:C] = np.arange(C)  # every class has a GT; class 0 has 161
    jit = rng.normal(0, 0.6, size=(2, 300, 4)).astype(np.float32)
    boxes = np.concatenate([gts + jit[0], gts + jit[1]])
    labs = np.concatenate([gl, gl])
    score = (rng.randint(0, 64, size=600) / np.float32(64)).astype(np.float32)
    d5 = np.concatenate([boxes, score[:, None]], 1).astype(np.float32)
    res = [d5[labs == c] for c in range(C)]
    ann = dict(bboxes=gts, labels=gl)
    small = ([d5[:40][labs[:40] == c] for c in range(C)],
             dict(bboxes=gts[:5], labels=gl[:5]))
    m, ap, has_gt = _host(_analyze([res, small[0]], [ann, small[1]], C))
    for i, (r, a) in enumerate(((res, ann), small)):
        m_o, _, ap_o, hg_o = IO.image_map(r, a)
        np.testing.assert_array_equal(ap[i], ap_o)
        np.testing.assert_array_equal(has_gt[i], hg_o)
        assert m[i] == m_o
    assert has_gt[0].all() and C > 128
    # class 0: more than 128 true positives at the lowest threshold
    tp0 = IO.class_ap(res[0], gts[gl == 0], np.zeros((0, 4)), [0.5])[0]
    assert tp0[0] > 128 / 161


def _raster(img, gts, dets, score_thr, thickness, gt_color, det_color):
    """Numpy rasteriser of the documented rule."""
    out = img.copy()
    H, W = img.shape[:2]
    dets = np.asarray(dets, np.float32).reshape(-1, 5)
    keep = dets[:, 4] >= np.float32(score_thr)
    boxes = [(b, gt_color) for b in np.asarray(gts, np.float32).reshape(-1, 4)]
    boxes += [(b[:4], det_color) for b in dets[keep]]
    ys, xs = np.mgrid[0:H, 0:W]
    for b, col in boxes:
        x1, y1, x2, y2 = (int(v) for v in b.astype(np.int32))
        inside = (xs >= x1) & (xs <= x2) & (ys >= y1) & (ys <= y2)
        band = (xs < x1 + thickness) | (xs > x2 - thickness) | \
            (ys < y1 + thickness) | (ys > y2 - thickness)
        out[inside & band] = col
    return out


def test_draw_gt_det_bboxes_vs_numpy_rasteriser():
    from ld_amd import analyze_results as A
    rng = np.random.RandomState(4)
    H, W = 97, 131
    img = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    gts = np.array([[10.9, 12.2, 60.7, 50.1],      # truncation, not rounding
                    [-20.5, -7.5, 30.2, 40.0],     # partly outside, negative
                    [100.0, 60.0, 400.0, 300.0],   # partly outside, far side
                    [-50.0, -50.0, -10.0, -10.0],  # wholly outside
                    [200.0, 10.0, 260.0, 40.0],    # wholly outside
                    [70.0, 70.0, 71.0, 71.0],      # thinner than the outline
                    [80.0, 20.0, 60.0, 40.0]],     # x2 < x1: nothing
                   np.float32)
    dets = np.concatenate([synthetic._eval_boxes(rng, 300, 2.0, 80.0) - 40.0,
                           rng.uniform(0, 1, (300, 1))], 1).astype(np.float32)
    dets[0, 4] = 0.3  # exactly on the threshold: kept (>=)
    for thr, th in ((0, 2), (0.3, 1), (0.3, 3), (2.0, 2)):
        out = A.draw_gt_det_bboxes(torch.from_numpy(img).cuda(), gts, dets,
                                   score_thr=thr, thickness=th)
        want = _raster(img, gts, dets, thr, th, (255, 102, 61),
                       (72, 101, 241))
        assert out.dtype == torch.uint8 and out.shape == (H, W, 3)
        np.testing.assert_array_equal(out.cpu().numpy(), want)
    # the input is not painted; host images and no boxes are fine
    src = torch.from_numpy(img).cuda()
    out = A.draw_gt_det_bboxes(src, gts[:1], dets[:0], gt_color=(1, 2, 3))
    np.testing.assert_array_equal(src.cpu().numpy(), img)
    np.testing.assert_array_equal(
        out.cpu().numpy(), _raster(img, gts[:1], dets[:0], 0, 2, (1, 2, 3),
                                   (0, 0, 0)))
    out = A.draw_gt_det_bboxes(img, np.zeros((0, 4)), np.zeros((0, 5)))
    np.testing.assert_array_equal(out.cpu().numpy(), img)


def test_empty_inputs():
    """No detections, no GTs, zero images: rc 0 and zeros."""
    from ld_amd import analyze_results as A
    C = 4
    none5, none4 = np.zeros((0, 5), np.float32), np.zeros((0, 4), np.float32)
    nol = np.zeros(0, np.int64)
    box = np.array([[0, 0, 10, 10]], np.float32)
    det = np.array([[0, 0, 10, 10, 0.9]], np.float32)
    one = np.array([1], np.int64)
    acc = A.ImageMapAnalyzer(C)
    acc.add([], [], [], [])  # zero images
    assert len(acc) == 0 and acc.topk(3) == ([], [])
    m, ap = acc.compute()
    assert m.shape == (0, ) and ap.shape == (0, 10, C)
    # an image with nothing, one with GTs only, one with detections only
    acc.add([none5, none5, det], [nol, nol, one], [none4, box, none4],
            [nol, one, nol])
    m, ap, has_gt = _host(acc)
    np.testing.assert_array_equal(m, np.zeros(3))
    np.testing.assert_array_equal(ap, np.zeros((3, 10, C), np.float32))
    np.testing.assert_array_equal(has_gt, [[0] * 4, [0, 1, 0, 0], [0] * 4])
    # and a perfect image scores 1
    assert A.bbox_map_eval([none5, det, none5, none5],
                           dict(bboxes=box, labels=one)) == 1.0
    assert A.bbox_map_eval(([none5, det, none5, none5], None),
                           dict(bboxes=box, labels=one)) == 1.0
    assert acc.topk(1) == ([(2, 0.0)], [(0, 0.0)])
