"""GPU tests (-m gpu) of the inference post-processing at its ties, windows and
NMS edges: ld_get_bboxes_ex / ld_get_bboxes_pre_nms / ld_aug_merge_nms through
ld_amd.lossblock, on the inputs of tests/_infer_exact.py, against the numpy
oracle.

Bar: detection count, labels, scores and all four coordinates BIT-EQUAL to the
oracle (np.array_equal) -- the inputs are built so that both sides do the same
fp32 arithmetic; tests/test_infer_edges_host.py checks those premises.  Every
case runs twice and the two device results must be torch.equal: the candidate
append order comes from atomics and must not reach the result.  Only the voted
coordinates of the voting case keep the bar of tests/test_gpu_infer.py (expf /
powf weights are not exact).

Branch of ld_amd/csrc/infer.hip each case reaches:
  three_paths       radix select (4608 anchors) + LDS sort (1152) + unsorted
                    levels in one launch, koff / keyoff of two images
  boundary levels   unsorted (A == k), LDS sort (A == k + 1, A == 4096), radix
                    select (A == 4097)
  topk_4500         infer_topk_sort_kernel (global bitonic over the level)
  window            best-4096 candidate select, the exhausted flag, the full
                    candidate sort + second NMS; at max_per_img 100 the fast
                    path alone
  keep_limits       the 256-wide NMS chunk loop and its max_keep exits
  many_images       N > 64: the forced full candidate sort, per-image counts
  voting            infer_nms_kernel<DIOU> + infer_vote_kernel
  aug_merge         aug_keys_kernel + the shared NMS tail over AugBoxes"""
import numpy as np
import pytest
import torch

import _infer_exact as X

pytestmark = pytest.mark.gpu

F32 = np.float32


def _dev(maps, dev):
    return None if maps is None else \
        [torch.from_numpy(np.ascontiguousarray(m)).to(dev) for m in maps]


def _call(case, dev, **over):
    from ld_amd import lossblock as LB
    return LB.get_bboxes(
        _dev(case.cls, dev), _dev(case.reg, dev), case.strides,
        case.img_shapes, case.scale_factors, prob=True, voting=case.voting,
        centernesses=_dev(case.ctr, dev), **case.variant,
        **dict(case.settings, **over))


def _twice(case, dev, **over):
    """Two device runs, equal to each other -> numpy (dets, labels) per image."""
    a, b = _call(case, dev, **over), _call(case, dev, **over)
    assert len(a) == len(b) == len(case.img_shapes)
    for n, ((d1, l1), (d2, l2)) in enumerate(zip(a, b)):
        assert torch.equal(d1, d2) and torch.equal(l1, l2), \
            f'image {n}: two runs of one call differ'
    return [(d.cpu().numpy(), l.cpu().numpy()) for d, l in a]


def _assert_exact(got, ref, what):
    assert len(got) == len(ref)
    for n, ((d, l), (rd, rl)) in enumerate(zip(got, ref)):
        tag = f'{what} image {n}'
        assert d.shape == rd.shape, f'{tag}: {d.shape[0]} vs {rd.shape[0]}'
        assert d.dtype == np.float32 and l.dtype == np.int64
        assert np.array_equal(l, rl), f'{tag}: labels'
        assert np.array_equal(d[:, 4], rd[:, 4]), f'{tag}: scores'
        bad = np.nonzero((d[:, :4] != rd[:, :4]).any(1))[0]
        assert bad.size == 0, f'{tag}: boxes differ first at detection ' \
            f'{bad[0]}: {d[bad[0]]} vs {rd[bad[0]]}'


def _exact(case, what, **over):
    dev = torch.device('cuda:0')
    got = _twice(case, dev, **over)
    _assert_exact(got, case.oracle(**over), what)
    return got


def _exact_pre_nms(case, what):
    """with_nms=False: the whole per-level selection, row for row."""
    from ld_amd import lossblock as LB
    dev = torch.device('cuda:0')
    res = LB.get_bboxes(
        _dev(case.cls, dev), _dev(case.reg, dev), case.strides,
        case.img_shapes, None, nms_pre=case.settings['nms_pre'], prob=True,
        centernesses=_dev(case.ctr, dev), with_nms=False, **case.variant)
    for n, (got, ref) in enumerate(zip(res, case.pre_nms())):
        C = ref[1].shape[1]
        assert np.array_equal(got[0].cpu().numpy(), ref[0]), \
            f'{what} image {n}: pre-NMS boxes'
        assert np.array_equal(got[1].cpu().numpy()[:, :C], ref[1]), \
            f'{what} image {n}: pre-NMS scores'
        if len(ref) > 2:
            assert np.array_equal(got[2].cpu().numpy(), ref[2])


# 1 ---------------------------------------------------------------------------
def test_three_selection_paths_in_one_call():
    case = X.three_paths()
    got = _exact(case, 'three_paths')
    assert [d.shape[0] for d, _ in got] == [1024, 1024]
    assert not np.array_equal(got[0][0], got[1][0])
    _exact_pre_nms(case, 'three_paths')


# 2 ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(X.BOUNDARY_LEVELS))
def test_level_size_boundaries(name):
    case = X.boundary(name)
    _exact(case, name)
    _exact_pre_nms(case, name)


def test_topk_reference_level():
    _exact(X.topk_reference_level(), 'reference level')


# 3 ---------------------------------------------------------------------------
def test_nms_pre_above_the_select_width(monkeypatch):
    case = X.topk_4500()
    monkeypatch.delenv('LD_INFER_SORT', raising=False)
    got = _exact(case, 'nms_pre 4500')
    _exact_pre_nms(case, 'nms_pre 4500')
    monkeypatch.setenv('LD_INFER_SORT', 'global')
    forced = _exact(case, 'nms_pre 4500, LD_INFER_SORT=global')
    for (d, l), (fd, fl) in zip(got, forced):
        assert np.array_equal(d, fd) and np.array_equal(l, fl)


# 4 ---------------------------------------------------------------------------
def test_window_runs_out_without_the_hook(monkeypatch):
    monkeypatch.delenv('LD_INFER_LIMIT', raising=False)
    monkeypatch.delenv('LD_INFER_SORT', raising=False)
    case = X.window()
    full = _exact(case, 'window')
    assert full[0][0].shape[0] == case.oracle()[0][0].shape[0] < 1024
    best = _exact(case, 'window, max_per_img 100', max_per_img=100)
    assert np.array_equal(best[0][0], full[0][0][:100])
    assert np.array_equal(best[0][1], full[0][1][:100])


# 5 ---------------------------------------------------------------------------
def test_nms_chunk_and_keep_limits():
    from ld_amd import lib as L
    case = X.keep_limits()
    full = _exact(case, 'max_per_img 1024', max_per_img=1024)[0]
    assert full[0].shape[0] == 1024
    for k in (1, 255, 256, 257):
        d, l = _exact(case, f'max_per_img {k}', max_per_img=k)[0]
        assert d.shape[0] == k
        assert np.array_equal(d, full[0][:k]) and np.array_equal(l, full[1][:k])
    dev = torch.device('cuda:0')
    for k in (1025, 0):
        with pytest.raises(L.LdError):
            _call(case, dev, max_per_img=k)


# 6 ---------------------------------------------------------------------------
def test_iou_equal_to_the_threshold():
    case = X.iou_half()
    both = _exact(case, 'iou_thr 0.5', iou_thr=0.5)
    one = _exact(case, 'iou_thr below 0.5', iou_thr=X.IOU_THR_BELOW_HALF)
    assert both[0][0].shape[0] == 2 and one[0][0].shape[0] == 1


def test_score_equal_to_the_threshold():
    got = _exact(X.score_thr_edge(), 'score_thr 0.25')
    assert np.all(got[0][0][:, 4] > F32(0.25))
    assert (got[0][0][:, 4] == F32(X.SCORE_ABOVE_THR)).sum() == 3


def test_zero_area_boxes_and_nan_overlap():
    got = _exact(X.zero_area(), 'zero area')
    d = got[0][0]
    assert ((d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1]) == 0).sum() == 4


# 7 ---------------------------------------------------------------------------
def test_more_than_64_images():
    case = X.many_images()
    got = _exact(case, 'N = 65')
    assert [d.shape[0] for d, _ in got] == \
        [X.many_images_count(n) for n in range(65)]


# 8 ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ctr_product_ties', 'fcos_points',
                                  'nine_anchors', 'scaled'])
def test_head_variants(name):
    case = getattr(X, name)()
    _exact(case, name)
    _exact_pre_nms(case, name)


# 9 ---------------------------------------------------------------------------
def test_voting_order_exact():
    case = X.voting()
    dev = torch.device('cuda:0')
    (d, l), = _twice(case, dev)
    rd, rl = case.oracle()[0]
    assert d.shape == rd.shape
    assert np.array_equal(l, rl)
    assert np.array_equal(d[:, 4], rd[:, 4])
    np.testing.assert_allclose(d[:, :4], rd[:, :4], atol=2e-3, rtol=0)


# 10 --------------------------------------------------------------------------
def test_aug_merge_view_major_ties():
    import ld_oracle as O
    from ld_amd import lossblock as LB
    dev = torch.device('cuda:0')
    views, boxes, scores = X.aug_views()
    dviews = [dict(v, boxes=torch.from_numpy(v['boxes']).to(dev),
                   scores=torch.from_numpy(v['scores']).to(dev))
              for v in views]
    s = X.AUG_SETTINGS
    rd, rl = O.multiclass_nms(boxes, scores, s['score_thr'], s['iou_thr'],
                              s['max_per_img'])
    runs = [LB.aug_merge_nms(dviews, rescale=True, **s) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and \
        torch.equal(runs[0][1], runs[1][1])
    got = [(runs[0][0].cpu().numpy(), runs[0][1].cpu().numpy())]
    _assert_exact(got, [(rd, rl)], 'aug merge')
    # rescale=False: the result times view 0's (power of two) scale factor
    d0, l0 = LB.aug_merge_nms(dviews, rescale=False, **s)
    want = rd.copy()
    want[:, :4] *= views[0]['scale_factor'][None]
    _assert_exact([(d0.cpu().numpy(), l0.cpu().numpy())], [(want, rl)],
                  'aug merge, rescale=False')
