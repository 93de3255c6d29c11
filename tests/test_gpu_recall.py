"""GPU parity (-m gpu) of the proposal recall (recall.hip:
ld_eval_recalls_match / ld_eval_recalls_count) through ld_amd.recall, against
 (1) tests/golden/recall.npz: the reference's bbox_overlaps + _recalls /
     eval_recalls run on CPU (tools/gen_golden_recall.py)
 (2) tests/_proposal_oracle.py, the numpy restatement of COCOeval's
     useCats = 0 path, for metric='proposal'.
Bars: recalls (float64) and the matched-IoU table (fp32) equal bit for bit,
NaN where the reference has NaN; the LDS and workspace routes, one add and
several, device and host inputs, two runs: the same bits."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from ld_amd import synthetic

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _proposal_oracle as PO  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden', 'recall.npz')
RUNS = {r[0]: r for r in synthetic.recall_cases()}
COCO = {c[0]: c for c in synthetic.COCO_CASES}
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)
    nan = np.isnan(a)
    assert a[~nan].tobytes() == b[~nan].tobytes()


def _run(tag, no_lds=False, chunk=None, to_device=False):
    """-> (recalls, gt_ious table) of one fixture run."""
    from ld_amd.recall import RecallAccumulator
    _, gts, props, nums, thrs, _, _ = RUNS[tag]
    acc = RecallAccumulator(nums, thrs, device=DEV)
    acc._no_lds = no_lds
    if to_device:
        props = [torch.from_numpy(p).to(DEV) for p in props]
        gts = [None if g is None else torch.from_numpy(g).to(DEV)
               for g in gts]
    chunk = chunk or len(gts)
    for i in range(0, len(gts), chunk):
        acc.add(props[i:i + chunk], gts[i:i + chunk])
    assert acc.num_imgs == len(gts)
    table = acc.gt_ious()
    assert table.is_cuda and table.dtype == torch.float32
    return acc.compute(), table.cpu().numpy()


@pytest.mark.parametrize('tag', list(RUNS))
def test_golden_bit_exact(gold, tag):
    from ld_amd.recall import eval_recalls
    rec, table = _run(tag)
    print(tag, 'recalls', rec.tolist())
    _same(table, gold[f'{tag}_gt_ious'])
    _same(rec, gold[f'{tag}_recalls'])
    # the reference's own entry point and argument forms
    _, gts, props, nums, thrs, _, _ = RUNS[tag]
    _same(eval_recalls(gts, props, nums, thrs, logger='silent', device=DEV),
          gold[f'{tag}_recalls'])


def test_workspace_route_equals_lds_route(gold):
    for tag in ('mixed', 'ties'):
        rec, table = _run(tag, no_lds=True)
        _same(table, gold[f'{tag}_gt_ious'])
        _same(rec, gold[f'{tag}_recalls'])


def test_three_adds_equal_one_and_device_inputs_equal_host(gold):
    for kw in (dict(chunk=2), dict(to_device=True),
               dict(chunk=2, to_device=True, no_lds=True)):
        rec, table = _run('mixed', **kw)
        _same(table, gold['mixed_gt_ious'])
        _same(rec, gold['mixed_recalls'])
    rec, table = _run('noscore', to_device=True, chunk=4)
    _same(table, gold['noscore_gt_ious'])


def test_two_runs_are_bit_identical():
    a, b = _run('big'), _run('big')
    assert a[0].tobytes() == b[0].tobytes()
    assert a[1].tobytes() == b[1].tobytes()


def test_mixed_column_counts_are_refused():
    """(k, 4) beside (k, 5) in one batch is an error; an image without
    proposals fits either."""
    from ld_amd.recall import RecallAccumulator
    _, gts, props, nums, thrs, _, _ = RUNS['mixed']
    full = [i for i, p in enumerate(props) if len(p)]
    bad = list(props)
    bad[full[0]] = bad[full[0]][:, :4]
    acc = RecallAccumulator(nums, thrs, device=DEV)
    with pytest.raises(ValueError, match='in one batch'):
        acc.add(bad, gts)
    assert acc.num_imgs == 0 and acc.total_gt == 0
    acc.add([p[:, :4] if len(p) else np.zeros((0, 5), np.float32)
             for p in props], gts)
    assert acc.num_imgs == len(gts)


def test_more_scored_proposals_than_one_lds_chunk():
    """An image with 12288 + 301 scored proposals: the order pass takes the
    score keys through LDS in two chunks, and the cap (12400, the last budget)
    cuts inside the second.  Bars: the same bits as the proposals sorted on
    the host and given without scores, and for the budget of 50 the same bits
    as its 50 best alone (which take the LDS route)."""
    from ld_amd.recall import RecallAccumulator
    rng = np.random.RandomState(11)
    K = 12288 + 301
    gt = np.array([[10, 10, 60, 50], [100, 40, 180, 120], [30, 200, 90, 260]],
                  np.float32)
    boxes = gt[rng.randint(0, 3, K)] + rng.normal(0, 6, (K, 4))
    scores = rng.permutation(K) / K  # pairwise distinct
    big = np.concatenate([boxes, scores[:, None]], 1).astype(np.float32)
    assert np.unique(big[:, 4]).size == K
    _, gts, props = RUNS['mixed'][:3]
    small, small_gt = props[-1], gts[-1]
    assert len(small) and small_gt is not None and len(small_gt)
    nums, thrs = (50, 13000, 12400), [0.5, 0.7, 0.9]

    def by_score(p):
        return p[np.argsort(-p[:, 4], kind='stable'), :4]

    a = RecallAccumulator(nums, thrs, device=DEV)
    a.add([big, small], [gt, small_gt])
    b = RecallAccumulator(nums, thrs, device=DEV)
    b.add([by_score(big), by_score(small)], [gt, small_gt])
    ta, tb = a.gt_ious().cpu().numpy(), b.gt_ious().cpu().numpy()
    assert ta.shape == (3, 3 + len(small_gt))
    assert ta.tobytes() == tb.tobytes()
    assert a.compute().tobytes() == b.compute().tobytes()
    assert (ta[:, :3] > 0).all() and (ta[:, :3] <= 1).all()
    c = RecallAccumulator(50, thrs, device=DEV)
    c.add([by_score(big)[:50]], [gt])
    assert c.gt_ious().cpu().numpy().tobytes() == ta[:1, :3].tobytes()


def test_evaluate_dict(gold):
    from ld_amd.recall import RecallAccumulator
    _, gts, props, nums, thrs, _, _ = RUNS['unsorted_nums']
    acc = RecallAccumulator(nums, thrs, device=DEV)
    acc.add_results(props, [dict(bboxes=np.zeros((0, 4), np.float32)
                                 if g is None else g) for g in gts])
    ev = acc.evaluate(logger='silent')
    want = gold['unsorted_nums_recalls']
    keys = [f'recall@{n}@{t}' for n in nums for t in np.asarray(thrs).tolist()]
    keys += [f'AR@{n}' for n in nums]
    assert list(ev) == keys and 'recall@12@0.5' in ev and 'AR@3' in ev
    for i, n in enumerate(nums):
        for j, t in enumerate(np.asarray(thrs).tolist()):
            assert ev[f'recall@{n}@{t}'] == want[i, j]
        assert ev[f'AR@{n}'] == want.mean(axis=1)[i]
    # one threshold: no AR keys
    acc = RecallAccumulator(10, 0.75, device=DEV)
    _, gts, props = RUNS['equal'][:3]
    acc.add(props, gts)
    ev = acc.evaluate(logger='silent')
    assert list(ev) == ['recall@10@0.75']
    assert ev['recall@10@0.75'] == gold['equal_int_float_recalls'][0, 0]


def test_device_path_from_head_get_bboxes():
    """GFLHead.get_bboxes output goes straight to RecallAccumulator.add
    (device tensors, the labels unused) and scores as its host copy does."""
    from ld_amd import model_zoo
    from ld_amd.recall import RecallAccumulator
    from ld_amd.registry import build_detector
    dev = torch.device(DEV)
    det = build_detector(model_zoo.gfl_detector(18)).to(dev)
    case = {c[0]: c for c in synthetic.INFER_CASES}['small']
    cls, reg, metas = synthetic.infer_inputs(case, device=dev)
    cfg = dict(nms_pre=1000, min_bbox_size=0, score_thr=0.05,
               nms=dict(type='nms', iou_threshold=0.6), max_per_img=100)
    res = det.bbox_head.get_bboxes(cls, reg, metas, cfg=cfg, rescale=True)
    dets = [d for d, _ in res]
    assert all(d.is_cuda and d.shape[1] == 5 for d in dets)
    assert sum(d.shape[0] for d in dets) > 20
    rng = np.random.RandomState(5)
    gts = []
    for d in dets:
        d = d.cpu().numpy()
        pick = rng.uniform(size=len(d)) < 0.5
        gts.append((d[pick, :4] + rng.normal(0, 2.0, size=(pick.sum(), 4)))
                   .astype(np.float32))
    a = RecallAccumulator((5, 20, 100), [0.5, 0.7, 0.9], device=dev)
    a.add(dets, gts)
    b = RecallAccumulator((5, 20, 100), [0.5, 0.7, 0.9], device=dev)
    b.add([d.cpu().numpy() for d in dets], gts)
    ra, rb = a.compute(), b.compute()
    assert ra.tobytes() == rb.tobytes()
    assert a.gt_ious().cpu().numpy().tobytes() == \
        b.gt_ious().cpu().numpy().tobytes()
    assert 0 < ra[-1, 0] <= 1 and ra[0, 0] <= ra[-1, 0]


# ------------------------------------------------------------------- COCO ----
def _coco(name, tmp_path):
    from ld_amd import coco_eval as CE
    ds, results, classes, kw = synthetic.coco_eval_inputs(COCO[name])
    f = tmp_path / 'ann.json'
    f.write_text(json.dumps(ds))
    return ds, results, classes, kw, CE.CocoGroundTruth.from_json(str(f),
                                                                  classes)


def test_proposal_fast_equals_eval_recalls_of_real_gts(tmp_path):
    from ld_amd.recall import coco_proposal_evaluate, eval_recalls
    ds, results, classes, _, gt = _coco('base', tmp_path)
    props = [np.concatenate(r) for r in results]
    gts = []
    for img in ds['images']:  # fast_eval_recall, coco.py:312-328
        b = [[a['bbox'][0], a['bbox'][1], a['bbox'][0] + a['bbox'][2],
              a['bbox'][1] + a['bbox'][3]] for a in ds['annotations']
             if a['image_id'] == img['id'] and not a['iscrowd']]
        gts.append(np.array(b, dtype=np.float32) if b else np.zeros((0, 4)))
    assert any(a['iscrowd'] for a in ds['annotations'])
    nums = (3, 8, 100)
    want = eval_recalls(gts, props, nums, None, logger='silent', device=DEV)
    assert want.shape == (3, 1)
    thrs = np.linspace(.5, 0.95, 10)
    want = eval_recalls(gts, props, nums, thrs, logger='silent', device=DEV)
    assert synthetic.recall_is_interior(want)
    for r in (props, results):  # arrays, and per-class lists concatenated
        ev = coco_proposal_evaluate(r, gt, 'proposal_fast', nums,
                                    logger='silent', device=DEV)
        assert list(ev) == ['AR@3', 'AR@8', 'AR@100']
        assert np.array([ev[k] for k in ev]).tobytes() == \
            want.mean(axis=1).tobytes()
    # every GT counted: a different (larger) denominator
    allg = eval_recalls([np.concatenate([g.reshape(-1, 4), np.array(
        [[a['bbox'][0], a['bbox'][1], a['bbox'][0] + a['bbox'][2],
          a['bbox'][1] + a['bbox'][3]] for a in ds['annotations']
         if a['image_id'] == img['id'] and a['iscrowd']],
        np.float32).reshape(-1, 4)]) for g, img in zip(gts, ds['images'])],
        props, nums, thrs, logger='silent', device=DEV)
    assert not np.array_equal(allg, want)


@pytest.mark.parametrize('name', ['base', 'maxdet'])
def test_proposal_equals_restatement(tmp_path, name):
    from ld_amd import coco_eval as CE
    from ld_amd.recall import CocoProposalEvaluator, coco_proposal_evaluate
    ds, results, classes, kw, gt = _coco(name, tmp_path)
    nums = kw.get('proposal_nums', (100, 300, 1000))
    items = None if name == 'base' else ['AR@100', 'AR@1000', 'mAP']
    want, ce = PO.evaluate_proposal(ds, results, classes, proposal_nums=nums,
                                    metric_items=items)
    got = coco_proposal_evaluate(results, gt, 'proposal', nums,
                                 metric_items=items, device=DEV)
    print(name, got)
    assert got == want and list(got) == list(want)
    assert any(0 < v < 1 for v in want.values())
    # the tables behind the rounded items, bit for bit
    ev = CocoProposalEvaluator(gt, 'proposal', nums, device=DEV)
    ev.add(range(len(results)),
           [torch.from_numpy(np.concatenate(r)).to(DEV) for r in results])
    out = ev._coco.compute()
    for k in ('precision', 'recall', 'scores'):
        assert out[k].shape == ce.eval[k].shape
        assert out[k].tobytes() == ce.eval[k].tobytes(), k
    assert out['stats'].tobytes() == ce.stats.tobytes()
    # both metrics in one call; the bbox refusal is as it was
    both = coco_proposal_evaluate(results, gt, ['proposal_fast', 'proposal'],
                                  nums, metric_items=items, logger='silent',
                                  device=DEV)
    assert all(both[k] == want[k] for k in want)
    with pytest.raises(NotImplementedError):
        CE.check_metrics('proposal')
