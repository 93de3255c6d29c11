"""GPU parity (-m gpu) of the COCO bbox evaluation (coco_eval.hip:
ld_coco_match / ld_coco_accumulate) through ld_amd.coco_eval, against
 (1) tests/golden/coco_eval.npz: the numpy restatement of COCOeval and of the
     reference's CocoDataset.evaluate glue (tools/gen_golden_coco.py)
 (2) the restatement itself (tests/_cocoeval_oracle.py) on a stress case.
Bars: match / ignore bits, npig exact; precision / recall / scores float64
bit-exact; stats and the evaluate() dicts equal."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from ld_amd import synthetic

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cocoeval_oracle as O  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden', 'coco_eval.npz')
CASES = {c[0]: c for c in synthetic.COCO_CASES}


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def _gt_from_json(tmp_path, dataset, classes):
    from ld_amd import coco_eval as CE
    f = tmp_path / 'ann.json'
    f.write_text(json.dumps(dataset))
    return CE.CocoGroundTruth.from_json(str(f), classes)


def _evaluator(gt, results, kw, order=None, chunk=None):
    from ld_amd import coco_eval as CE
    dev = torch.device('cuda:0')
    ev = CE.CocoEvaluator(gt, kw.get('iou_thrs'),
                          kw.get('proposal_nums', (100, 300, 1000)), dev)
    order = list(range(len(results))) if order is None else order
    chunk = chunk or len(order)
    for i in range(0, len(order), chunk):
        idx = order[i:i + chunk]
        dets, labels = [], []
        for j in idx:
            rows = [np.asarray(r, np.float32).reshape(-1, 5)
                    for r in results[j]]
            dets.append(torch.from_numpy(np.concatenate(rows)).to(dev))
            labels.append(torch.from_numpy(np.concatenate(
                [np.full(len(r), c, np.int64) for c, r in enumerate(rows)]))
                .to(dev))
        ev.add(idx, dets, labels)
    return ev


def _same(a, b):
    for k in ('precision', 'recall', 'scores'):
        assert a[k].dtype == np.float64
        assert a[k].tobytes() == b[k].tobytes(), k
    np.testing.assert_array_equal(a['npig'], b['npig'])
    assert a['stats'].tobytes() == b['stats'].tobytes()


@pytest.mark.parametrize('name', list(CASES))
def test_golden_bit_exact(gold, tmp_path, name):
    from ld_amd import coco_eval as CE
    ds, results, classes, kw = synthetic.coco_eval_inputs(CASES[name])
    gt = _gt_from_json(tmp_path, ds, classes)
    # the evaluate() dict through the reference's input form
    got = CE.coco_evaluate(results, gt, classwise=True, **kw)
    assert json.dumps(got) == str(gold[f'{name}_eval'])
    ev = _evaluator(gt, results, kw)
    out = ev.compute()
    for k in ('precision', 'recall', 'scores'):
        assert out[k].shape == gold[f'{name}_{k}'].shape
        assert out[k].tobytes() == gold[f'{name}_{k}'].tobytes(), k
    np.testing.assert_array_equal(out['npig'], gold[f'{name}_npig'])
    np.testing.assert_array_equal(out['stats'], gold[f'{name}_stats'])
    # per detection (records are in det2json order here): kept, match, ignore
    rec = ev.records()
    kept = rec['cat'] < ev.K
    np.testing.assert_array_equal(kept, gold[f'{name}_kept'])
    np.testing.assert_array_equal(rec['match'][kept],
                                  gold[f'{name}_match'][kept])
    np.testing.assert_array_equal(rec['ign'][kept], gold[f'{name}_ign'][kept])
    rows = CE._classwise_table(out['precision'], gt, None, 'silent')
    assert json.dumps(rows) == str(gold[f'{name}_classwise'])


@pytest.mark.parametrize('chunk', [1, 3, 17])
def test_streaming_and_order_bit_identical(tmp_path, chunk):
    for name in ('base', 'ties'):
        ds, results, classes, kw = synthetic.coco_eval_inputs(CASES[name])
        gt = _gt_from_json(tmp_path, ds, classes)
        one = _evaluator(gt, results, kw).compute()
        many = _evaluator(gt, results, kw, chunk=chunk).compute()
        _same(one, many)
        order = list(np.random.RandomState(chunk).permutation(len(results)))
        _same(one, _evaluator(gt, results, kw, order=order,
                              chunk=chunk).compute())


def test_add_refuses_an_image_twice(tmp_path):
    ds, results, classes, kw = synthetic.coco_eval_inputs(CASES['base'])
    gt = _gt_from_json(tmp_path, ds, classes)
    ev = _evaluator(gt, results[:2], kw)
    with pytest.raises(ValueError, match='twice'):
        _evaluator_add_again(ev, 1)


def _evaluator_add_again(ev, idx):
    z = torch.zeros((0, 5), device='cuda:0')
    ev.add([idx], [z], [torch.zeros(0, dtype=torch.int64, device='cuda:0')])


def test_device_path_from_head_get_bboxes():
    """GFLHead.get_bboxes output goes straight to CocoEvaluator.add (device
    tensors, no host copy) and scores exactly as coco_evaluate(bbox2result)."""
    from ld_amd import coco_eval as CE, core, model_zoo
    from ld_amd.registry import build_detector
    dev = torch.device('cuda:0')
    det = build_detector(model_zoo.gfl_detector(18)).to(dev)
    head = det.bbox_head
    case = {c[0]: c for c in synthetic.INFER_CASES}['small']
    cls, reg, metas = synthetic.infer_inputs(case, device=dev)
    cfg = dict(nms_pre=1000, min_bbox_size=0, score_thr=0.05,
               nms=dict(type='nms', iou_threshold=0.6), max_per_img=100)
    res = head.get_bboxes(cls, reg, metas, cfg=cfg, rescale=True)
    C = head.num_classes
    assert sum(d.shape[0] for d, _ in res) > 20
    rng = np.random.RandomState(5)
    anns = []
    for d, l in res:
        d, l = d.cpu().numpy(), l.cpu().numpy()
        pick = rng.uniform(size=len(l)) < 0.5
        b = d[pick, :4] + rng.normal(0, 2.0, size=(pick.sum(), 4)).astype(
            np.float32)
        anns.append(dict(bboxes=b.astype(np.float32), labels=l[pick],
                         bboxes_ignore=d[:1, :4].copy(),
                         labels_ignore=l[:1].copy()))
    gt = CE.CocoGroundTruth.from_annotations(anns, num_classes=C)
    ev = CE.CocoEvaluator(gt, device=dev)
    ev.add(range(len(res)), [d for d, _ in res], [l for _, l in res])
    out = ev.compute()
    det_results = [core.bbox2result(d, l, C) for d, l in res]
    ev2 = CE.CocoEvaluator(gt, device=dev)
    ev2.add(range(len(res)),
            [torch.from_numpy(np.concatenate(r)).to(dev) for r in det_results],
            [torch.from_numpy(np.concatenate(
                [np.full(len(x), c, np.int64) for c, x in enumerate(r)]))
             .to(dev) for r in det_results])
    _same(out, ev2.compute())
    got = CE.coco_evaluate(det_results, gt)
    assert got == ev.evaluate()
    assert got['bbox_mAP_50'] > 0


def _stress_inputs():
    """Three categories over 200 images: category 0 holds >16k detections
    across images; image 0 has one cell of 1000 detections x 200 GTs
    (category 1: its 200k-entry IoU tile exceeds the LDS budget); scores on a
    1/64 grid (ties everywhere); ~5% crowds."""
    rng = np.random.RandomState(77)
    K, num_imgs = 3, 200
    images = [dict(id=1000 - i, width=800, height=800) for i in range(num_imgs)]
    cats = [dict(id=c + 1, name=f'c{c}') for c in range(K)]
    anns, results, nid = [], [], 1
    for n in range(num_imgs):
        rows = [[] for _ in range(K)]
        spec = [(0, 5, 85)] + ([(1, 200, 1000)] if n == 0 else
                               [(1, 2, 4), (2, 3, 6)])
        for k, ng, nd in spec:
            xy = rng.uniform(0, 700, size=(ng, 2))
            wh = np.exp(rng.uniform(np.log(8), np.log(160), size=(ng, 2)))
            for g in range(ng):
                anns.append(dict(id=nid, image_id=images[n]['id'],
                                 category_id=k + 1,
                                 bbox=[float(xy[g, 0]), float(xy[g, 1]),
                                       float(wh[g, 0]), float(wh[g, 1])],
                                 area=float(wh[g, 0] * wh[g, 1] * 0.8),
                                 iscrowd=int(rng.uniform() < 0.05)))
                nid += 1
            src = rng.randint(0, ng, size=nd)
            jit = rng.normal(0, 0.15, size=(nd, 4)) * np.concatenate(
                [wh[src], wh[src]], 1)
            b = np.concatenate([xy[src], xy[src] + wh[src]], 1) + jit
            rows[k] = np.concatenate(
                [b, np.round(rng.uniform(0, 1, size=(nd, 1)) * 64) / 64],
                1).astype(np.float32)
        results.append([np.asarray(r, np.float32).reshape(-1, 5)
                        for r in rows])
    return dict(images=images, annotations=anns, categories=cats), results


def test_stress_vs_restatement(tmp_path):
    from ld_amd import coco_eval as CE
    ds, results = _stress_inputs()
    assert sum(len(r[0]) for r in results) > 16384
    gt = _gt_from_json(tmp_path, ds, None)
    kw = dict(proposal_nums=(100, 300, 1000))
    ev = _evaluator(gt, results, kw, chunk=64)
    out = ev.compute()
    ref, coco_eval, _ = O.evaluate(ds, results, None, **kw)
    for k in ('precision', 'recall', 'scores'):
        assert out[k].tobytes() == coco_eval.eval[k].tobytes(), k
    np.testing.assert_array_equal(out['npig'], O.npig(coco_eval))
    np.testing.assert_array_equal(out['stats'], coco_eval.stats)
    n = sum(len(r) for per_img in results for r in per_img)
    match, ign, kept = O.match_bits(coco_eval, n)
    # records are in add order: image after image, det2json order inside
    rec = ev.records()
    mine = rec['cat'] < ev.K
    np.testing.assert_array_equal(mine, kept)
    np.testing.assert_array_equal(rec['match'][kept], match[kept])
    np.testing.assert_array_equal(rec['ign'][kept], ign[kept])
    assert CE.coco_evaluate(results, gt, **kw) == ref
