"""GPU parity (-m gpu) of the COCO error analysis (coco_eval.hip:
ld_coco_match_errors + ld_coco_accumulate) through ld_amd.coco_analysis,
against the numpy restatement of the reference's coco_error_analysis.py
(tests/_coco_error_oracle.py).  Bars: ps, the raw rows and the aps table
bit-identical; rows 0-2 bit-identical to CocoEvaluator."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _coco_error_oracle as E  # noqa: E402
import _cocoeval_oracle as O  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUPS = ['animal', 'vehicle', 'food']


def _scene(seed, num_imgs=24, K=6, big=False):
    """Seeded scene: category ids ascending and sparse, three supercategories,
    image ids unsorted; boxes spanning S / M / L, json areas != box areas,
    ~6% crowds; detections jittered from GTs with own (60%), same-
    supercategory (20%) or any (20%) labels, plus false positives; scores on
    a 1/32 grid (ties).  Image 1 has no detections.  ``big``: image 0 holds
    300 GTs and 150 detections of one category (global-tile path, maxDets
    truncation)."""
    rng = np.random.RandomState(seed)
    cat_ids = sorted(int(c) for c in rng.choice(60, K, replace=False) + 1)
    cats = [dict(id=c, name=f'c{c}', supercategory=SUPS[k % 3])
            for k, c in enumerate(cat_ids)]
    img_ids = [int(x) for x in rng.choice(10 * num_imgs, num_imgs,
                                          replace=False)]
    anns, results, nid = [], [], 1
    for n, img in enumerate(img_ids):
        ng = 300 if (big and n == 0) else rng.randint(0, 9)
        xy = rng.uniform(0, 500, size=(ng, 2))
        wh = np.exp(rng.uniform(np.log(4), np.log(250), size=(ng, 2)))
        labs = rng.randint(0, K, size=ng)
        if big and n == 0:
            labs[:40] = 0
        rows = [[] for _ in range(K)]
        for g in range(ng):
            box = [float(xy[g, 0]), float(xy[g, 1]), float(wh[g, 0]),
                   float(wh[g, 1])]
            anns.append(dict(id=nid, image_id=img,
                             category_id=cat_ids[labs[g]], bbox=box,
                             area=float(box[2] * box[3] *
                                        rng.uniform(0.5, 1.0)),
                             iscrowd=int(rng.uniform() < 0.06)))
            nid += 1
            nd = 1 if (big and n == 0) else rng.randint(0, 4)
            for _ in range(nd):
                j = rng.normal(0, 0.2, size=4) * [box[2], box[3], box[2],
                                                   box[3]]
                u = rng.uniform()
                if u < 0.6:
                    lab = labs[g]
                elif u < 0.8:
                    lab = (labs[g] + 3 * rng.randint(1, 3)) % K
                else:
                    lab = rng.randint(0, K)
                if big and n == 0:
                    lab = 0 if g < 150 else lab
                rows[lab].append([box[0] + j[0], box[1] + j[1],
                                  box[0] + box[2] + j[2],
                                  box[1] + box[3] + j[3]])
        for _ in range(rng.randint(0, 5)):
            x, y = rng.uniform(0, 450, size=2)
            w, h = np.exp(rng.uniform(np.log(4), np.log(150), size=2))
            rows[rng.randint(0, K)].append([x, y, x + w, y + h])
        res = []
        for c in range(K):
            r = np.array(rows[c], np.float32).reshape(-1, 4)
            s = np.round(rng.uniform(0.05, 1.0, size=len(r)) * 32) / 32
            res.append(np.concatenate([r, s[:, None]], 1).astype(np.float32))
        if n == 1:
            res = [np.zeros((0, 5), np.float32) for _ in range(K)]
        results.append(res)
    ds = dict(images=[dict(id=i) for i in img_ids], annotations=anns,
              categories=cats)
    return ds, results


def _oracle(ds, results):
    gt = O.COCO(ds)
    dets = O.det2json(results, gt.getImgIds(), gt.getCatIds())
    ps, raw, _ = E.analyze_results(ds, dets)
    return ps, raw, dets


def _analysis(gt, results, order=None, chunk=None, skip=()):
    from ld_amd import coco_analysis as CA
    dev = torch.device('cuda:0')
    ev = CA.CocoErrorAnalysis(gt, dev)
    order = [i for i in (range(len(results)) if order is None else order)
             if i not in skip]
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
    return ev.compute()


def _same(a, b):
    for k in ('ps', 'raw'):
        assert a[k].dtype == np.float64
        assert a[k].tobytes() == b[k].tobytes(), k
    assert json.dumps(a['aps']) == json.dumps(b['aps'])


@pytest.mark.parametrize('seed, big', [(11, False), (12, False), (13, True)])
def test_bit_exact_vs_restatement(seed, big):
    from ld_amd import coco_analysis as CA
    from ld_amd.coco_eval import CocoGroundTruth
    ds, results = _scene(seed, big=big)
    gt = CocoGroundTruth.from_json(ds)
    # images 2 and 5 are never added: the same as images without detections
    skip = (2, 5)
    for i in skip:
        results[i] = [np.zeros((0, 5), np.float32) for _ in results[i]]
    ps, raw, _ = _oracle(ds, results)
    out = _analysis(gt, results, skip=skip)
    assert out['ps'].shape == (7, 101, 6, 4, 1)
    assert out['raw'].tobytes() == raw.tobytes()
    assert out['ps'].tobytes() == ps.tobytes()
    ref = E.aps_table(ps, gt.cat_names)
    assert json.dumps(out['aps']) == json.dumps(ref)
    # the scene exercises every row: Sim / Oth forgive something somewhere
    assert (raw[3] > raw[2]).any() and (raw[4] > raw[3]).any()
    assert CA.fill(raw).tobytes() == ps.tobytes()


@pytest.mark.parametrize('chunk', [1, 5])
def test_streaming_and_order_bit_identical(chunk):
    from ld_amd.coco_eval import CocoGroundTruth
    ds, results = _scene(21, big=True)
    gt = CocoGroundTruth.from_json(ds)
    one = _analysis(gt, results)
    _same(one, _analysis(gt, results, chunk=chunk))
    order = list(np.random.RandomState(chunk).permutation(len(results)))
    _same(one, _analysis(gt, results, order=order, chunk=chunk))


def test_json_path_equals_device_path(tmp_path):
    from ld_amd import coco_analysis as CA
    from ld_amd.coco_eval import CocoGroundTruth
    ds, results = _scene(31)
    gt = CocoGroundTruth.from_json(ds)
    dets = O.det2json(results, gt.img_ids, gt.cat_ids)
    f = tmp_path / 'res.json'
    f.write_text(json.dumps(dets))
    a = CA.coco_error_analysis(str(f), gt)
    _same(a, CA.coco_error_analysis(results, gt))
    _same(a, _analysis(gt, results))


def test_rows_0_2_equal_coco_evaluator_on_get_bboxes():
    """GFLHead.get_bboxes output into both: rows C75 / C50 / Loc equal
    CocoEvaluator(iou_thrs=[.75, .5, .1]) precision at maxDets 100."""
    from ld_amd import coco_analysis as CA, coco_eval as CE, model_zoo
    from ld_amd import synthetic
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
    rng = np.random.RandomState(5)
    anns = []
    for d, l in res:
        d, l = d.cpu().numpy(), l.cpu().numpy()
        pick = rng.uniform(size=len(l)) < 0.5
        b = d[pick, :4] + rng.normal(0, 4.0, size=(pick.sum(), 4)).astype(
            np.float32)
        lab = l[pick].copy()
        swap = rng.uniform(size=len(lab)) < 0.3
        lab[swap] = rng.randint(0, C, size=swap.sum())
        anns.append(dict(bboxes=b.astype(np.float32), labels=lab,
                         bboxes_ignore=d[:1, :4].copy(),
                         labels_ignore=l[:1].copy()))
    gt = CE.CocoGroundTruth.from_annotations(
        anns, num_classes=C, supercategories=[f's{c % 7}' for c in range(C)])
    ea = CA.CocoErrorAnalysis(gt, dev)
    ea.add(range(len(res)), [d for d, _ in res], [l for _, l in res])
    out = ea.compute()
    ev = CE.CocoEvaluator(gt, [.75, .5, .1], (1, 10, 100), dev)
    ev.add(range(len(res)), [d for d, _ in res], [l for _, l in res])
    ref = ev.compute()
    assert out['raw'][:3].tobytes() == \
        np.ascontiguousarray(ref['precision'][..., 2:3]).tobytes()
    np.testing.assert_array_equal(out['npig'], ref['npig'])
    assert (out['raw'][:3] > 0).any()


def test_cli_writes_pngs_and_table(tmp_path):
    pytest.importorskip('matplotlib')
    from ld_amd.coco_eval import CocoGroundTruth
    ds, results = _scene(41, num_imgs=10, K=3)
    gt = CocoGroundTruth.from_json(ds)
    ann = tmp_path / 'ann.json'
    ann.write_text(json.dumps(ds))
    res = tmp_path / 'res.json'
    res.write_text(json.dumps(O.det2json(results, gt.img_ids, gt.cat_ids)))
    out = tmp_path / 'out'
    env = dict(os.environ, MPLBACKEND='Agg')
    subprocess.run([sys.executable, os.path.join(REPO, 'tools',
                                                 'coco_error_analysis.py'),
                    str(res), str(out), '--ann', str(ann), '--types', 'bbox'],
                   check=True, timeout=600, env=env, cwd=REPO)
    names = sorted(os.listdir(out / 'bbox'))
    want = sorted([f'bbox-{n}-{a}.png' for n in gt.cat_names + ['allclass']
                   for a in E.AREA_NAMES] + ['aps.json'])
    assert names == want
    table = json.loads((out / 'bbox' / 'aps.json').read_text())
    ps, _, _ = _oracle(ds, results)
    assert table == json.loads(json.dumps(E.aps_table(ps, gt.cat_names)))
