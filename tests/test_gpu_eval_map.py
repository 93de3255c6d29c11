"""GPU parity (-m gpu) of the mAP evaluation (eval.hip: ld_eval_tpfp /
ld_eval_ap) through ld_amd.evaluation, against
 (1) the REFERENCE's eval_map / tpfp_default outputs (tests/golden/eval_map.npz)
 (2) the numpy restatement (tests/_evalmap_oracle.py) at VOC07-test size.
Bars: TP/FP, num_gts, num_dets exact; recall / precision bit-exact; AP and mAP
within 1e-6."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

from ld_amd import synthetic

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _evalmap_oracle as O  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden', 'eval_map.npz')
CASES = {c[0]: c for c in synthetic.EVAL_CASES}
RUNS = [(case, ds, thr) for case in synthetic.EVAL_CASES
        for ds, thr in synthetic.EVAL_RUNS[case[0]]]


def run_tag(name, dataset, iou_thr):
    return f'{name}_{dataset or "area"}_{int(round(iou_thr * 100))}'


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def _flat_device_tpfp(acc):
    """Record TP/FP of threshold 0 in the golden layout: class-major, image
    order inside a class."""
    thr, cls, _, tp, fp = acc.records()
    keep = thr == 0
    order = np.argsort(cls[keep], kind='stable')
    return tp[:, keep][:, order], fp[:, keep][:, order]


def _check(res, mean_ap, gold, tag, S):
    ng, nd, rec, prec, ap = O.flatten(res, S)
    np.testing.assert_array_equal(ng, gold[f'{tag}_num_gts'])
    np.testing.assert_array_equal(nd, gold[f'{tag}_num_dets'])
    assert rec.dtype == np.float64 and prec.dtype == np.float32
    np.testing.assert_array_equal(rec, gold[f'{tag}_recall'])
    np.testing.assert_array_equal(prec, gold[f'{tag}_precision'])
    np.testing.assert_allclose(ap, gold[f'{tag}_ap'], rtol=0, atol=1e-6)
    np.testing.assert_allclose(np.atleast_1d(mean_ap), gold[f'{tag}_mean_ap'],
                               rtol=0, atol=1e-6)


@pytest.mark.parametrize('case,dataset,iou_thr', RUNS,
                         ids=[run_tag(c[0], d, t) for c, d, t in RUNS])
def test_eval_map_vs_reference_golden(gold, case, dataset, iou_thr):
    from ld_amd import evaluation as E
    tag = run_tag(case[0], dataset, iou_thr)
    S = 1 if case[4] is None else len(case[4])
    det_results, annotations = synthetic.eval_map_inputs(case)
    mean_ap, res = E.eval_map(det_results, annotations, scale_ranges=case[4],
                              iou_thr=iou_thr, dataset=dataset, nproc=1)
    _check(res, mean_ap, gold, tag, S)
    # shapes / types as the reference returns them (mean_ap.py:345-399)
    if case[4] is None:
        assert isinstance(mean_ap, float)
        assert all(isinstance(r['num_gts'], int) and r['recall'].ndim == 1
                   and np.ndim(r['ap']) == 0 for r in res)
    else:
        assert len(mean_ap) == S
        assert all(r['recall'].shape[0] == S and r['ap'].shape == (S, )
                   for r in res)
    # per-image TP/FP of tpfp_default, through the accumulator
    acc = E.MapAccumulator(case[3], (iou_thr, ), case[4], dataset)
    acc.add_results(det_results, annotations)
    tp, fp = _flat_device_tpfp(acc)
    np.testing.assert_array_equal(tp, gold[f'{tag}_tp'])
    np.testing.assert_array_equal(fp, gold[f'{tag}_fp'])


@pytest.mark.parametrize('name', ['base', 'ignore'])
def test_evaluate_as_custom_dataset(gold, name):
    """Several thresholds in one accumulator: each eval_map result, and
    evaluate() as CustomDataset.evaluate(metric='mAP', iou_thr=[...]) builds it
    (datasets/custom.py:297-312) from the reference's numbers."""
    from ld_amd import evaluation as E
    case = CASES[name]
    thrs = (0.5, 0.75)
    det_results, annotations = synthetic.eval_map_inputs(case)
    acc = E.MapAccumulator(case[3], thrs)
    acc.add_results(det_results, annotations)
    for thr, (mean_ap, res) in zip(thrs, acc.compute()):
        _check(res, mean_ap, gold, run_tag(name, None, thr), 1)
    got = acc.evaluate()
    ref = [float(gold[f'{run_tag(name, None, t)}_mean_ap'][0]) for t in thrs]
    want = OrderedDict([('AP50', round(ref[0], 3)), ('AP75', round(ref[1], 3)),
                        ('mAP', sum(ref) / 2)])
    assert list(got) == list(want)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-6, (k, got[k], want[k])


@pytest.mark.parametrize('chunk', [1, 3, 17])
def test_streaming_chunks_bit_identical(chunk):
    from ld_amd import evaluation as E
    for name in ('base', 'exact'):
        case = CASES[name]
        det_results, annotations = synthetic.eval_map_inputs(case)
        one = E.MapAccumulator(case[3], (0.5, 0.75), case[4], 'voc07'
                               if name == 'exact' else None)
        one.add_results(det_results, annotations)
        many = E.MapAccumulator(case[3], (0.5, 0.75), case[4], one.dataset)
        for i in range(0, len(det_results), chunk):
            many.add_results(det_results[i:i + chunk],
                             annotations[i:i + chunk])
        assert many.num_imgs == len(det_results)
        for (ma, ra), (mb, rb) in zip(one.compute(), many.compute()):
            assert np.array_equal(np.atleast_1d(ma), np.atleast_1d(mb))
            for a, b in zip(ra, rb):
                assert a['num_dets'] == b['num_dets']
                assert np.array_equal(a['num_gts'], b['num_gts'])
                for k in ('recall', 'precision', 'ap'):
                    assert np.asarray(a[k]).tobytes() == \
                        np.asarray(b[k]).tobytes(), k


def test_device_path_from_head_get_bboxes():
    """GFLHead.get_bboxes output on seeded maps goes straight to
    MapAccumulator.add (device tensors, no bbox2result, no host copy) and
    scores exactly as eval_map(bbox2result(...)) does."""
    from ld_amd import core, evaluation as E, model_zoo
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
    # GTs: a jittered half of the detections (both classes and misses), plus
    # one ignored GT per image
    rng = np.random.RandomState(5)
    gts, gls, igs, ils = [], [], [], []
    for d, l in res:
        d, l = d.cpu().numpy(), l.cpu().numpy()
        pick = rng.uniform(size=len(l)) < 0.5
        b = d[pick, :4] + rng.normal(0, 2.0, size=(pick.sum(), 4)).astype(
            np.float32)
        gts.append(b.astype(np.float32))
        gls.append(l[pick])
        igs.append(d[:1, :4].copy())
        ils.append(l[:1].copy())
    acc = E.MapAccumulator(C, (0.5, 0.75), device=dev)
    acc.add([d for d, _ in res], [l for _, l in res],
            [torch.from_numpy(g).to(dev) for g in gts],
            [torch.from_numpy(g).to(dev) for g in gls],
            [torch.from_numpy(g).to(dev) for g in igs],
            [torch.from_numpy(g).to(dev) for g in ils])
    got = acc.compute()
    det_results = [core.bbox2result(d, l, C) for d, l in res]
    anns = [dict(bboxes=g, labels=gl, bboxes_ignore=ig, labels_ignore=il)
            for g, gl, ig, il in zip(gts, gls, igs, ils)]
    for thr, (mean_ap, r) in zip((0.5, 0.75), got):
        m_ref, r_ref = E.eval_map(det_results, anns, iou_thr=thr)
        assert mean_ap == m_ref
        for a, b in zip(r, r_ref):
            assert a['num_gts'] == b['num_gts']
            assert a['num_dets'] == b['num_dets']
            for k in ('recall', 'precision', 'ap'):
                assert np.asarray(a[k]).tobytes() == \
                    np.asarray(b[k]).tobytes(), k
        # and the restatement agrees with both
        m_o, r_o, _, _ = O.eval_map(det_results, anns, None, thr)
        _, _, rec, prec, ap = O.flatten(r_o, 1)
        _, _, rec_d, prec_d, ap_d = O.flatten(r, 1)
        np.testing.assert_array_equal(rec_d, rec)
        np.testing.assert_array_equal(prec_d, prec)
        np.testing.assert_allclose(ap_d, ap, rtol=0, atol=1e-6)
    assert got[0][0] > 0.0


def test_voc07_test_scale_vs_restatement():
    """4952 images x 20 classes x 100 detections (~25k per class, one
    segment far above the 4096 of the inference sort), scores on a 1/512 grid
    so equal scores are everywhere: the stable tie rule decides."""
    from ld_amd import evaluation as E
    dev = torch.device('cuda:0')
    s = synthetic.eval_map_scale_inputs()
    B, C = s['dets'].shape[0], 20
    dets = torch.from_numpy(s['dets']).to(dev)
    labels = torch.from_numpy(s['labels']).to(dev)
    gts = torch.from_numpy(s['gts']).to(dev)
    gl = torch.from_numpy(s['gt_labels']).to(dev)
    off = s['gt_off']
    acc = E.MapAccumulator(C, (0.5, ), device=dev)
    for i in range(0, B, 512):
        j = min(B, i + 512)
        acc.add(list(dets[i:j]), list(labels[i:j]),
                [gts[off[k]:off[k + 1]] for k in range(i, j)],
                [gl[off[k]:off[k + 1]] for k in range(i, j)])
    mean_ap, res = acc.compute()[0]
    det_results, anns = [], []
    for k in range(B):
        d, l = s['dets'][k], s['labels'][k]
        det_results.append([d[l == c] for c in range(C)])
        anns.append(dict(bboxes=s['gts'][off[k]:off[k + 1]],
                         labels=s['gt_labels'][off[k]:off[k + 1]]))
    m_o, r_o, tp_o, fp_o = O.eval_map(det_results, anns, None, 0.5)
    tp, fp = _flat_device_tpfp(acc)
    np.testing.assert_array_equal(tp, tp_o)
    np.testing.assert_array_equal(fp, fp_o)
    ng, nd, rec, prec, ap = O.flatten(r_o, 1)
    ng_d, nd_d, rec_d, prec_d, ap_d = O.flatten(res, 1)
    assert nd.min() > 4096 * 4
    np.testing.assert_array_equal(ng_d, ng)
    np.testing.assert_array_equal(nd_d, nd)
    np.testing.assert_array_equal(rec_d, rec)
    np.testing.assert_array_equal(prec_d, prec)
    np.testing.assert_allclose(ap_d, ap, rtol=0, atol=1e-6)
    assert abs(mean_ap - m_o) <= 1e-6
