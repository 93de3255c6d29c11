"""CPU checks of the mAP evaluation: the numpy restatement
(tests/_evalmap_oracle.py) against the reference's own outputs
(tests/golden/eval_map.npz, tools/gen_golden_evalmap.py), the argument
refusals of ld_amd.evaluation, and the new C ABI (declared, exported,
host-side argument validation)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from ld_amd import synthetic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _evalmap_oracle as O  # noqa: E402

GOLD = os.path.join(REPO, 'tests', 'golden', 'eval_map.npz')
RUNS = [(case, ds, thr) for case in synthetic.EVAL_CASES
        for ds, thr in synthetic.EVAL_RUNS[case[0]]]


def run_tag(name, dataset, iou_thr):
    return f'{name}_{dataset or "area"}_{int(round(iou_thr * 100))}'


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize('case,dataset,iou_thr', RUNS,
                         ids=[run_tag(c[0], d, t) for c, d, t in RUNS])
def test_restatement_matches_reference(gold, case, dataset, iou_thr):
    tag = run_tag(case[0], dataset, iou_thr)
    S = 1 if case[4] is None else len(case[4])
    det_results, annotations = synthetic.eval_map_inputs(case)
    mean_ap, res, tp, fp = O.eval_map(det_results, annotations, case[4],
                                      iou_thr, dataset)
    np.testing.assert_array_equal(tp, gold[f'{tag}_tp'])
    np.testing.assert_array_equal(fp, gold[f'{tag}_fp'])
    ng, nd, rec, prec, ap = O.flatten(res, S)
    np.testing.assert_array_equal(ng, gold[f'{tag}_num_gts'])
    np.testing.assert_array_equal(nd, gold[f'{tag}_num_dets'])
    assert rec.dtype == np.float64 and prec.dtype == np.float32
    np.testing.assert_array_equal(rec, gold[f'{tag}_recall'])
    np.testing.assert_array_equal(prec, gold[f'{tag}_precision'])
    np.testing.assert_allclose(ap, gold[f'{tag}_ap'], rtol=0, atol=1e-7)
    np.testing.assert_allclose(np.atleast_1d(mean_ap), gold[f'{tag}_mean_ap'],
                               rtol=0, atol=1e-7)


def test_golden_covers_the_edges(gold):
    """The fixture exercises what the issue lists: an exact fp32 IoU of 0.5,
    a GT of area exactly 32**2, classes without GTs or detections, and the
    11-point quirk (earlier scales divided by 11 once per later scale)."""
    assert O.iou_matrix([[0, 0, 10, 5]], [[0, 0, 10, 10]])[0, 0] == \
        np.float32(0.5)
    ng = gold['exact_area_50_num_gts']  # scales (0,32), (32,64), (64, 1e5)
    det_results, annotations = synthetic.eval_map_inputs(synthetic.EVAL_CASES[-1])
    assert O._areas(annotations[0]['bboxes'])[1] == 32 * 32
    assert ng.sum() > 0
    assert (gold['empty_area_50_num_gts'][-3:] == 0).all()
    assert gold['empty_area_50_num_dets'][-1] == 0
    a11 = gold['scales_voc07_50_ap']
    assert (a11[:, 0] <= 1 / 11**2 + 1e-7).all()  # divided three times


def test_stable_ties_in_restatement():
    """Equal scores: the earlier detection in the class array takes the GT."""
    g = np.array([[0, 0, 10, 10]], np.float32)
    d = np.array([[0, 0, 10, 9, .5], [0, 0, 10, 10, .5]], np.float32)
    tp, fp = O.tpfp(d, g, np.zeros((0, 4)), 0.5, None)
    assert tp.tolist() == [[1, 0]] and fp.tolist() == [[0, 1]]


def test_refusals():
    from ld_amd import evaluation as E
    dets = [[np.zeros((0, 5), np.float32)]]
    ann = [{'bboxes': np.zeros((0, 4), np.float32),
            'labels': np.zeros(0, np.int64)}]
    with pytest.raises(NotImplementedError, match='tpfp_imagenet'):
        E.eval_map(dets, ann, dataset='det')
    with pytest.raises(NotImplementedError, match='tpfp_imagenet'):
        E.eval_map(dets, ann, dataset='vid')
    with pytest.raises(NotImplementedError, match='tpfp_fn'):
        E.eval_map(dets, ann, tpfp_fn=lambda *a: None)
    with pytest.raises(NotImplementedError, match='tpfp_imagenet'):
        E.MapAccumulator(3, dataset='det', device='cuda:0')
    with pytest.raises(ValueError):
        E.MapAccumulator(3, iou_thrs=[0.5] * 17, device='cuda:0')
    with pytest.raises(ValueError):
        E.MapAccumulator(0, device='cuda:0')
    from ld_amd.lib import LdError
    with pytest.raises(LdError, match='no CPU path'):
        E.MapAccumulator(3, device='cpu')
    import ld_amd
    assert ld_amd.eval_map is E.eval_map
    assert ld_amd.MapAccumulator is E.MapAccumulator


def _declared():
    src = open(os.path.join(REPO, 'include', 'ld_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return set(re.findall(r'\b(ld_[a-z0-9_]+)\s*\(', src))


def test_eval_symbols_declared_and_exported():
    from ld_amd import lib as L
    names = {'ld_eval_tpfp', 'ld_eval_tpfp_workspace_bytes', 'ld_eval_ap',
             'ld_eval_ap_workspace_bytes'}
    assert names <= _declared()
    assert names <= set(L.SIGNATURES)
    if not L.lib_available():
        import __graft_entry__
        __graft_entry__.build()
    so = ctypes.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(so, n), n
    # ld_eval_batch_t: 9 pointers, 4 int32
    assert ctypes.sizeof(L.EvalBatchT) == 88


def test_eval_abi_validates_on_the_host():
    """Malformed arguments are refused before anything reaches the device."""
    from ld_amd import lib as L
    if not L.lib_available():
        import __graft_entry__
        __graft_entry__.build()
    lib = L.get_lib()
    assert lib.ld_eval_tpfp_workspace_bytes(-1) == 0
    assert lib.ld_eval_tpfp_workspace_bytes(1000) >= 8000
    assert lib.ld_eval_ap_workspace_bytes(10, 0) == 0
    assert lib.ld_eval_ap_workspace_bytes(10, 17) == 0
    assert lib.ld_eval_ap_workspace_bytes(1 << 20, 3) > (1 << 20) * 24
    thr = (ctypes.c_float * 1)(0.5)
    b = L.EvalBatchT()
    b.num_imgs = 0
    tp = lib.ld_eval_tpfp
    assert tp(None, 3, 1, None, 1, ctypes.cast(thr, ctypes.c_void_p), None,
              None, None, None, None, 0, None) == -1
    assert tp(ctypes.byref(b), 3, 1, None, 1,
              ctypes.cast(thr, ctypes.c_void_p), None, None, None, None, None,
              0, None) == -1  # no images
    b.num_imgs = 1
    assert tp(ctypes.byref(b), 3, 2, None, 1,
              ctypes.cast(thr, ctypes.c_void_p), None, None, None, None, None,
              0, None) == -1  # two scales need ranges
    assert tp(ctypes.byref(b), 3, 1, None, 17,
              ctypes.cast(thr, ctypes.c_void_p), None, None, None, None, None,
              0, None) == -1  # too many thresholds
    ap = lib.ld_eval_ap
    assert ap(0, None, None, None, 3, 1, 1, None, 0, None, None, None, None,
              None, 0, None) == -1  # no num_gts / outputs
    assert ap(0, None, None, None, 3, 1, 1, None, 4, None, None, None, None,
              None, 0, None) == -1  # unknown flag
