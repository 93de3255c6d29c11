"""CPU-side checks of ld_amd.eval_common, the host plumbing the device
evaluators share: packing of per-image rows, the reference's result lists, the
growing record buffers and the device refusal.  Everything here runs on CPU
tensors."""
import logging

import numpy as np
import pytest
import torch

from ld_amd import eval_common as EC
from ld_amd.lib import LdError

CPU = torch.device('cpu')


def _rows(counts, cols=5, seed=0):
    rng = np.random.RandomState(seed)
    return [torch.from_numpy(rng.rand(n, cols).astype(np.float32))
            for n in counts]


@pytest.mark.parametrize('counts', [(3, 0, 2, 0, 0, 4), (0, 0, 0), (7, ),
                                    (0, )])
def test_pack_rows_offsets_and_counts(counts):
    rows = _rows(counts)
    cat, off, host = EC.pack_rows(rows, CPU)
    assert host == list(counts)
    assert off.dtype == torch.int32 and off.shape == (len(counts) + 1, )
    want = np.concatenate([[0], np.cumsum(counts)])
    np.testing.assert_array_equal(off.numpy(), want)
    assert cat.shape == (sum(counts), 5) and cat.is_contiguous()
    for i, r in enumerate(rows):
        assert torch.equal(cat[want[i]:want[i + 1]], r)


def test_pack_rows_refuses_2_31_rows():
    class Fake:  # only shape[0] is read before the refusal
        shape = (2 ** 30, 5)
    with pytest.raises(LdError, match='X.add: batch too large'):
        EC.pack_rows([Fake(), Fake()], CPU, 'X.add')


def _results(C, counts_per_img, seed=3):
    rng = np.random.RandomState(seed)
    return [[rng.rand(n, 5).astype(np.float32) for n in counts[:C]]
            for counts in counts_per_img]


@pytest.mark.parametrize('ignore', [False, True])
def test_results_to_lists(ignore):
    C = 3
    results = _results(C, [(2, 0, 1), (0, 0, 0)])
    anns = [dict(bboxes=np.arange(8, dtype=np.float64).reshape(2, 4),
                 labels=np.array([2, 0])),
            dict(bboxes=np.zeros((0, 4)), labels=np.zeros(0, np.int64))]
    if ignore:
        anns[0]['bboxes_ignore'] = np.ones((1, 4))
        anns[0]['labels_ignore'] = np.array([1])
    dets, labels, gb, gl, ib, il = EC.results_to_lists(results, anns, C)
    np.testing.assert_array_equal(dets[0], np.concatenate(results[0]))
    np.testing.assert_array_equal(labels[0], [0, 0, 2])
    assert dets[1].shape == (0, 5) and labels[1].shape == (0, )
    assert dets[0].dtype == np.float32 and labels[0].dtype == np.int64
    assert gb[0].dtype == np.float32 and gb[0].shape == (2, 4)
    np.testing.assert_array_equal(gl[0], [2, 0])
    assert ib[1].shape == (0, 4) and il[1].shape == (0, )
    if ignore:
        np.testing.assert_array_equal(ib[0], np.ones((1, 4), np.float32))
        np.testing.assert_array_equal(il[0], [1])
    else:
        assert ib[0].shape == (0, 4) and il[0].shape == (0, )


def test_results_to_lists_bbox_segm_tuple_only_where_asked():
    from ld_amd import analyze_results as A
    C = 3
    res = _results(C, [(1, 2, 0)])
    ann = [dict(bboxes=np.zeros((1, 4)), labels=np.array([1]))]
    plain = EC.results_to_lists(res, ann, C)
    tupled = [(res[0], ['segm'])]
    for got in (EC.results_to_lists(tupled, ann, C, bbox_segm=True),
                A._results_to_lists(tupled, ann, C)):
        for x, y in zip(got, plain):
            np.testing.assert_array_equal(x[0], y[0])
    # MapAccumulator.add_results' form: a 2-tuple is two class arrays
    with pytest.raises(ValueError, match='2 class arrays, expected 3'):
        EC.results_to_lists(tupled, ann, C)


def test_results_to_lists_refusals():
    res = _results(2, [(1, 1)])
    ann = [dict(bboxes=np.zeros((0, 4)), labels=np.zeros(0))]
    with pytest.raises(ValueError, match='2 class arrays, expected 3'):
        EC.results_to_lists(res, ann, 3)
    with pytest.raises(ValueError, match='one annotation per image'):
        EC.results_to_lists(res, ann + ann, 2)


def test_record_buffers_growth_keeps_prefix_and_never_shrinks():
    rec = EC.RecordBuffers(dict(score=torch.float32, bits=torch.int32,
                                match=torch.int64), CPU, 16)
    assert rec.capacity == 0 and rec.n == 0
    rng = np.random.RandomState(5)
    want = {k: np.zeros(0, t.numpy().dtype) for k, t in rec.views().items()}
    caps = []
    for extra in (3, 13, 1, 0, 40, 2, 200, 1):
        rec.reserve(extra)
        assert rec.capacity >= rec.n + extra
        new = rec.views(rec.n, rec.n + extra)
        for k, v in new.items():
            x = rng.randint(-2 ** 31, 2 ** 31, size=extra).astype(np.int32)
            x = x.view(np.float32) if k == 'score' else x  # any bit pattern
            v.copy_(torch.from_numpy(x.astype(want[k].dtype)))
            want[k] = np.concatenate([want[k], x.astype(want[k].dtype)])
        rec.n += extra
        caps.append(rec.capacity)
        for k, v in rec.views().items():  # bit for bit
            assert v.numpy().tobytes() == want[k].tobytes()
            assert rec[k].numel() == rec.capacity
    # max(need, 2 * capacity, floor)
    assert caps == [16, 16, 32, 32, 64, 64, 259, 518]
    assert all(b >= a for a, b in zip(caps, caps[1:]))


def test_eval_device_refuses_cpu():
    with pytest.raises(LdError, match=r'Who: device cpu is not a HIP device '
                                      r'\(there is no CPU path\)'):
        EC.eval_device('cpu', 'Who')
    with pytest.raises(LdError, match='no CPU path'):
        EC.eval_device(torch.device('cpu'), 'Who')


def test_eval_logger_choice():
    own = logging.getLogger('ld_amd.somewhere')
    other = logging.getLogger('other')
    assert EC.eval_logger(other, own) is other
    assert EC.eval_logger('other', own) is other
    assert EC.eval_logger(None, own) is own
    assert EC.eval_logger('silent', own) is own


def test_pack_det_gt_batch_checks_and_layout():
    d = _rows((2, 0, 3))
    lab = [torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int64),
           torch.ones(3, dtype=torch.int64)]
    g = _rows((1, 1, 0), cols=4, seed=1)
    gl = [torch.zeros(1), torch.ones(1), torch.zeros(0)]
    b = EC.pack_det_gt_batch('W.add', ('a', 'b'), d, lab, g, gl, None, None,
                             CPU)
    assert sorted(b) == sorted(EC._BATCH_KEYS)
    np.testing.assert_array_equal(b['det_off'].numpy(), [0, 2, 2, 5])
    np.testing.assert_array_equal(b['gt_off'].numpy(), [0, 1, 2, 2])
    np.testing.assert_array_equal(b['ign_off'].numpy(), [0, 0, 0, 0])
    assert b['dets'].shape == (5, 5) and b['ign'].shape == (0, 4)
    assert b['gt_labels'].dtype == torch.int64
    assert EC.pack_det_gt_batch('W.add', ('a', 'b'), [], [], [], [], None,
                                None, CPU) is None
    with pytest.raises(ValueError, match='W.add: a, b, gt_bboxes and '
                                         'gt_labels need one entry'):
        EC.pack_det_gt_batch('W.add', ('a', 'b'), d, lab[:2], g, gl, None,
                             None, CPU)
    with pytest.raises(ValueError, match='go together'):
        EC.pack_det_gt_batch('W.add', ('a', 'b'), d, lab, g, gl, g, None, CPU)
    with pytest.raises(ValueError, match='GTs and their labels differ'):
        EC.pack_det_gt_batch('W.add', ('a', 'b'), d, lab, g, gl[::-1], None,
                             None, CPU)
