"""CPU checks of the per-image mAP ranking (ld_amd/analyze_results.py,
eval_image.hip): the numpy restatement (tests/_imagemap_oracle.py) against the
REFERENCE's bbox_map_eval outputs (tests/golden/analyze_results.npz) bit for
bit, the summation-order model the kernel implements against numpy itself, the
topk rule, the PNG writer and the C ABI declarations."""
import os
import re
import struct
import sys
import zlib

import numpy as np
import pytest

from ld_amd import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _imagemap_oracle as IO  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden', 'analyze_results.npz')
CASES = synthetic.image_map_cases()
NEW_SYMBOLS = ('ld_eval_image_map_workspace_bytes', 'ld_eval_image_map',
               'ld_rank_images_workspace_bytes', 'ld_rank_images',
               'ld_draw_boxes')


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def test_golden_was_made_with_this_numpy_promotion(gold):
    """The threshold comparison follows the numpy that wrote the fixture:
    NumPy 2 promotes fp32-vs-float64 scalar comparisons to float64."""
    assert str(gold['numpy_version']).split('.')[0] == '2'
    assert np.float32(0.55) >= np.float64(0.55)  # a float64 comparison


def test_fixture_covers_what_it_must(gold):
    """'crowd' has images above the kernel's LDS route and one with >= 9
    classes with GTs; nothing is excluded for ties."""
    results, anns, C = synthetic.image_map_inputs(CASES[-1])
    assert CASES[-1][0] == 'crowd'
    ndet = [sum(len(r) for r in res) for res in results]
    ngt = [len(a['bboxes']) + len(a['bboxes_ignore']) for a in anns]
    assert sum(n > 256 for n in ndet) >= 3 and sum(g > 128 for g in ngt) >= 2
    assert gold['crowd_has_gt'].sum(1).max() >= 9
    for case in CASES:
        assert gold[f'{case[0]}_valid'].all()
        res, _, _ = synthetic.image_map_inputs(case)
        for r in res:  # tie-free inputs: the reference has one answer
            assert all(len(np.unique(x[:, 4])) == len(x) for x in r)


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize('use_model', [False, True], ids=['numpy', 'model'])
def test_restatement_equals_reference_bitwise(gold, case, use_model):
    name = case[0]
    results, anns, C = synthetic.image_map_inputs(case)
    assert gold[f'{name}_ap'].shape == (len(results), 10, C)
    for i, (res, ann) in enumerate(zip(results, anns)):
        m, mean_ap, ap, has_gt = IO.image_map(res, ann, use_model=use_model)
        assert ap.dtype == np.float32 and isinstance(m, float)
        np.testing.assert_array_equal(ap.view(np.uint32),
                                      gold[f'{name}_ap'][i].view(np.uint32))
        np.testing.assert_array_equal(has_gt, gold[f'{name}_has_gt'][i])
        np.testing.assert_array_equal(mean_ap, gold[f'{name}_mean_ap'][i])
        assert m == gold[f'{name}_map'][i]


def test_sum_order_model_is_numpy():
    """What eval_image.hip implements for np.sum (float64 AP) and np.mean
    (float32 mean over classes): sequential below 8, eight accumulators up to
    128, numpy's recursive split above."""
    rng = np.random.RandomState(3)
    for n in list(range(1, 140)) + [255, 256, 257, 300, 1000, 1203]:
        for _ in range(3):
            a32 = rng.uniform(0, 1, n).astype(np.float32)
            a64 = rng.uniform(0, 1, n) * rng.uniform(0, 1, n)
            assert IO.np_sum_model(a64) == np.sum(a64), n
            assert IO.np_sum_model(a32) == np.sum(a32), n
            assert IO.np_mean_model(a32) == a32.mean(), n


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_topk_clamp_and_order(gold, case):
    name = case[0]
    maps = gold[f'{name}_map'].tolist()
    n = len(maps)
    for tag, k in (('3', 3), ('all', n)):
        good, bad = IO.rank(maps, k)
        assert good == gold[f'{name}_good{tag}'].tolist()
        assert bad == gold[f'{name}_bad{tag}'].tolist()
    good, bad = IO.rank(maps, n)  # 2k > len: k = len // 2
    assert len(good) == len(bad) == n // 2
    assert maps[bad[0]] == min(maps) and maps[good[-1]] == max(maps)
    assert all(maps[a] <= maps[b] for a, b in zip(bad, bad[1:]))


def _read_png(path):
    raw = open(path, 'rb').read()
    assert raw[:8] == b'\x89PNG\r\n\x1a\n'
    pos, chunks = 8, []
    while pos < len(raw):
        n, = struct.unpack('>I', raw[pos:pos + 4])
        tag, data = raw[pos + 4:pos + 8], raw[pos + 8:pos + 8 + n]
        crc, = struct.unpack('>I', raw[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + data) & 0xffffffff
        chunks.append((tag, data))
        pos += 12 + n
    assert [t for t, _ in chunks] == [b'IHDR', b'IDAT', b'IEND']
    w, h, depth, ctype, comp, flt, lace = struct.unpack('>IIBBBBB',
                                                        chunks[0][1])
    assert (depth, ctype, comp, flt, lace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(
        h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 3)


def test_png_writer_round_trip(tmp_path):
    from ld_amd import analyze_results as A
    rng = np.random.RandomState(0)
    for shape in ((1, 1, 3), (7, 13, 3), (64, 48, 3)):
        img = rng.randint(0, 256, size=shape).astype(np.uint8)
        path = str(tmp_path / 'x.png')
        A.write_png(path, img)
        np.testing.assert_array_equal(_read_png(path), img)
    with pytest.raises(ValueError):
        A.write_png(str(tmp_path / 'y.png'), np.zeros((4, 4), np.uint8))


def test_new_symbols_declared():
    """Header and ctypes table name the new entries (tests/test_cabi.py then
    requires the library to export them), and the package exports the Python
    side."""
    from ld_amd import lib as L
    hdr = open(os.path.join(REPO, 'include', 'ld_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for n in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % n, hdr), n
        assert n in L.SIGNATURES, n
    assert 'LD_EVAL_IMAGE_NO_LDS' in hdr and L.LD_EVAL_IMAGE_NO_LDS == 1
    import ld_amd
    for n in ('bbox_map_eval', 'ImageMapAnalyzer', 'draw_gt_det_bboxes'):
        assert hasattr(ld_amd, n), n


def test_argument_validation_without_gpu():
    """Bad arguments are refused before any launch: callable on CPU."""
    import ctypes as C
    from ld_amd import lib as L
    lib = L.get_lib()
    assert lib.ld_eval_image_map_workspace_bytes(100, 4) > 0
    assert lib.ld_eval_image_map_workspace_bytes(-1, 4) == 0
    assert lib.ld_rank_images_workspace_bytes(5000) > 0
    thr = (C.c_double * 1)(0.5)
    b = L.EvalBatchT()
    assert lib.ld_eval_image_map(None, 3, 1, thr, 0, None, None, None, None,
                                 0, None) == -1
    assert lib.ld_eval_image_map(C.byref(b), 3, 1, thr, 0, None, None, None,
                                 None, 0, None) == 0  # zero images
    assert lib.ld_eval_image_map(C.byref(b), 3, L.LD_EVAL_MAX_THRS + 1, thr,
                                 0, None, None, None, None, 0, None) == -1
    assert lib.ld_eval_image_map(C.byref(b), 3, 1, thr, 2, None, None, None,
                                 None, 0, None) == -1  # unknown flag
    assert lib.ld_rank_images(0, None, None, None, None, 0, None) == 0
    assert lib.ld_rank_images(-1, None, None, None, None, 0, None) == -1
    assert lib.ld_rank_images(4, None, None, None, None, 0, None) == -1
    assert lib.ld_draw_boxes(None, 0, 0, None, 0, None, 0, 0.0, 2, 0, 0,
                             None) == 0
    assert lib.ld_draw_boxes(None, 8, 8, None, 1, None, 0, 0.0, 2, 0, 0,
                             None) == -1
    assert lib.ld_draw_boxes(None, 8, 8, None, 0, None, 0, 0.0, 0, 0, 0,
                             None) == -1  # thickness < 1
    from ld_amd import analyze_results as A
    import torch
    with pytest.raises(L.LdError):
        A.ImageMapAnalyzer(3, device='cpu')
    with pytest.raises(L.LdError):
        A.rank_images(torch.zeros(3, dtype=torch.float64))
