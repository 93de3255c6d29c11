"""GPU parity (-m gpu) of the label painter (eval_image.hip: ld_draw_labels)
through ``ld_amd.analyze_results.draw_labels``, ``draw_gt_det_bboxes(labels=)``
and the detectors' ``show_result``, against the numpy restatement
tests/_labels_oracle.py.  Bar: every pixel equal (assert_array_equal), and the
bytes around the image untouched."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _labels_oracle as LO  # noqa: E402

H, W = 37, 53
GUARD = 4096
FG, BG = (250, 3, 77), (9, 200, 31)


def _image(seed=0):
    return np.random.RandomState(seed).randint(
        0, 256, size=(H, W, 3)).astype(np.uint8)


def _guarded(img):
    """The image between two 4 KiB guard regions of one allocation."""
    n = img.size
    buf = torch.full((GUARD + n + GUARD, ), 0xA5, dtype=torch.uint8,
                     device='cuda')
    view = buf[GUARD:GUARD + n].view(*img.shape)
    view.copy_(torch.from_numpy(img))
    return buf, view


def _check(texts, xy, scale, seed=0):
    from ld_amd import analyze_results as A
    img = _image(seed)
    buf, view = _guarded(img)
    out = A.draw_labels(view, texts, xy, scale, FG, BG)
    assert out is view
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[-GUARD:] == 0xA5).all()
    want = LO.draw_labels(img, texts, xy, scale, FG, BG)
    got = host[GUARD:-GUARD].reshape(H, W, 3)
    np.testing.assert_array_equal(got, want)
    return got, img


CASES = {
    # clipped at the left, right, top and bottom borders and at a corner; a
    # label with y1 < 8 * scale goes below y1, and y1 < 0 starts above row 0
    'left': (['left|0.50'], [(-7, 20)]),
    'right': (['right|0.50'], [(W - 8, 20)]),
    'top': (['top'], [(10, -3)]),
    'bottom': (['bottom'], [(10, H + 3)]),
    'corner': (['corner'], [(W - 5, H + 5)]),
    'corner_top_left': (['corner'], [(-4, -2)]),
    'flip_below': (['flip|0.99'], [(3, 5)]),
    'flip_edge': (['ab', 'cd'], [(3, 7), (20, 8)]),  # 8 * scale: above at 8
    'overlap_ab': (['first|0.10', 'second|0.20'], [(2, 20), (11, 23)]),
    'overlap_ba': (['second|0.20', 'first|0.10'], [(11, 23), (2, 20)]),
    'same_spot': (['AAAA', '0'], [(5, 30), (5, 30)]),
    'empty': (['', 'x', ''], [(0, 20), (30, 20), (5, 30)]),
    'outside_font': ([b'a\x7f\x1f\xe9\x00b'], [(1, 30)]),
    'every_glyph': ([bytes(range(0x20 + 8 * k, min(0x20 + 8 * k + 8, 0x7F)))
                     for k in range(12)],
                    [(0 if k < 6 else 5, 8 * (k % 6) + (0 if k < 6 else 1))
                     for k in range(12)]),
    'too_long': (['x' * 70], [(-350, 20)]),
    'far_away': (['gone', 'gone'], [(10 ** 9, 5), (-2 ** 40, -2 ** 40)]),
}


@pytest.mark.parametrize('scale', (1, 2))
@pytest.mark.parametrize('name', sorted(CASES))
def test_draw_labels_vs_oracle(name, scale):
    texts, xy = CASES[name]
    if name == 'far_away':  # the wrapper clamps to +-2^30, as the kernel does
        got, img = _check(texts, np.clip(xy, -(1 << 30), 1 << 30), scale)
        np.testing.assert_array_equal(got, img)
    else:
        _check(texts, xy, scale)


def test_overlap_orders_differ_and_flip_is_below():
    a, img = _check(*CASES['overlap_ab'], 1)
    b, _ = _check(*CASES['overlap_ba'], 1)
    assert (a != b).any()
    got, img = _check(*CASES['flip_below'], 1)
    changed = (got != img).any(axis=2)
    assert changed[5:13, 3:3 + 9 * 6].any() and not changed[:5].any()


def test_many_labels_more_than_one_stage():
    """More labels than one workgroup stages at once (256)."""
    rng = np.random.RandomState(3)
    n = 300
    texts = ['%d|%.2f' % (k, rng.rand()) for k in range(n)]
    xy = np.stack([rng.randint(-20, W + 5, n), rng.randint(-5, H + 12, n)], 1)
    _check(texts, xy, 1)


def test_zero_labels_and_errors():
    from ld_amd import analyze_results as A
    from ld_amd import lib as L
    img = _image(1)
    buf, view = _guarded(img)
    A.draw_labels(view, [], np.zeros((0, 2)), 1)
    np.testing.assert_array_equal(view.cpu().numpy(), img)
    with pytest.raises(ValueError):
        A.draw_labels(view, ['a'], [(0, 0)], 0)
    with pytest.raises(ValueError):
        A.draw_labels(view, ['a', 'b'], [(0, 0)], 1)
    with pytest.raises(ValueError):
        A.draw_labels(view[:, :, :2], ['a'], [(0, 0)], 1)
    lib = L.get_lib()
    text = torch.zeros(64, dtype=torch.uint8, device='cuda')
    desc = torch.zeros(4, dtype=torch.int32, device='cuda')
    args = (L.ptr(text), L.ptr(desc), 1)
    assert lib.ld_draw_labels(L.ptr(view), H, W, *args, 0, 0, 0, None) == -1
    assert lib.ld_draw_labels(L.ptr(view), -1, W, *args, 1, 0, 0, None) == -1
    assert lib.ld_draw_labels(L.ptr(view), H, W, L.ptr(text), L.ptr(desc), -1,
                              1, 0, 0, None) == -1
    assert lib.ld_draw_labels(None, H, W, *args, 1, 0, 0, None) == -1
    assert lib.ld_draw_labels(L.ptr(view), H, W, None, L.ptr(desc), 1, 1, 0,
                              0, None) == -1
    assert lib.ld_draw_labels(L.ptr(view), H, W, *args, 1025, 0, 0,
                              None) == -3
    assert lib.ld_draw_labels(L.ptr(view), 0, W, *args, 1, 0, 0, None) == 0
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[-GUARD:] == 0xA5).all()
    np.testing.assert_array_equal(host[GUARD:-GUARD].reshape(H, W, 3), img)


def test_descriptor_bounds_applied():
    """A descriptor straight to the library with len far outside 0..64 and
    corners far outside int range of an image: len is clamped (negative draws
    nothing, large reads its 64-byte slot only)."""
    from ld_amd import lib as L
    from ld_amd import font5x7 as F
    img = _image(2)
    buf, view = _guarded(img)
    text = np.full((2, F.MAX_LEN), ord('m'), np.uint8)
    desc = np.array([[1, 20, -5, 0], [-370, 30, 2 ** 31 - 1, 0]], np.int32)
    rc = L.get_lib().ld_draw_labels(
        L.ptr(view), H, W, L.ptr(torch.from_numpy(text).cuda()),
        L.ptr(torch.from_numpy(desc).cuda()), 2, 1, 0x010203, 0x040506, None)
    assert rc == 0
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[-GUARD:] == 0xA5).all()
    want = LO.draw_labels(img, ['m' * 64], [(-370, 30)], 1, (3, 2, 1),
                          (6, 5, 4))
    np.testing.assert_array_equal(host[GUARD:-GUARD].reshape(H, W, 3), want)


def _raster(img, dets, thickness, color):
    """The documented rule of ld_draw_boxes, for detections only."""
    out = img.copy()
    ys, xs = np.mgrid[0:img.shape[0], 0:img.shape[1]]
    for b in dets:
        x1, y1, x2, y2 = (int(v) for v in b[:4].astype(np.int32))
        inside = (xs >= x1) & (xs <= x2) & (ys >= y1) & (ys <= y2)
        band = (xs < x1 + thickness) | (xs > x2 - thickness) | \
            (ys < y1 + thickness) | (ys > y2 - thickness)
        out[inside & band] = color
    return out


def _read_png(path):
    """8-bit RGB, filter 0 rows: what write_png writes."""
    raw = open(path, 'rb').read()
    assert raw[:8] == b'\x89PNG\r\n\x1a\n'
    pos, idat, size = 8, b'', None
    while pos < len(raw):
        n = int.from_bytes(raw[pos:pos + 4], 'big')
        tag, body = raw[pos + 4:pos + 8], raw[pos + 8:pos + 8 + n]
        if tag == b'IHDR':
            size = (int.from_bytes(body[:4], 'big'),
                    int.from_bytes(body[4:8], 'big'))
        elif tag == b'IDAT':
            idat += body
        pos += 12 + n
    w, h = size
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 3)


def test_draw_gt_det_bboxes_with_labels_and_show_result(tmp_path):
    from ld_amd import analyze_results as A
    from ld_amd.detectors import SingleStageDetector
    img = _image(5)
    names = ('cat', 'dog', 'bird')
    result = [np.array([[4.6, 12.2, 30.9, 33.0, 0.91],
                        [20.0, 2.0, 50.0, 20.0, 0.3]], np.float32),
              np.zeros((0, 5), np.float32),
              np.array([[-6.0, 25.0, 18.0, 60.0, 0.301],
                        [30.0, 30.0, 36.0, 36.0, 0.05]], np.float32)]
    dets = np.vstack(result)
    labels = np.array([0, 0, 2, 2])
    # default: no text, today's output
    plain = A.draw_gt_det_bboxes(img, np.zeros((0, 4)), dets, score_thr=0.3)
    np.testing.assert_array_equal(
        plain.cpu().numpy(),
        _raster(img, dets[dets[:, 4] >= np.float32(0.3)], 2, (72, 101, 241)))
    # labels=: the kept (>=) detections get their text on a det_color ground
    out = A.draw_gt_det_bboxes(img, np.zeros((0, 4)), dets, score_thr=0.3,
                               class_names=names, labels=labels)
    kept = [0, 1, 2]
    want = LO.draw_labels(
        plain.cpu().numpy(), ['cat|0.91', 'cat|0.30', 'bird|0.30'],
        dets[kept, :2].astype(np.int32), 1, (255, 255, 255), (72, 101, 241))
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    with pytest.raises(ValueError):
        A.draw_gt_det_bboxes(img, np.zeros((0, 4)), dets, class_names=names)

    # show_result keeps score > score_thr (strict), names from CLASSES
    class Det(SingleStageDetector):
        def __init__(self):  # the method reads CLASSES only
            torch.nn.Module.__init__(self)
    det = Det()
    det.CLASSES = names
    path = str(tmp_path / 'sub' / 'shown.png')
    got = det.show_result(img, result, score_thr=0.3, out_file=path)
    keep = [0, 2]
    want = _raster(img, dets[keep], 2, (72, 101, 241))
    want = LO.draw_labels(want, ['cat|0.91', 'bird|0.30'],
                          dets[keep, :2].astype(np.int32), 1, (255, 255, 255),
                          (72, 101, 241))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(_read_png(path), want[:, :, ::-1])
    # score_thr = 0 keeps everything; a (bbox, segm) tuple uses its bbox part
    got = det.show_result(img, (result, None), score_thr=0,
                          class_names=('a', 'b', 'c'), font_scale=2)
    want = LO.draw_labels(
        _raster(img, dets, 2, (72, 101, 241)),
        ['a|0.91', 'a|0.30', 'c|0.30', 'c|0.05'],
        dets[:, :2].astype(np.int32), 2, (255, 255, 255), (72, 101, 241))
    np.testing.assert_array_equal(got, want)
