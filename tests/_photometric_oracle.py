"""Numpy float32 restatement of what ``ld_preprocess_batch_photo`` computes for
one image -- TEST INFRASTRUCTURE ONLY.  Every array is float32 and every
operation one numpy ufunc, in the order the kernel (and the header comment of
``ld_image_photo_t``) states, so the kernel's output equals this bit for bit.

The two colour conversions are OpenCV's PUBLISHED float formulas
(cvtColor BGR2HSV / HSV2BGR on 32-bit images: H in [0, 360), S = diff / (|V| +
FLT_EPSILON), V the maximum, the documented branch order for ties, the sector
table on the way back) and the resize is cv2's float INTER_LINEAR.  PARITY
UNPINNED against cv2 itself: it is not available where the goldens are made.
What IS pinned on the reference's own PhotoMetricDistortion
(tests/golden/photometric.npz): the order of the chain, the float32 rounding
of the drawn scalars, the hue wraps, the permutation and that nothing clips.

The composition is the reference's, each step on a real intermediate array:
chain -> float canvas -> window -> resize -> crop -> flip -> normalise -> pad.
"""
import numpy as np

F = np.float32
EPS = F(1.1920928955078125e-07)      # FLT_EPSILON
HSCALE = F(6.0) / F(360.0)           # OpenCV's hscale for hrange = 360
# (B, G, R) = tab[SECTOR[i]]; tab = (V, p, q, t)
SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3],
                   [2, 1, 0]])


def bgr2hsv(img):
    """(..., 3) float32 BGR -> HSV, H in [0, 360]."""
    img = np.asarray(img)
    assert img.dtype == np.float32
    b, g, r = img[..., 0], img[..., 1], img[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    vmin = np.minimum(np.minimum(r, g), b)
    diff = v - vmin
    s = diff / (np.abs(v) + EPS)
    k = F(60.0) / (diff + EPS)
    h = np.where(v == r, (g - b) * k,
                 np.where(v == g, (b - r) * k + F(120.0),
                          (r - g) * k + F(240.0)))
    h = np.where(h < 0, h + F(360.0), h)
    out = np.stack([h, s, v], -1)
    assert out.dtype == np.float32
    return out


def hsv2bgr(img):
    """(..., 3) float32 HSV (H within [-360, 720)) -> BGR."""
    img = np.asarray(img)
    assert img.dtype == np.float32
    h, s, v = img[..., 0], img[..., 1], img[..., 2]
    h = h * HSCALE
    h = np.where(h < 0, h + F(6.0), np.where(h >= F(6.0), h - F(6.0), h))
    sector = np.floor(h).astype(np.int64)
    f = h - sector.astype(np.float32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    f = np.where(bad, F(0.0), f)
    one = F(1.0)
    tab = np.stack([v, v * (one - s), v * (one - s * f),
                    v * (one - s * (one - f))], -1)
    out = np.take_along_axis(tab, SECTOR[sector], -1)
    out = np.where((s == 0)[..., None], v[..., None], out)
    assert out.dtype == np.float32
    return out


def chain(img, photo):
    """PhotoMetricDistortion.__call__ (transforms.py:858-899) on a float32 BGR
    image with the draws of ``photometric_draw`` (None = step not taken).
    ``photo`` None: LoadImageFromFile(to_float32=True) alone, no round trip."""
    x = np.array(img, np.float32)
    if photo is None:
        return x
    if photo['delta'] is not None:
        x = x + F(photo['delta'])
    if photo['mode'] == 1 and photo['alpha'] is not None:
        x = x * F(photo['alpha'])
    x = bgr2hsv(x)
    if photo['saturation'] is not None:
        x[..., 1] = x[..., 1] * F(photo['saturation'])
    if photo['hue'] is not None:
        h = x[..., 0] + F(photo['hue'])
        h = np.where(h > F(360.0), h - F(360.0), h)
        h = np.where(h < 0, h + F(360.0), h)
        x[..., 0] = h
    x = hsv2bgr(x)
    if photo['mode'] == 0 and photo['alpha'] is not None:
        x = x * F(photo['alpha'])
    if photo['perm'] is not None:
        x = x[..., list(photo['perm'])]
    assert x.dtype == np.float32
    return np.ascontiguousarray(x)


def hue_wraps(img, photo):
    """(any H + hue > 360, any H + hue < 0) of the chain above."""
    if photo is None or photo['hue'] is None:
        return False, False
    x = np.array(img, np.float32)
    if photo['delta'] is not None:
        x = x + F(photo['delta'])
    if photo['mode'] == 1 and photo['alpha'] is not None:
        x = x * F(photo['alpha'])
    h = bgr2hsv(x)[..., 0] + F(photo['hue'])
    return bool((h > 360).any()), bool((h < 0).any())


def _coef(dst, src):
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * (float(src) / float(dst)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo = s < 0
    f[lo], s[lo] = 0.0, 0
    hi = s >= src - 1
    f[hi], s[hi] = 0.0, src - 1
    s1 = np.minimum(s + 1, src - 1)
    return s, s1, F(1.0) - f, f


def resize_linear_f32(img, new_h, new_w):
    """cv2.resize(img, (new_w, new_h), interpolation=INTER_LINEAR), float32
    HWC: float coefficients, horizontal pass then vertical pass."""
    img = np.asarray(img)
    assert img.dtype == np.float32
    h, w = img.shape[:2]
    sx0, sx1, ax0, ax1 = _coef(new_w, w)
    sy0, sy1, ay0, ay1 = _coef(new_h, h)
    rows = img[:, sx0] * ax0[None, :, None] + img[:, sx1] * ax1[None, :, None]
    out = rows[sy0] * ay0[:, None, None] + rows[sy1] * ay1[:, None, None]
    assert out.dtype == np.float32
    return out


def normalize(img, mean, std, to_rgb):
    """mmcv.imnormalize on a float32 image: BGR -> RGB, cv2.subtract of the
    float32 mean, cv2.multiply by float32(1 / float64(std))."""
    v = np.asarray(img, np.float32)
    if to_rgb:
        v = v[..., ::-1]
    mean = np.asarray(mean, np.float32)
    stdinv = (1.0 / np.asarray(std, np.float32).astype(np.float64)).astype(
        np.float32)
    return (v - mean) * stdinv


def augment(img, plan, mean, std, to_rgb, pad_h, pad_w, pad_val=(0, 0, 0)):
    """``img`` (h, w, 3) uint8 BGR and a float-mode plan of
    ``DevicePipeline.plan_image`` (or a hand-made dict; missing geometry keys
    mean "not applied", ``photo`` missing or None the identity chain) ->
    (3, pad_h, pad_w) fp32."""
    assert img.dtype == np.uint8
    h, w = img.shape[:2]
    x = chain(img.astype(np.float32), plan.get('photo'))
    ch, cw, top, left = plan.get('canvas', (h, w, 0, 0))
    canvas = np.empty((ch, cw, 3), np.float32)
    canvas[:] = np.asarray(plan.get('fill', (0, 0, 0)), np.float32)
    canvas[top:top + h, left:left + w] = x
    y, x0, wh, ww = plan.get('window', (0, 0, ch, cw))
    window = canvas[y:y + wh, x0:x0 + ww]
    assert window.shape[:2] == (wh, ww)
    new_h, new_w = plan.get('resized', plan['img_shape'][:2])
    r = resize_linear_f32(window, new_h, new_w)
    cy, cx = plan.get('crop', (0, 0))
    oh, ow = plan['img_shape'][:2]
    r = r[cy:cy + oh, cx:cx + ow]
    assert r.shape[:2] == (oh, ow)
    if plan['flip']:
        r = r[:, ::-1]
    v = normalize(r, mean, std, to_rgb)
    out = np.empty((3, pad_h, pad_w), np.float32)
    out[:] = np.broadcast_to(np.asarray(pad_val, np.float32),
                             (3,))[:, None, None]
    out[:, :oh, :ow] = v.transpose(2, 0, 1)
    return out


# ---------------------------------------------------------------------------
# the same two conversions in float64: the sanity bar of the float32 ones
# ---------------------------------------------------------------------------
def roundtrip_f64(img):
    """hsv2bgr(bgr2hsv(x)) with every operation in float64 (the constants are
    the float32 ones, widened)."""
    x = np.asarray(img, np.float64)
    eps, hs = np.float64(EPS), np.float64(HSCALE)
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    vmin = np.minimum(np.minimum(r, g), b)
    diff = v - vmin
    s = diff / (np.abs(v) + eps)
    k = 60.0 / (diff + eps)
    h = np.where(v == r, (g - b) * k,
                 np.where(v == g, (b - r) * k + 120.0, (r - g) * k + 240.0))
    h = np.where(h < 0, h + 360.0, h)
    h = h * hs
    h = np.where(h < 0, h + 6.0, np.where(h >= 6.0, h - 6.0, h))
    sector = np.floor(h).astype(np.int64)
    f = h - sector
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    f = np.where(bad, 0.0, f)
    tab = np.stack([v, v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))],
                   -1)
    out = np.take_along_axis(tab, SECTOR[sector], -1)
    return np.where((s == 0)[..., None], v[..., None], out)
