"""numpy restatement of DeltaXYWHBBoxCoder (the reference's
mmdet/core/bbox/coder/delta_xywh_bbox_coder.py:87-237), float32 throughout and
in the reference's operation order.  Independent of ld_amd: the host test pins
it on the reference's stored rows, the GPU tests may use it as a second
opinion."""
import numpy as np

WH_RATIO_CLIP = 16 / 1000


def bbox2delta(proposals, gt, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.)):
    p, g = np.asarray(proposals, np.float32), np.asarray(gt, np.float32)
    half = np.float32(0.5)
    px, py = (p[:, 0] + p[:, 2]) * half, (p[:, 1] + p[:, 3]) * half
    pw, ph = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    gx, gy = (g[:, 0] + g[:, 2]) * half, (g[:, 1] + g[:, 3]) * half
    gw, gh = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    d = np.stack([(gx - px) / pw, (gy - py) / ph, np.log(gw / pw),
                  np.log(gh / ph)], axis=-1).astype(np.float32)
    return ((d - np.asarray(means, np.float32)[None]) /
            np.asarray(stds, np.float32)[None]).astype(np.float32)


def delta2bbox(rois, deltas, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.),
               max_shape=None, wh_ratio_clip=WH_RATIO_CLIP, clip_border=True):
    r, d = np.asarray(rois, np.float32), np.asarray(deltas, np.float32)
    d = d * np.asarray(stds, np.float32)[None] + \
        np.asarray(means, np.float32)[None]
    max_ratio = np.float32(np.abs(np.log(wh_ratio_clip)))
    dx, dy = d[:, 0], d[:, 1]
    dw = np.clip(d[:, 2], -max_ratio, max_ratio)
    dh = np.clip(d[:, 3], -max_ratio, max_ratio)
    half = np.float32(0.5)
    px, py = (r[:, 0] + r[:, 2]) * half, (r[:, 1] + r[:, 3]) * half
    pw, ph = r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
    gw, gh = pw * np.exp(dw), ph * np.exp(dh)
    gx, gy = px + pw * dx, py + ph * dy
    out = np.stack([gx - gw * half, gy - gh * half, gx + gw * half,
                    gy + gh * half], axis=-1).astype(np.float32)
    if clip_border and max_shape is not None:
        h, w = np.float32(max_shape[0]), np.float32(max_shape[1])
        out[:, 0::2] = np.clip(out[:, 0::2], 0, w)
        out[:, 1::2] = np.clip(out[:, 1::2], 0, h)
    return out


def close_rows(got, want, rtol):
    """|got - want| <= rtol * max(|want|, the row's largest |want|): a box
    corner is a difference of a centre and half a size, so its rounding error
    scales with those, not with the corner itself.  -> (ok, worst ratio)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.maximum(np.abs(want), np.abs(want).max(-1, keepdims=True))
    ratio = np.abs(got - want) / np.maximum(scale, 1e-30)
    return bool((ratio <= rtol).all()), float(ratio.max())
