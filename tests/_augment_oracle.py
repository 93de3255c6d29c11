"""Numpy restatement of what ``ld_preprocess_batch_aug`` computes for one image
-- TEST INFRASTRUCTURE ONLY.  It composes the steps the way the reference's
pipeline does, each on a real intermediate array: Expand's canvas, the
MinIoURandomCrop slice, the restated resize of that slice
(oracle/pipeline_oracle.py), the RandomCrop slice, the flip, the
normalisation, the pad.  The kernel keeps none of these arrays."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import pipeline_oracle as PO  # noqa: E402


def augment(img, plan, mean, std, to_rgb, pad_h, pad_w, pad_val=(0, 0, 0)):
    """``img`` (h, w, 3) uint8 BGR and a plan of ``DevicePipeline.plan_image``
    (or a hand-made dict with its geometry keys; missing ones mean "not
    applied") -> (3, pad_h, pad_w) fp32."""
    h, w = img.shape[:2]
    ch, cw, top, left = plan.get('canvas', (h, w, 0, 0))
    canvas = np.empty((ch, cw, 3), np.uint8)
    canvas[:] = np.asarray(plan.get('fill', (0, 0, 0)), np.uint8)
    canvas[top:top + h, left:left + w] = img
    y, x, wh, ww = plan.get('window', (0, 0, ch, cw))
    window = canvas[y:y + wh, x:x + ww]
    assert window.shape[:2] == (wh, ww)
    new_h, new_w = plan.get('resized', plan['img_shape'][:2])
    r = PO.resize_linear_u8(window, new_h, new_w)
    cy, cx = plan.get('crop', (0, 0))
    oh, ow = plan['img_shape'][:2]
    r = r[cy:cy + oh, cx:cx + ow]
    assert r.shape[:2] == (oh, ow)
    if plan['flip']:
        r = r[:, ::-1]
    v = r.astype(np.float32)
    if to_rgb:
        v = v[..., ::-1]
    mean = np.asarray(mean, np.float32)
    stdinv = (1.0 / np.asarray(std, np.float32).astype(np.float64)).astype(
        np.float32)
    v = (v - mean) * stdinv
    out = np.empty((3, pad_h, pad_w), np.float32)
    out[:] = np.broadcast_to(np.asarray(pad_val, np.float32),
                             (3,))[:, None, None]
    out[:, :oh, :ow] = v.transpose(2, 0, 1)
    return out
