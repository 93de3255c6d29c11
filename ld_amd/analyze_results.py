"""Per-image mAP ranking on the device: the reference's
``tools/analysis_tools/analyze_results.py`` -- ``bbox_map_eval`` (lines 13-45)
for every image, the good / bad ``topk`` selection of
``ResultVisualizer.evaluate_and_show`` (89-134) and the box overlay of the
images it saves -- run by eval_image.hip (``ld_eval_image_map``,
``ld_draw_boxes``, ``ld_draw_labels``) and ``ld_rank_images`` of eval.hip.

``ImageMapAnalyzer`` takes detections where the heads leave them (device
``(n, 5)`` + ``(n,)`` per image), scores every image of a batch in one launch
and keeps the scores on the device; ``topk`` sorts them there.

Numerics are the reference's for a one-image dataset: IoU fp32, recall
float64, precision fp32, 'area' AP summed in float64 (numpy's pairwise order)
and stored as float32, the mean over classes with GTs a float32 ``np.mean``,
the mean over thresholds float64.  Equal scores in one class are ordered by
position in the class array (stable), which the reference's ``np.argsort``
leaves open.

IoU thresholds: the reference compares fp32 IoUs with the ``np.float64``
scalars of ``np.linspace(.5, .95, 10)``.  Under NumPy 2 promotion (the
installed numpy, 2.x) that comparison is made in float64, and this module does
the same: the kernel takes float64 thresholds.  (NumPy 1 value-based casting
would compare in fp32, as ``ld_amd.eval_map`` does; the two differ only for an
IoU between a threshold and its fp32 rounding.)
"""
import struct
import zlib

import numpy as np
import torch

from . import lib as L
from .eval_common import (as_boxes, eval_batch, eval_device,
                          pack_det_gt_batch, results_to_lists)
from .lossblock import workspace

__all__ = ['bbox_map_eval', 'ImageMapAnalyzer', 'draw_gt_det_bboxes',
           'draw_labels', 'label_texts', 'write_png', 'default_iou_thrs']


def default_iou_thrs():
    """analyze_results.py:38-39, as float64."""
    return np.linspace(
        .5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)


def eval_image_map(batch, num_classes, iou_thrs, no_lds=False):
    """ld_eval_image_map on a packed batch (the dict ``evaluation.eval_tpfp``
    takes) -> device (map (I,) f64, ap (I, T, C) f32, has_gt (I, C) u8)."""
    lib = L.get_lib()
    dev = batch['det_off'].device
    b = eval_batch(batch)
    I = b.num_imgs
    T, C_ = len(iou_thrs), int(num_classes)
    thr = (L.C.c_double * T)(*[float(t) for t in iou_thrs])
    ap = torch.empty((I, T, C_), dtype=torch.float32, device=dev)
    has_gt = torch.empty((I, C_), dtype=torch.uint8, device=dev)
    m = torch.empty((I, ), dtype=torch.float64, device=dev)
    ws = workspace(dev, lib.ld_eval_image_map_workspace_bytes(b.num_dets, I),
                   'eval_image_map')
    L.check(lib.ld_eval_image_map(
        L.C.byref(b), C_, T, L.C.cast(thr, L.C.c_void_p),
        L.LD_EVAL_IMAGE_NO_LDS if no_lds else 0, L.ptr(ap), L.ptr(has_gt),
        L.ptr(m), L.ptr(ws), ws.numel(), L.stream_ptr(dev)),
        'ld_eval_image_map')
    return m, ap, has_gt


def rank_images(scores):
    """ld_rank_images: device float64 (I,) -> (order int32 (I,), sorted f64
    (I,)), ascending and stable."""
    lib = L.get_lib()
    dev = scores.device
    L.require_device(scores, torch.float64, 'scores')
    n = scores.numel()
    order = torch.empty(n, dtype=torch.int32, device=dev)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    ws = workspace(dev, lib.ld_rank_images_workspace_bytes(n), 'rank_images')
    L.check(lib.ld_rank_images(n, L.ptr(scores), L.ptr(order), L.ptr(out),
                               L.ptr(ws), ws.numel(), L.stream_ptr(dev)),
            'ld_rank_images')
    return order, out


def _results_to_lists(results, annotations, num_classes):
    """The reference's list forms -> the per-image lists ``add`` takes; a
    ``(bbox, segm)`` tuple stands for its bbox part."""
    return results_to_lists(results, annotations, num_classes, bbox_segm=True)


class ImageMapAnalyzer:
    """Scores every image on its own (``bbox_map_eval``) and ranks them.

    ``iou_thrs``: float64 thresholds, default ``default_iou_thrs()``; they
    reach the kernel as float64 (see the module docstring)."""

    def __init__(self, num_classes, iou_thrs=None, device=None):
        self.num_classes = int(num_classes)
        if self.num_classes < 1:
            raise ValueError('ImageMapAnalyzer: num_classes must be >= 1')
        thrs = default_iou_thrs() if iou_thrs is None else \
            np.atleast_1d(np.asarray(iou_thrs, dtype=np.float64))
        if not 1 <= len(thrs) <= L.LD_EVAL_MAX_THRS:
            raise ValueError(f'ImageMapAnalyzer: 1..{L.LD_EVAL_MAX_THRS} IoU '
                             f'thresholds, got {len(thrs)}')
        self.iou_thrs = thrs
        self.device = eval_device(device, 'analyze_results')
        self._no_lds = False  # tests: every image through the workspace route
        self._map, self._ap, self._has_gt = [], [], []

    def __len__(self):
        return sum(m.numel() for m in self._map)

    def add(self, det_bboxes, det_labels, gt_bboxes, gt_labels,
            gt_bboxes_ignore=None, gt_labels_ignore=None):
        """One batch: per-image lists of detections (n, 5) with labels (n,)
        -- device tensors as ``get_bboxes`` / ``aug_test`` return them -- and
        GTs (g, 4) / (g,), optionally ignored GTs.  Packed as
        ``MapAccumulator.add`` packs them; one launch."""
        batch = pack_det_gt_batch(
            'ImageMapAnalyzer.add', ('det_bboxes', 'det_labels'), det_bboxes,
            det_labels, gt_bboxes, gt_labels, gt_bboxes_ignore,
            gt_labels_ignore, self.device)
        if batch is None:
            return
        m, ap, has_gt = eval_image_map(batch, self.num_classes, self.iou_thrs,
                                       self._no_lds)
        self._map.append(m)
        self._ap.append(ap)
        self._has_gt.append(has_gt)

    def add_results(self, results, annotations):
        """The reference's forms: ``results[i]`` a list of per-class (k, 5)
        arrays (or a ``(bbox, segm)`` tuple), ``annotations[i]`` a dict of
        ``bboxes`` / ``labels`` and optional ``bboxes_ignore`` /
        ``labels_ignore``."""
        self.add(*_results_to_lists(results, annotations, self.num_classes))

    def _cat(self, parts, shape, dtype):
        if not parts:
            return torch.zeros(shape, dtype=dtype, device=self.device)
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def compute(self):
        """-> device tensors ``map`` (I,) float64 and ``ap`` (I, T, C)
        float32, images in the order they were added."""
        T, C_ = len(self.iou_thrs), self.num_classes
        return (self._cat(self._map, (0, ), torch.float64),
                self._cat(self._ap, (0, T, C_), torch.float32))

    def has_gt(self):
        """-> device (I, C) uint8: the class has a non-ignored GT in the
        image."""
        return self._cat(self._has_gt, (0, self.num_classes), torch.uint8)

    def topk(self, k):
        """analyze_results.py:107-129 -> ``(good, bad)``, lists of ``(index,
        mAP)``: the images in ascending stable mAP order, ``bad`` the first k
        and ``good`` the last k; k is ``len // 2`` when ``2 * k > len``.  The
        sort runs on the device; only the 2k selected pairs come to the host."""
        assert k > 0
        n = len(self)
        if k * 2 > n:
            k = n // 2
        if n == 0:
            return [], []
        order, scores = rank_images(self.compute()[0])

        def pairs(sl):
            return list(zip(order[sl].cpu().tolist(), scores[sl].cpu().tolist()))
        # _mAPs[-0:] is the whole list, _mAPs[:0] is empty
        good = pairs(slice(n - k, n)) if k > 0 else pairs(slice(0, n))
        bad = pairs(slice(0, k))
        return good, bad


def bbox_map_eval(det_result, annotation):
    """The reference's ``bbox_map_eval`` for one image: ``det_result`` a list
    of per-class (k, 5) arrays, or a ``(bbox, segm)`` tuple whose bbox part is
    used; ``annotation`` a dict of ``bboxes`` / ``labels`` and optional
    ``bboxes_ignore`` / ``labels_ignore``.  -> float."""
    bbox = det_result[0] if isinstance(det_result, tuple) else det_result
    acc = ImageMapAnalyzer(len(bbox))
    acc.add_results([bbox], [annotation])
    return float(acc.compute()[0][0].item())


def _color(c):
    c = [int(v) for v in c]
    if len(c) != 3 or not all(0 <= v <= 255 for v in c):
        raise ValueError(f'draw_gt_det_bboxes: color {c} is not three bytes')
    return c[0] | (c[1] << 8) | (c[2] << 16)


def label_texts(det_bboxes, labels, class_names):
    """The text the reference puts on a detection
    (core/visualization/image.py:135-138): ``f'{class_name}|{score:.02f}'``,
    ``f'cls {label}'`` for a label without a name."""
    texts = []
    for b, l in zip(np.asarray(det_bboxes, np.float32).reshape(-1, 5),
                    np.asarray(labels).reshape(-1)):
        name = class_names[int(l)] if class_names is not None and \
            0 <= int(l) < len(class_names) else f'cls {int(l)}'
        texts.append(f'{name}|{float(b[4]):.02f}')
    return texts


def draw_labels(img, texts, xy, scale=1, fg_color=(255, 255, 255),
                bg_color=(0, 0, 0)):
    """Paints text labels IN PLACE into a device (H, W, 3) uint8 tensor, in one
    launch (``ld_draw_labels``).  ``texts[i]`` (str, or bytes) goes at the
    integer corner ``xy[i] = (x1, y1)``: a filled ``bg_color`` rectangle of
    ``len * 6 * scale`` by ``8 * scale`` pixels above ``y1`` (below it when that
    would leave the image at the top), glyph pixels in ``fg_color``.  The font
    is the fixed 5 x 7 table of ``ld_amd.font5x7`` (ASCII 0x20-0x7E; other bytes
    draw as ``?``); a text is cut at ``font5x7.MAX_LEN`` bytes.  Later labels
    paint over earlier ones.  -> ``img``."""
    from . import font5x7 as F
    L.require_device(img, torch.uint8, 'draw_labels image')
    if img.dim() != 3 or img.shape[2] != 3 or not img.is_contiguous():
        raise ValueError('draw_labels: image must be contiguous (H, W, 3)')
    xy = np.asarray(xy, np.int64).reshape(-1, 2)
    n = len(texts)
    if len(xy) != n:
        raise ValueError(f'draw_labels: {n} texts but {len(xy)} corners')
    if int(scale) < 1:
        raise ValueError('draw_labels: scale must be >= 1')
    if n == 0:
        return img
    text = np.zeros((n, F.MAX_LEN), np.uint8)
    desc = np.zeros((n, 4), np.int32)
    desc[:, :2] = np.clip(xy, -(1 << 30), 1 << 30)
    for i, t in enumerate(texts):
        raw = t if isinstance(t, (bytes, bytearray)) else \
            str(t).encode('latin-1', 'replace')
        raw = bytes(raw)[:F.MAX_LEN]
        text[i, :len(raw)] = np.frombuffer(raw, np.uint8)
        desc[i, 2] = len(raw)
    dev = img.device
    dtext = torch.from_numpy(text).to(dev)
    ddesc = torch.from_numpy(desc).to(dev)
    L.check(L.get_lib().ld_draw_labels(
        L.ptr(img), img.shape[0], img.shape[1], L.ptr(dtext), L.ptr(ddesc), n,
        int(scale), _color(fg_color), _color(bg_color), L.stream_ptr(dev)),
        'ld_draw_labels')
    return img


def draw_gt_det_bboxes(img_u8_hwc, gt_bboxes, det_bboxes, score_thr=0,
                       thickness=2, gt_color=(255, 102, 61),
                       det_color=(72, 101, 241), class_names=None, labels=None,
                       text_color=(255, 255, 255), font_scale=1):
    """The overlay of the reference's saved images, in one launch
    (``ld_draw_boxes``): rectangle outlines painted into a COPY of the (H, W,
    3) uint8 image, the GT boxes (g, 4) first, then the detections (m, 5) with
    ``score >= score_thr``.  Coordinates are truncated as
    ``bbox.astype(np.int32)`` does; a box covers x1..x2 and y1..y2 inclusive,
    its outline is the band of ``thickness`` pixels inside each edge, and what
    falls outside the image is dropped.  Colors go to channels 0, 1, 2 in the
    order given.

    With ``labels`` (m,), the class index of every detection, the kept
    detections also get their text ``f'{class_name}|{score:.02f}'``
    (``class_names`` a sequence; ``cls {label}`` without one) at the truncated
    (x1, y1) of their box, through ``draw_labels``: ``text_color`` on a
    ``det_color`` ground, in a fixed 5 x 7 font scaled by ``font_scale`` (the
    reference renders text with matplotlib, which this package does not depend
    on, so the glyphs differ from its).  Without ``labels`` no text is drawn.
    -> device uint8 tensor."""
    img = torch.as_tensor(img_u8_hwc)
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise ValueError('draw_gt_det_bboxes: image must be (H, W, 3) uint8')
    dev = img.device if img.device.type == 'cuda' else \
        eval_device(None, 'analyze_results')
    out = img.to(dev).contiguous().clone()
    g = as_boxes(gt_bboxes, dev, 4).contiguous()
    d = as_boxes(det_bboxes, dev, 5).contiguous()
    lib = L.get_lib()
    L.check(lib.ld_draw_boxes(
        L.ptr(out), out.shape[0], out.shape[1], L.ptr(g), g.shape[0], L.ptr(d),
        d.shape[0], float(score_thr), int(thickness), _color(gt_color),
        _color(det_color), L.stream_ptr(dev)), 'ld_draw_boxes')
    if labels is None:
        if class_names is not None:
            raise ValueError('draw_gt_det_bboxes: class_names needs labels')
        return out
    dn = d.cpu().numpy()
    lab = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor)
                     else labels).reshape(-1)
    if len(lab) != len(dn):
        raise ValueError(f'draw_gt_det_bboxes: {len(dn)} detections but '
                         f'{len(lab)} labels')
    keep = dn[:, 4] >= np.float32(score_thr)  # the kernel's rule
    dn, lab = dn[keep], lab[keep]
    return draw_labels(out, label_texts(dn, lab, class_names),
                       dn[:, :2].astype(np.int32), font_scale, text_color,
                       det_color)


def write_png(path, img_u8_hwc):
    """A minimal PNG writer (8-bit RGB, no filter, stdlib zlib)."""
    a = np.ascontiguousarray(np.asarray(
        img_u8_hwc.cpu() if isinstance(img_u8_hwc, torch.Tensor)
        else img_u8_hwc))
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError('write_png: image must be (H, W, 3) uint8')
    h, w = a.shape[:2]
    raw = np.zeros((h, 1 + 3 * w), dtype=np.uint8)  # filter type 0 per row
    raw[:, 1:] = a.reshape(h, 3 * w)

    def chunk(tag, data):
        body = tag + data
        return struct.pack('>I', len(data)) + body + \
            struct.pack('>I', zlib.crc32(body) & 0xffffffff)

    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n')
        f.write(chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)))
        f.write(chunk(b'IDAT', zlib.compress(raw.tobytes(), 6)))
        f.write(chunk(b'IEND', b''))
