"""Device input pipeline + distributed group sampler.

The reference feeds the train step from CPU dataloader workers
(data.workers_per_gpu=2, configs/_base_/datasets/coco_detection.py) running

    Resize(img_scale=(1333, 800), keep_ratio=True) -> RandomFlip(0.5) ->
    Normalize(mean, std, to_rgb=True) -> Pad(size_divisor=32) ->
    DefaultFormatBundle -> Collect -> mmcv.parallel.collate

(configs/ld/ld_r18_gflv1_r101_fpn_coco_1x.py:66-77;
mmdet/datasets/pipelines/transforms.py:31-300 Resize, :303-460 RandomFlip,
:463-540 Pad, :543-590 Normalize).  At the MI355X step rate (50-90 images/s
per GPU) two CPU workers per GPU cannot keep up, so here everything after the
JPEG decode runs on the device: the decoded uint8 HWC images are copied to HBM
as they are (3 bytes / pixel over PCIe instead of 12) and ONE launch of
``ld_preprocess_batch`` (csrc/pipeline.hip) writes the padded fp32 NCHW batch.
The per-image bookkeeping the reference keeps in ``img_metas`` and the GT-box
transforms are host integer / float arithmetic restated below with the same
rounding; GT boxes are tiny and go to the device with the same async copy.

``DistributedGroupSampler`` restates mmdet/datasets/samplers/group_sampler.py:
51-147 (the sampler build_dataloader picks for dist=True) index for index; it
is pinned against the reference's own sampler in tests/test_pipeline.py.

Train-time augmentations -- Expand, MinIoURandomCrop, Resize(keep_ratio=False),
RandomCrop, Pad(size=, pad_val=) (transforms.py:916-1000, 1008-1140, 588-760,
476-540) -- stay in that one launch (``ld_preprocess_batch_aug``): the host
draws and transforms the boxes exactly as the reference does
(``DevicePipeline.plan_image``, pinned on the reference's own classes in
tests/golden/augment.npz), the kernel walks every output pixel back through
crop, resize, window and canvas.  The plain pipeline keeps the plain launch.

Float-image mode -- LoadImageFromFile(to_float32=True), with or without
PhotoMetricDistortion (transforms.py:810-902) in front of the steps above --
is a third launch (``ld_preprocess_batch_photo``): the host makes the
distortion's draws in the reference's order (``photometric_draw``, pinned on
the reference's own class in tests/golden/photometric.npz), the kernel runs
the pointwise chain on each tap, fills Expand's canvas with the float mean and
resizes in float32.

There is no CPU fallback for the image arithmetic: DevicePipeline refuses to
run without the HIP library and a device.
"""
import ctypes as C
import math

import numpy as np
import torch


# ---------------------------------------------------------------------------
# host arithmetic (mmcv.imrescale's size rule, box transforms, img_metas)
# ---------------------------------------------------------------------------
def rescale_size(old_size, scale):
    """mmcv.image.geometric.rescale_size (mmcv 1.2.x, the version the
    reference pins in requirements): ``old_size`` (w, h); ``scale`` a
    (long_edge, short_edge) pair in any order, or a float factor."""
    w, h = old_size
    if isinstance(scale, (float, int)):
        if scale <= 0:
            raise ValueError(f'Invalid scale {scale}, must be positive.')
        factor = scale
    elif isinstance(scale, tuple):
        max_long_edge = max(scale)
        max_short_edge = min(scale)
        factor = min(max_long_edge / max(h, w), max_short_edge / min(h, w))
    else:
        raise TypeError(
            f'Scale must be a number or tuple of int, but got {type(scale)}')
    return int(w * float(factor) + 0.5), int(h * float(factor) + 0.5)


def sample_scale(img_scale, multiscale_mode='range', ratio_range=None,
                 rng=np.random):
    """Resize._random_scale (transforms.py:170-200): the draw order and the
    draws themselves are the reference's, so that the same numpy seed picks the
    same scale."""
    scales = img_scale if isinstance(img_scale, list) else [img_scale]
    if ratio_range is not None:
        lo, hi = ratio_range
        ratio = rng.random_sample() * (hi - lo) + lo
        return int(scales[0][0] * ratio), int(scales[0][1] * ratio)
    if len(scales) == 1:
        return tuple(scales[0])
    if multiscale_mode == 'range':
        longs = [max(s) for s in scales]
        shorts = [min(s) for s in scales]
        long_edge = rng.randint(min(longs), max(longs) + 1)
        short_edge = rng.randint(min(shorts), max(shorts) + 1)
        return long_edge, short_edge
    if multiscale_mode == 'value':
        return tuple(scales[rng.randint(len(scales))])
    raise NotImplementedError(multiscale_mode)


def resize_bboxes(bboxes, scale_factor, img_shape, clip=True):
    """Resize._resize_bboxes (transforms.py:233-241); fp32 like the reference
    (gt boxes are float32, scale_factor is a float32 4-vector)."""
    b = np.asarray(bboxes, np.float32).reshape(-1, 4) * scale_factor
    if clip:
        b[:, 0::2] = np.clip(b[:, 0::2], 0, img_shape[1])
        b[:, 1::2] = np.clip(b[:, 1::2], 0, img_shape[0])
    return b


def flip_bboxes(bboxes, img_shape):
    """RandomFlip.bbox_flip, direction='horizontal' (transforms.py:384-401)."""
    b = np.asarray(bboxes, np.float32)
    out = b.copy()
    w = img_shape[1]
    out[..., 0::4] = w - b[..., 2::4]
    out[..., 2::4] = w - b[..., 0::4]
    return out


def _ceil_to(v, d):
    return int(math.ceil(v / d)) * d


def patch_overlaps(patch, boxes, eps=1e-6):
    """mmdet/core/evaluation/bbox_overlaps.py:4-48 (mode='iou', no + 1) for
    one patch against (k, 4) boxes, in fp32 as there."""
    a = np.asarray(patch).reshape(4).astype(np.float32)
    b = np.asarray(boxes).reshape(-1, 4).astype(np.float32)
    if len(b) == 0:
        return np.zeros(0, np.float32)
    area1 = (a[2] - a[0]) * (a[3] - a[1])
    area2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    overlap = np.maximum(np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]),
                         0) * \
        np.maximum(np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]), 0)
    union = np.maximum(area1 + area2 - overlap, eps)
    return (overlap / union).astype(np.float32)


def _centers_in_patch(boxes, patch):
    """MinIoURandomCrop's is_center_of_bboxes_in_patch (transforms.py:
    1097-1103): strict on all four sides."""
    center = (boxes[:, :2] + boxes[:, 2:]) / 2
    return ((center[:, 0] > patch[0]) * (center[:, 1] > patch[1]) *
            (center[:, 0] < patch[2]) * (center[:, 1] < patch[3]))


def expand_draw(shape, rng, ratio_range=(1, 4), prob=0.5):
    """Expand.__call__'s draws (transforms.py:955-975) for an (h, w) image:
    None when ``prob`` skips it, else (canvas_h, canvas_w, top, left)."""
    h, w = shape
    if rng.uniform(0, 1) > prob:
        return None
    ratio = rng.uniform(ratio_range[0], ratio_range[1])
    left = int(rng.uniform(0, w * ratio - w))
    top = int(rng.uniform(0, h * ratio - h))
    return int(h * ratio), int(w * ratio), top, left


def min_iou_patch(shape, boxes, rng, min_ious=(0.1, 0.3, 0.5, 0.7, 0.9),
                  min_crop_size=0.3):
    """MinIoURandomCrop.__call__'s search (transforms.py:1064-1107) on an
    (h, w) image with all bbox fields concatenated in ``boxes``: the mode
    drawn last and the accepted patch (x1, y1, x2, y2) as an int array, or
    None for mode 1.  ``random.uniform(w - new_w)`` is numpy's
    uniform(low=w - new_w, high=1.0), drawn as the reference draws it."""
    h, w = shape
    sample_mode = (1, *min_ious, 0)
    while True:
        mode = rng.choice(sample_mode)
        if mode == 1:
            return mode, None
        for _ in range(50):
            new_w = rng.uniform(min_crop_size * w, w)
            new_h = rng.uniform(min_crop_size * h, h)
            if new_h / new_w < 0.5 or new_h / new_w > 2:
                continue
            left = rng.uniform(w - new_w)
            top = rng.uniform(h - new_h)
            patch = np.array(
                (int(left), int(top), int(left + new_w), int(top + new_h)))
            if patch[2] == patch[0] or patch[3] == patch[1]:
                continue
            overlaps = patch_overlaps(patch, boxes)
            if len(overlaps) > 0 and overlaps.min() < mode:
                continue
            if len(overlaps) > 0 and not _centers_in_patch(boxes, patch).any():
                continue
            return mode, patch


def crop_size_draw(image_size, crop_size, crop_type, rng):
    """RandomCrop._get_crop_size (transforms.py:716-744)."""
    h, w = image_size
    if crop_type == 'absolute':
        return min(crop_size[0], h), min(crop_size[1], w)
    if crop_type == 'absolute_range':
        assert crop_size[0] <= crop_size[1]
        crop_h = rng.randint(min(h, crop_size[0]), min(h, crop_size[1]) + 1)
        crop_w = rng.randint(min(w, crop_size[0]), min(w, crop_size[1]) + 1)
        return crop_h, crop_w
    if crop_type == 'relative':
        crop_h, crop_w = crop_size
        return int(h * crop_h + 0.5), int(w * crop_w + 0.5)
    if crop_type == 'relative_range':
        cs = np.asarray(crop_size, dtype=np.float32)
        crop_h, crop_w = cs + rng.rand(2) * (1 - cs)
        return int(h * crop_h + 0.5), int(w * crop_w + 0.5)
    raise ValueError(f'Invalid crop_type {crop_type}.')


def crop_bboxes(bboxes, offset_w, offset_h, img_shape, clip=True):
    """RandomCrop._crop_data's bbox half (transforms.py:684-691): the fp32
    offset subtraction, the clip, and ``valid_inds``.  Returns (the shifted
    boxes BEFORE selection, valid_inds)."""
    off = np.array([offset_w, offset_h, offset_w, offset_h], dtype=np.float32)
    b = bboxes - off
    if clip:
        b[:, 0::2] = np.clip(b[:, 0::2], 0, img_shape[1])
        b[:, 1::2] = np.clip(b[:, 1::2], 0, img_shape[0])
    return b, (b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])


def photometric_draw(rng, brightness_delta=32, contrast_range=(0.5, 1.5),
                     saturation_range=(0.5, 1.5), hue_delta=18):
    """PhotoMetricDistortion.__call__'s draws (transforms.py:858-899), every
    one of them in its order with the reference's calls: ``delta``, ``alpha``,
    ``saturation``, ``hue`` as drawn (None when ``randint(2)`` skipped the
    step), ``mode`` (1: contrast before the HSV step, 0: after it) and
    ``perm`` (a tuple, or None).  The reference applies the Python floats in
    place to a float32 array, where they act as float32 scalars; the rounding
    is the descriptor's."""
    d = dict(delta=None, mode=0, alpha=None, saturation=None, hue=None,
             perm=None)
    if rng.randint(2):
        d['delta'] = float(rng.uniform(-brightness_delta, brightness_delta))
    d['mode'] = int(rng.randint(2))
    if d['mode'] == 1:
        if rng.randint(2):
            d['alpha'] = float(rng.uniform(contrast_range[0],
                                           contrast_range[1]))
    if rng.randint(2):
        d['saturation'] = float(rng.uniform(saturation_range[0],
                                            saturation_range[1]))
    if rng.randint(2):
        d['hue'] = float(rng.uniform(-hue_delta, hue_delta))
    if d['mode'] == 0:
        if rng.randint(2):
            d['alpha'] = float(rng.uniform(contrast_range[0],
                                           contrast_range[1]))
    if rng.randint(2):
        d['perm'] = tuple(int(v) for v in rng.permutation(3))
    return d


_STEP_RANK = {'Expand': 0, 'MinIoURandomCrop': 1, 'Resize': 2, 'RandomCrop': 3,
              'RandomFlip': 4, 'Normalize': 4, 'Pad': 5}


class DevicePipeline:
    """The reference's train_pipeline from Resize to collate, on the device.

    ``__call__(images, gt_bboxes, gt_labels)`` takes per-image decoded uint8 HWC
    arrays (BGR, what LoadImageFromFile produces) and float32 (k, 4) / int64
    (k,) annotations; returns the dict the detector's ``forward_train`` takes:
    ``img`` (N, 3, Hpad, Wpad) fp32 on the device, ``img_metas`` (the keys of
    Collect's default meta_keys that the heads read), ``gt_bboxes`` /
    ``gt_labels`` lists of device tensors, and ``gt_bboxes_ignore`` when the
    optional ``gt_bboxes_ignore=`` is given (transformed like ``gt_bboxes``).
    """

    def __init__(self, img_scale=(1333, 800), keep_ratio=True, flip_ratio=0.5,
                 mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375),
                 to_rgb=True, size_divisor=32, multiscale_mode='range',
                 ratio_range=None, bbox_clip_border=True, device=None,
                 crop=None, expand=None, min_iou_crop=None, pad_size=None,
                 pad_val=0, to_float32=False, photo=None,
                 min_gt_bbox_wh=None):
        """``crop`` / ``expand`` / ``min_iou_crop``: the keyword dicts of the
        reference's RandomCrop / Expand / MinIoURandomCrop (or None);
        ``pad_size`` (H, W) and ``pad_val``: Pad(size=, pad_val=).
        ``to_float32``: LoadImageFromFile(to_float32=True), the float-image
        mode (float Expand fill, float resize); ``photo``: the keyword dict
        of PhotoMetricDistortion (or None), which needs that mode.
        ``min_gt_bbox_wh``: FilterAnnotations' (w, h), applied first."""
        if photo is not None and not to_float32:
            # transforms.py:855 asserts img.dtype == np.float32
            raise ValueError(
                'photo= (PhotoMetricDistortion) needs to_float32=True: the '
                'reference asserts a float32 image')
        self.float_mode = bool(to_float32)
        self.photo = None if photo is None else dict(
            dict(brightness_delta=32, contrast_range=(0.5, 1.5),
                 saturation_range=(0.5, 1.5), hue_delta=18), **photo)
        if self.photo is not None and not abs(self.photo['hue_delta']) <= 360:
            raise ValueError(
                f"hue_delta {self.photo['hue_delta']}: the one wrap each way "
                'of the reference needs |hue_delta| <= 360')
        self.min_gt_bbox_wh = None if min_gt_bbox_wh is None else tuple(
            float(v) for v in min_gt_bbox_wh)
        if pad_size is not None and size_divisor is not None:
            # transforms.py:495 asserts that only one of them is given
            raise ValueError(
                f'Pad: size={tuple(pad_size)} and size_divisor={size_divisor} '
                'are both given; pass size_divisor=None with a fixed size')
        self.keep_ratio = bool(keep_ratio)
        self.crop = None if crop is None else dict(
            dict(crop_type='absolute', allow_negative_crop=False,
                 bbox_clip_border=True), **crop)
        if self.crop is not None and self.crop['crop_type'] not in (
                'relative_range', 'relative', 'absolute', 'absolute_range'):
            raise ValueError(f"Invalid crop_type {self.crop['crop_type']}.")
        self.expand = None if expand is None else dict(
            dict(mean=(0, 0, 0), to_rgb=True, ratio_range=(1, 4), prob=0.5),
            **expand)
        # Expand's canvas colour as the reference builds it: the mean in the
        # decoded image's BGR order, cast to uint8 by np.full (transforms.py:
        # 937-940, 971-973)
        self.expand_fill = (0, 0, 0)
        if self.expand is not None:
            m = self.expand['mean']
            m = m[::-1] if self.expand['to_rgb'] else m
            # img.dtype is float32 after LoadImageFromFile(to_float32=True)
            self.expand_fill = tuple(
                float(v) for v in np.full((3,), m, dtype=np.float32)) \
                if self.float_mode else tuple(
                    int(v) for v in np.full((3,), m, dtype=np.uint8))
        self.min_iou_crop = None if min_iou_crop is None else dict(
            dict(min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.3,
                 bbox_clip_border=True), **min_iou_crop)
        self.pad_size = None if pad_size is None else tuple(
            int(v) for v in pad_size)
        self.pad_val = np.broadcast_to(
            np.asarray(pad_val, np.float32), (3,)).copy()
        # everything ld_preprocess_batch cannot express goes through
        # ld_preprocess_batch_aug; the plain pipeline keeps the plain launch
        self.augmented = bool(
            self.crop or self.expand or self.min_iou_crop or self.pad_size
            or not self.keep_ratio or self.pad_val.any() or self.float_mode
            or self.min_gt_bbox_wh)
        self.img_scale = img_scale
        self.multiscale_mode = multiscale_mode
        self.ratio_range = ratio_range
        self.flip_ratio = float(flip_ratio or 0.0)
        self.mean = np.asarray(mean, np.float32)
        self.std = np.asarray(std, np.float32)
        # mmcv.imnormalize: stdinv = 1 / np.float64(std.reshape(1, -1)), then
        # cv2.multiply on the float32 image
        self.std_inv = (1.0 / self.std.astype(np.float64)).astype(np.float32)
        self.to_rgb = bool(to_rgb)
        self.size_divisor = size_divisor
        self.bbox_clip_border = bbox_clip_border
        self.device = torch.device(device if device is not None else 'cuda')

    @classmethod
    def from_cfg(cls, train_pipeline, device=None):
        """Build from a reference config's ``train_pipeline`` list (the dicts
        with type Resize / RandomFlip / Normalize / Pad); other entries are the
        loading / formatting steps this class subsumes.  The optional
        augmentations are taken in one order only: [Expand],
        [MinIoURandomCrop], Resize, [RandomCrop], RandomFlip / Normalize in
        either order, Pad last.  LoadImageFromFile(to_float32=True) selects
        the float-image mode; PhotoMetricDistortion is taken only after it and
        before every step of that list, FilterAnnotations only before both."""
        kw = {}
        prev = None
        for step in train_pipeline:
            t = step['type']
            if t == 'LoadImageFromFile':
                if step.get('to_float32', False):
                    kw['to_float32'] = True
                continue
            if t == 'PhotoMetricDistortion':
                # anywhere else the reference fails its float32 assertion or
                # distorts the canvas too: not this launch
                if not kw.get('to_float32') or prev is not None or \
                        'photo' in kw:
                    raise NotImplementedError(f'pipeline step {t}')
                kw['photo'] = {k: v for k, v in step.items() if k != 'type'}
                continue
            if t == 'FilterAnnotations':
                if prev is not None or 'photo' in kw or \
                        'min_gt_bbox_wh' in kw:
                    raise NotImplementedError(f'pipeline step {t}')
                kw['min_gt_bbox_wh'] = step['min_gt_bbox_wh']
                continue
            if t in _STEP_RANK:
                if prev is not None and _STEP_RANK[t] < _STEP_RANK[prev]:
                    raise NotImplementedError(
                        f'pipeline step {t} after {prev}: the device '
                        'pipeline runs Expand, MinIoURandomCrop, Resize, '
                        'RandomCrop, RandomFlip / Normalize, Pad in this '
                        'order only')
                prev = t
            args = {k: v for k, v in step.items() if k != 'type'}
            if t == 'Expand':
                if args.get('seg_ignore_label') is not None:
                    raise NotImplementedError(
                        'Expand(seg_ignore_label=...): segmentation maps are '
                        'not carried by the device pipeline')
                args.pop('seg_ignore_label', None)
                kw['expand'] = args
            elif t == 'MinIoURandomCrop':
                kw['min_iou_crop'] = args
            elif t == 'RandomCrop':
                kw['crop'] = args
            elif t == 'Resize':
                kw['img_scale'] = step['img_scale']
                kw['keep_ratio'] = step.get('keep_ratio', True)
                kw['multiscale_mode'] = step.get('multiscale_mode', 'range')
                kw['ratio_range'] = step.get('ratio_range')
            elif t == 'RandomFlip':
                kw['flip_ratio'] = step.get('flip_ratio')
            elif t == 'Normalize':
                kw['mean'], kw['std'] = step['mean'], step['std']
                kw['to_rgb'] = step.get('to_rgb', True)
            elif t == 'Pad':
                kw['size_divisor'] = step.get('size_divisor')
                kw['pad_size'] = step.get('size')
                kw['pad_val'] = step.get('pad_val', 0)
            elif t not in ('LoadAnnotations', 'DefaultFormatBundle',
                           'Collect'):
                raise NotImplementedError(f'pipeline step {t}')
        if kw.get('to_float32') and 'size_divisor' not in kw:
            # the stock SSD pipelines have no Pad step: collate pads to the
            # batch maximum only.  (An 8-bit pipeline without Pad keeps the
            # constructor's size_divisor, as it always has.)
            kw['size_divisor'] = None
        return cls(device=device, **kw)

    @classmethod
    def from_test_cfg(cls, test_pipeline, device=None):
        """Build from a reference config's ``test_pipeline``: the
        MultiScaleFlipAug entry (test_time_aug.py:9-112) and its inner Resize /
        RandomFlip / Normalize / Pad.  The views ``aug_views`` expands an image
        into are its img_scale list x [(no flip)] + the flip directions.  The
        device pixel path flips horizontally only."""
        aug = None
        for step in test_pipeline:
            t = step['type']
            if t == 'MultiScaleFlipAug':
                aug = step
            elif t != 'LoadImageFromFile':
                raise NotImplementedError(f'test pipeline step {t}')
        if aug is None:
            raise NotImplementedError('test_pipeline without MultiScaleFlipAug')
        if aug.get('img_scale') is None:
            raise NotImplementedError('MultiScaleFlipAug(scale_factor=...): '
                                      'no configs/ld test pipeline uses it')
        scales = aug['img_scale']
        scales = [tuple(x) for x in (scales if isinstance(scales, list)
                                     else [scales])]
        flip = bool(aug.get('flip', False))
        dirs = aug.get('flip_direction', 'horizontal')
        dirs = list(dirs) if isinstance(dirs, list) else [dirs]
        if flip and any(d != 'horizontal' for d in dirs):
            raise NotImplementedError(
                f'flip_direction {dirs}: the device pipeline flips '
                'horizontally only')
        kw = {}
        for step in aug.get('transforms', []):
            t = step['type']
            if t == 'Resize':
                kw['keep_ratio'] = step.get('keep_ratio', True)
            elif t == 'Normalize':
                kw['mean'], kw['std'] = step['mean'], step['std']
                kw['to_rgb'] = step.get('to_rgb', True)
            elif t == 'Pad':
                kw['size_divisor'] = step.get('size_divisor')
            elif t not in ('RandomFlip', 'ImageToTensor', 'DefaultFormatBundle',
                           'Collect'):
                raise NotImplementedError(f'test pipeline step {t}')
        self = cls(img_scale=scales[0], flip_ratio=0.0, device=device, **kw)
        self.aug_scales = scales
        self.aug_flips = [(False, None)] + \
            ([(True, d) for d in dirs] if flip else [])
        return self

    def view_plans(self, shape):
        """MultiScaleFlipAug.__call__ order (test_time_aug.py:96-106): scale
        major, then (no flip), then each flip direction; one plan per view of
        an image of ``shape`` (h, w)."""
        h, w = shape
        if not self.keep_ratio:
            raise NotImplementedError(
                'keep_ratio=False is not used by any configs/ld or configs/ldv2 '
                'test pipeline')
        scales = getattr(self, 'aug_scales', [tuple(self.img_scale)])
        flips = getattr(self, 'aug_flips', [(False, None)])
        plans = []
        for scale in scales:
            new_w, new_h = rescale_size((w, h), tuple(scale))
            sf = np.array([new_w / w, new_h / h, new_w / w, new_h / h],
                          np.float32)
            for flip, direction in flips:
                if flip and direction != 'horizontal':
                    raise NotImplementedError(
                        f'flip_direction {direction!r}: the device pipeline '
                        'flips horizontally only')
                plans.append(dict(ori_shape=(h, w, 3),
                                  img_shape=(new_h, new_w, 3),
                                  scale_factor=sf, flip=flip,
                                  flip_direction=direction,
                                  scale=tuple(scale)))
        return plans

    def aug_views(self, image, stream=None):
        """One decoded image -> the test-time views, in ONE ld_preprocess_batch
        launch (one descriptor per view).  Returns ``(imgs, img_metas)`` as
        ``forward_test`` takes them: per view a (1, 3, Hpad_v, Wpad_v) tensor
        padded to its own size_divisor multiple, and a one-element meta list
        (ori_shape, img_shape, pad_shape, scale_factor, flip,
        flip_direction)."""
        plans = self.view_plans(tuple(image.shape[:2]))
        res = self([image] * len(plans), plans=plans, stream=stream)
        imgs, metas = [], []
        for v, (p, m) in enumerate(zip(plans, res['img_metas'])):
            ph, pw = m['pad_shape'][:2]
            imgs.append(res['img'][v:v + 1, :, :ph, :pw].contiguous())
            m['flip_direction'] = p['flip_direction']
            m['scale'] = p['scale']
            metas.append([m])
        return imgs, metas

    # -- per-image host decisions -------------------------------------------
    def plan(self, shapes, rng=np.random, gt_bboxes=None, gt_labels=None,
             gt_bboxes_ignore=None):
        """For each (h, w): the scale, the resized size, scale_factor and the
        flip decision, drawing from ``rng`` in the reference's order (scale
        draws of Resize, then RandomFlip's one np.random.choice).

        With augmentations (``self.augmented``) the annotations decide draws
        and survive or not, so they are planned too: see ``plan_image``."""
        if self.augmented:
            n = len(shapes)
            none = [None] * n
            return [self.plan_image(s, rng, b, l, ig) for s, b, l, ig in zip(
                shapes, gt_bboxes or none, gt_labels or none,
                gt_bboxes_ignore or none)]
        plans = []
        for (h, w) in shapes:
            scale = sample_scale(self.img_scale, self.multiscale_mode,
                                 self.ratio_range, rng)
            new_w, new_h = rescale_size((w, h), tuple(scale))
            flip = False
            if self.flip_ratio > 0:
                # np.random.choice(['horizontal', None], p=[r, 1 - r])
                flip = int(rng.choice(2, p=[self.flip_ratio,
                                            1 - self.flip_ratio])) == 0
            sf = np.array([new_w / w, new_h / h, new_w / w, new_h / h],
                          np.float32)
            plans.append(dict(ori_shape=(h, w, 3), img_shape=(new_h, new_w, 3),
                              scale_factor=sf, flip=flip, scale=tuple(scale)))
        return plans

    def plan_image(self, shape, rng=np.random, gt_bboxes=None, gt_labels=None,
                   gt_bboxes_ignore=None):
        """One image through [FilterAnnotations] -> [PhotoMetricDistortion]
        -> Expand -> MinIoURandomCrop -> Resize ->
        RandomCrop -> RandomFlip on the host: every draw the reference makes,
        in its order, and its box arithmetic on the two bbox fields.  The plan
        carries the geometry the kernel needs (``canvas`` (h, w, top, left),
        ``window`` (y, x, h, w) in canvas coordinates, ``resized`` (h, w),
        ``crop`` (y, x) in resized coordinates, ``img_shape``, ``flip``), the
        transformed ``gt_bboxes`` / ``gt_labels`` / ``gt_bboxes_ignore`` and
        which input rows they are (``keep`` / ``keep_ignore``).  A RandomCrop
        that the reference answers with None gives ``dict(rejected=True)``;
        no draw is made after it.  So does a FilterAnnotations that keeps no
        box (loading.py:445-452), before any draw.  In float mode the plan
        also carries ``photo``: the draws of ``photometric_draw``, made before
        Expand's (None without PhotoMetricDistortion), and ``fill`` is the
        float mean."""
        h, w = shape
        boxes = np.zeros((0, 4), np.float32) if gt_bboxes is None else \
            np.array(gt_bboxes, np.float32).reshape(-1, 4)
        ignore = np.zeros((0, 4), np.float32) if gt_bboxes_ignore is None \
            else np.array(gt_bboxes_ignore, np.float32).reshape(-1, 4)
        keep, keep_ig = np.arange(len(boxes)), np.arange(len(ignore))
        # FilterAnnotations (loading.py:445-458): gt_bboxes only
        if self.min_gt_bbox_wh is not None:
            big = ((boxes[:, 2] - boxes[:, 0]) > self.min_gt_bbox_wh[0]) & \
                ((boxes[:, 3] - boxes[:, 1]) > self.min_gt_bbox_wh[1])
            if not big.any():
                return dict(rejected=True, ori_shape=(h, w, 3))
            boxes, keep = boxes[big], keep[big]
        # PhotoMetricDistortion (transforms.py:858-899): its draws come first
        extra = {}
        if self.float_mode:
            extra['photo'] = None if self.photo is None else \
                photometric_draw(rng, **self.photo)
        # Expand (transforms.py:945-997)
        canvas = (h, w, 0, 0)
        if self.expand is not None:
            e = expand_draw((h, w), rng, self.expand['ratio_range'],
                            self.expand['prob'])
            if e is not None:
                canvas = e
                shift = np.tile((e[3], e[2]), 2)
                boxes = boxes + shift.astype(boxes.dtype)
                ignore = ignore + shift.astype(ignore.dtype)
        ch, cw = canvas[:2]
        # MinIoURandomCrop (transforms.py:1045-1137)
        window, mode = (0, 0, ch, cw), None
        if self.min_iou_crop is not None:
            m = self.min_iou_crop
            mode, patch = min_iou_patch(
                (ch, cw), np.concatenate([ignore, boxes], 0), rng,
                m['min_ious'], m['min_crop_size'])
            if patch is not None:
                if len(boxes) + len(ignore) > 0:
                    out = []
                    for b, k in ((boxes, keep), (ignore, keep_ig)):
                        b = b.copy()
                        mask = _centers_in_patch(b, patch)
                        b = b[mask]
                        if m['bbox_clip_border']:
                            b[:, 2:] = b[:, 2:].clip(max=patch[2:])
                            b[:, :2] = b[:, :2].clip(min=patch[:2])
                        b -= np.tile(patch[:2], 2)
                        out += [b, k[mask]]
                    boxes, keep, ignore, keep_ig = out
                # img[patch[1]:patch[3], patch[0]:patch[2]]
                y2, x2 = min(int(patch[3]), ch), min(int(patch[2]), cw)
                window = (int(patch[1]), int(patch[0]), y2 - int(patch[1]),
                          x2 - int(patch[0]))
        wh, ww = window[2:]
        # Resize (transforms.py:203-241)
        scale = sample_scale(self.img_scale, self.multiscale_mode,
                             self.ratio_range, rng)
        if self.keep_ratio:
            new_w, new_h = rescale_size((ww, wh), tuple(scale))
        else:  # mmcv.imresize(img, size=(w, h)): independent w_scale, h_scale
            new_w, new_h = int(scale[0]), int(scale[1])
        sf = np.array([new_w / ww, new_h / wh, new_w / ww, new_h / wh],
                      np.float32)
        boxes = resize_bboxes(boxes, sf, (new_h, new_w), self.bbox_clip_border)
        ignore = resize_bboxes(ignore, sf, (new_h, new_w),
                               self.bbox_clip_border)
        # RandomCrop (transforms.py:651-760)
        crop, img_shape = (0, 0), (new_h, new_w, 3)
        if self.crop is not None:
            c = self.crop
            crop_h, crop_w = crop_size_draw((new_h, new_w), c['crop_size'],
                                            c['crop_type'], rng)
            assert crop_h > 0 and crop_w > 0
            off_h = int(rng.randint(0, max(new_h - crop_h, 0) + 1))
            off_w = int(rng.randint(0, max(new_w - crop_w, 0) + 1))
            crop = (off_h, off_w)
            img_shape = (min(off_h + crop_h, new_h) - off_h,
                         min(off_w + crop_w, new_w) - off_w, 3)
            ignore, valid = crop_bboxes(ignore, off_w, off_h, img_shape,
                                        c['bbox_clip_border'])
            ignore, keep_ig = ignore[valid, :], keep_ig[valid]
            boxes, valid = crop_bboxes(boxes, off_w, off_h, img_shape,
                                       c['bbox_clip_border'])
            if not valid.any() and not c['allow_negative_crop']:
                return dict(rejected=True, ori_shape=(h, w, 3))
            boxes, keep = boxes[valid, :], keep[valid]
        # RandomFlip (transforms.py:416-450)
        flip = False
        if self.flip_ratio > 0:
            flip = int(rng.choice(2, p=[self.flip_ratio,
                                        1 - self.flip_ratio])) == 0
        if flip:
            boxes = flip_bboxes(boxes, img_shape)
            ignore = flip_bboxes(ignore, img_shape)
        labels = None if gt_labels is None else \
            np.asarray(gt_labels, np.int64)[keep]
        return dict(rejected=False, ori_shape=(h, w, 3), img_shape=img_shape,
                    scale_factor=sf, flip=flip, scale=tuple(scale),
                    canvas=tuple(int(v) for v in canvas), window=window,
                    resized=(new_h, new_w), crop=crop, fill=self.expand_fill,
                    mode=None if mode is None else float(mode),
                    gt_bboxes=boxes, gt_labels=labels,
                    gt_bboxes_ignore=ignore, keep=keep, keep_ignore=keep_ig,
                    **extra)

    def transform_boxes(self, bboxes, plan):
        if 'gt_bboxes' in plan:
            raise ValueError('an augmented plan carries its own boxes '
                             "(plan['gt_bboxes'])")
        b = resize_bboxes(bboxes, plan['scale_factor'], plan['img_shape'],
                          self.bbox_clip_border)
        if plan['flip']:
            b = flip_bboxes(b, plan['img_shape'])
        return b

    @staticmethod
    def fill_descriptor(d, plan, shape):
        """The geometry of one plan -> an ``ld_image_aug_t`` (``data``,
        ``src_h`` / ``src_w`` and ``flip`` are the caller's).  A plain plan
        (no canvas, window or crop) gives the identity descriptor."""
        h, w = shape
        ch, cw, top, left = plan.get('canvas', (h, w, 0, 0))
        d.canvas_h, d.canvas_w, d.img_top, d.img_left = ch, cw, top, left
        d.win_y, d.win_x, d.win_h, d.win_w = plan.get('window',
                                                      (0, 0, ch, cw))
        d.new_h, d.new_w = plan.get('resized', plan['img_shape'][:2])
        d.crop_y, d.crop_x = plan.get('crop', (0, 0))
        d.out_h, d.out_w = plan['img_shape'][:2]
        fill = plan.get('fill', (0, 0, 0))
        for c in range(3):
            d.fill[c] = int(fill[c])

    @staticmethod
    def fill_photo_descriptor(d, plan, shape):
        """The variant for an ``ld_image_photo_t``: the same geometry, the
        fill as float32 and the draws of ``plan['photo']`` (missing or None:
        the identity chain without the HSV round trip).  The c_float fields
        round each drawn double to float32, as numpy does when the reference
        applies it to its float32 image."""
        fill = plan.get('fill', (0, 0, 0))
        DevicePipeline.fill_descriptor(d, dict(plan, fill=(0, 0, 0)), shape)
        for c in range(3):
            d.fill[c] = float(fill[c])
        ph = plan.get('photo')
        on = ph is not None
        get = (lambda k: ph[k]) if on else (lambda k: None)
        for field, key, flag, neutral in (
                ('delta', 'delta', 'do_brightness', 0.0),
                ('alpha', 'alpha', 'do_contrast', 1.0),
                ('saturation', 'saturation', 'do_saturation', 1.0),
                ('hue', 'hue', 'do_hue', 0.0)):
            v = get(key)
            setattr(d, flag, int(v is not None))
            setattr(d, field, neutral if v is None else float(v))
        d.contrast_mode = int(ph['mode']) if on else 0
        d.do_hsv = int(on)
        perm = (get('perm') or (0, 1, 2))
        if sorted(perm) != [0, 1, 2]:
            raise ValueError(f'perm {perm} is not a permutation of 0, 1, 2')
        for c in range(3):
            d.perm[c] = int(perm[c])
        d.reserved = 0

    def batch_shape(self, plans):
        """(Hpad, Wpad) of the batch tensor.  Pad(size_divisor) per image, then
        collate pads to the batch maximum; Pad(size) is that size for every
        batch, and an image larger than it raises (mmcv.impad asserts)."""
        if self.pad_size is not None:
            for p in plans:
                if p['img_shape'][0] > self.pad_size[0] or \
                        p['img_shape'][1] > self.pad_size[1]:
                    raise ValueError(
                        f"Pad(size={self.pad_size}): the image is "
                        f"{tuple(p['img_shape'][:2])}, larger than the pad "
                        'size')
            return self.pad_size
        div = self.size_divisor or 1
        return (max(_ceil_to(p['img_shape'][0], div) for p in plans),
                max(_ceil_to(p['img_shape'][1], div) for p in plans))

    # -- the batch ------------------------------------------------------------
    def __call__(self, images, gt_bboxes=None, gt_labels=None, rng=np.random,
                 plans=None, stream=None, gt_bboxes_ignore=None):
        from . import lib as L
        lib = L.get_lib()  # raises when the HIP library is missing
        if self.device.type != 'cuda':
            raise RuntimeError('DevicePipeline needs a GPU device')
        if self.augmented:
            return self._call_augmented(images, gt_bboxes, gt_labels, rng,
                                        plans, stream, gt_bboxes_ignore)
        N = len(images)
        shapes = [tuple(im.shape[:2]) for im in images]
        if plans is None:
            plans = self.plan(shapes, rng)
        div = self.size_divisor or 1
        # Pad(size_divisor) per image, then collate pads to the batch maximum
        Hpad = max(_ceil_to(p['img_shape'][0], div) for p in plans)
        Wpad = max(_ceil_to(p['img_shape'][1], div) for p in plans)
        # one pinned staging buffer -> one async H2D copy for all raw images
        sizes = [h * w * 3 for h, w in shapes]
        offs = np.concatenate([[0], np.cumsum([(s + 255) // 256 * 256
                                               for s in sizes])])
        stage = torch.empty(int(offs[-1]), dtype=torch.uint8, pin_memory=True)
        for im, o, s in zip(images, offs, sizes):
            t = im if isinstance(im, torch.Tensor) else torch.from_numpy(
                np.ascontiguousarray(im))
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
                raise ValueError('images must be uint8 HWC with 3 channels')
            stage[int(o):int(o) + s].copy_(t.reshape(-1))
        raw = stage.to(self.device, non_blocking=True)
        desc = (L.ImageT * N)()
        for i, (p, (h, w)) in enumerate(zip(plans, shapes)):
            desc[i].data = raw.data_ptr() + int(offs[i])
            desc[i].src_h, desc[i].src_w = h, w
            desc[i].new_h, desc[i].new_w = p['img_shape'][:2]
            desc[i].flip = int(p['flip'])
        dbytes = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8)
        ddesc = dbytes.pin_memory().to(self.device, non_blocking=True)
        out = torch.empty(N, 3, Hpad, Wpad, dtype=torch.float32,
                          device=self.device)
        s = stream if stream is not None else torch.cuda.current_stream(
            self.device)
        mean = (C.c_float * 3)(*self.mean.tolist())
        sinv = (C.c_float * 3)(*self.std_inv.tolist())
        L.check(lib.ld_preprocess_batch(ddesc.data_ptr(), N, Hpad, Wpad, mean,
                                        sinv, int(self.to_rgb), out.data_ptr(),
                                        s.cuda_stream), 'ld_preprocess_batch')
        metas = []
        for p in plans:
            pad_h = _ceil_to(p['img_shape'][0], div)
            pad_w = _ceil_to(p['img_shape'][1], div)
            metas.append(dict(
                ori_shape=p['ori_shape'], img_shape=p['img_shape'],
                pad_shape=(pad_h, pad_w, 3), scale_factor=p['scale_factor'],
                flip=p['flip'],
                flip_direction='horizontal' if p['flip'] else None,
                img_norm_cfg=dict(mean=self.mean, std=self.std,
                                  to_rgb=self.to_rgb)))
        result = dict(img=out, img_metas=metas)
        if gt_bboxes is not None:
            result['gt_bboxes'] = [
                torch.from_numpy(self.transform_boxes(b, p)).to(
                    self.device, non_blocking=True)
                for b, p in zip(gt_bboxes, plans)]
        if gt_bboxes_ignore is not None:  # transformed like gt_bboxes
            result['gt_bboxes_ignore'] = [
                torch.from_numpy(self.transform_boxes(b, p)).to(
                    self.device, non_blocking=True)
                for b, p in zip(gt_bboxes_ignore, plans)]
        if gt_labels is not None:
            result['gt_labels'] = [
                torch.as_tensor(np.asarray(l, np.int64)).to(
                    self.device, non_blocking=True) for l in gt_labels]
        return result

    def _call_augmented(self, images, gt_bboxes, gt_labels, rng, plans, stream,
                        gt_bboxes_ignore):
        """``__call__`` of a pipeline with augmentations: the same staging
        copy, then ONE ``ld_preprocess_batch_aug`` launch (float mode: ONE
        ``ld_preprocess_batch_photo`` launch); the annotations are the
        plans' own (transformed and selected by ``plan_image``)."""
        from . import lib as L
        lib = L.get_lib()  # raises when the HIP library is missing
        if self.device.type != 'cuda':
            raise RuntimeError('DevicePipeline needs a GPU device')
        N = len(images)
        shapes = [tuple(im.shape[:2]) for im in images]
        if plans is None:
            plans = self.plan(shapes, rng, gt_bboxes, gt_labels,
                              gt_bboxes_ignore)
        if any(p.get('rejected') for p in plans):
            raise ValueError(
                'a rejected plan (RandomCrop left no gt box) cannot be '
                'launched: the loader replaces such an image')
        Hpad, Wpad = self.batch_shape(plans)
        sizes = [h * w * 3 for h, w in shapes]
        offs = np.concatenate([[0], np.cumsum([(s + 255) // 256 * 256
                                               for s in sizes])])
        stage = torch.empty(int(offs[-1]), dtype=torch.uint8, pin_memory=True)
        for im, o, s in zip(images, offs, sizes):
            t = im if isinstance(im, torch.Tensor) else torch.from_numpy(
                np.ascontiguousarray(im))
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
                raise ValueError('images must be uint8 HWC with 3 channels')
            stage[int(o):int(o) + s].copy_(t.reshape(-1))
        raw = stage.to(self.device, non_blocking=True)
        desc = ((L.ImagePhotoT if self.float_mode else L.ImageAugT) * N)()
        fill = self.fill_photo_descriptor if self.float_mode else \
            self.fill_descriptor
        for i, (p, (h, w)) in enumerate(zip(plans, shapes)):
            desc[i].data = raw.data_ptr() + int(offs[i])
            desc[i].src_h, desc[i].src_w = h, w
            desc[i].flip = int(p['flip'])
            fill(desc[i], p, (h, w))
        dbytes = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8)
        ddesc = dbytes.pin_memory().to(self.device, non_blocking=True)
        out = torch.empty(N, 3, Hpad, Wpad, dtype=torch.float32,
                          device=self.device)
        s = stream if stream is not None else torch.cuda.current_stream(
            self.device)
        mean = (C.c_float * 3)(*self.mean.tolist())
        sinv = (C.c_float * 3)(*self.std_inv.tolist())
        pad = (C.c_float * 3)(*self.pad_val.tolist())
        entry = 'ld_preprocess_batch_photo' if self.float_mode else \
            'ld_preprocess_batch_aug'
        L.check(getattr(lib, entry)(
            ddesc.data_ptr(), N, Hpad, Wpad, mean, sinv, pad,
            int(self.to_rgb), out.data_ptr(), s.cuda_stream), entry)
        div = self.size_divisor or 1
        metas = []
        for p in plans:
            pad_shape = (_ceil_to(p['img_shape'][0], div),
                         _ceil_to(p['img_shape'][1], div), 3)
            if self.pad_size is not None:
                pad_shape = self.pad_size + (3,)
            metas.append(dict(
                ori_shape=p['ori_shape'], img_shape=p['img_shape'],
                pad_shape=pad_shape, scale_factor=p['scale_factor'],
                flip=p['flip'],
                flip_direction='horizontal' if p['flip'] else None,
                img_norm_cfg=dict(mean=self.mean, std=self.std,
                                  to_rgb=self.to_rgb)))
            if self.pad_size is not None:
                metas[-1]['pad_fixed_size'] = self.pad_size
        result = dict(img=out, img_metas=metas)

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(
                self.device, non_blocking=True)
        for key, given in (('gt_bboxes', gt_bboxes), ('gt_labels', gt_labels),
                           ('gt_bboxes_ignore', gt_bboxes_ignore)):
            if given is not None:
                result[key] = [dev(p[key]) for p in plans]
        return result


# ---------------------------------------------------------------------------
# samplers
# ---------------------------------------------------------------------------
class DistributedGroupSampler(torch.utils.data.Sampler):
    """mmdet/datasets/samplers/group_sampler.py:51-147.

    Images are grouped by aspect-ratio flag (``dataset.flag``: 1 when w / h > 1)
    so that a per-GPU batch pads little.  Per epoch, seeded by epoch + seed and
    identical on every rank: each group is permuted and padded (by repeating
    its own permuted order) to a multiple of samples_per_gpu * num_replicas;
    the concatenation is cut into samples_per_gpu chunks, the chunks are
    permuted, and rank r takes the r-th contiguous num_samples slice.
    """

    def __init__(self, dataset, samples_per_gpu=1, num_replicas=None,
                 rank=None, seed=0):
        if num_replicas is None or rank is None:
            import torch.distributed as dist
            on = dist.is_available() and dist.is_initialized()
            if num_replicas is None:
                num_replicas = dist.get_world_size() if on else 1
            if rank is None:
                rank = dist.get_rank() if on else 0
        self.dataset = dataset
        self.samples_per_gpu = samples_per_gpu
        self.num_replicas = num_replicas
        self.rank = rank
        self.epoch = 0
        self.seed = seed if seed is not None else 0
        if not hasattr(dataset, 'flag'):
            raise AttributeError('dataset needs an aspect-ratio `flag` array')
        self.flag = np.asarray(dataset.flag)
        self.group_sizes = np.bincount(self.flag)
        unit = samples_per_gpu * num_replicas
        self._padded = [int(math.ceil(int(n) / unit)) * unit
                        for n in self.group_sizes]
        self.total_size = sum(self._padded)
        self.num_samples = self.total_size // num_replicas

    def epoch_indices(self):
        """All ranks' indices for the current epoch (total_size long)."""
        g = torch.Generator()
        g.manual_seed(self.epoch + self.seed)
        order = []
        for gid, (size, padded) in enumerate(zip(self.group_sizes,
                                                 self._padded)):
            size = int(size)
            if size == 0:
                continue
            members = np.flatnonzero(self.flag == gid)
            perm = members[torch.randperm(size, generator=g).numpy()]
            reps = np.tile(perm, padded // size + 1)[:padded]
            order.append(reps)
        order = np.concatenate(order) if order else np.zeros(0, np.int64)
        spg = self.samples_per_gpu
        chunks = torch.randperm(len(order) // spg, generator=g).numpy()
        return order.reshape(-1, spg)[chunks].reshape(-1).astype(np.int64)

    def __iter__(self):
        lo = self.num_samples * self.rank
        return iter(self.epoch_indices()[lo:lo + self.num_samples].tolist())

    def __len__(self):
        return self.num_samples

    def set_epoch(self, epoch):
        self.epoch = epoch


class GroupSampler(torch.utils.data.Sampler):
    """mmdet/datasets/samplers/group_sampler.py:10-48 (the non-distributed
    sampler): numpy's global RNG, drawn in the reference's order."""

    def __init__(self, dataset, samples_per_gpu=1):
        if not hasattr(dataset, 'flag'):
            raise AttributeError('dataset needs an aspect-ratio `flag` array')
        self.dataset = dataset
        self.samples_per_gpu = samples_per_gpu
        self.flag = np.asarray(dataset.flag).astype(np.int64)
        self.group_sizes = np.bincount(self.flag)
        self.num_samples = sum(
            int(math.ceil(int(n) / samples_per_gpu)) * samples_per_gpu
            for n in self.group_sizes)

    def __iter__(self):
        spg = self.samples_per_gpu
        parts = []
        for gid, size in enumerate(self.group_sizes):
            if size == 0:
                continue
            members = np.flatnonzero(self.flag == gid)
            np.random.shuffle(members)
            extra = int(math.ceil(int(size) / spg)) * spg - len(members)
            parts.append(np.concatenate(
                [members, np.random.choice(members, extra)]))
        flat = np.concatenate(parts)
        chunks = np.random.permutation(range(len(flat) // spg))
        return iter(flat.reshape(-1, spg)[chunks].reshape(-1).astype(
            np.int64).tolist())

    def __len__(self):
        return self.num_samples
