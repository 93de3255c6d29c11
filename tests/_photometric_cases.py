"""What tools/gen_golden_photometric.py runs the reference's own classes on
and tests/test_photometric_host.py replays: the 8 x 8 palette image, the boxes
and the two toy pipelines.  The seeds are the tool's (it adds seeds until the
edges the issue names are reached) and are read back from the golden file.
"""
import numpy as np

# (B, G, R) of the pixels the image is there for
PALETTE = [
    (128, 128, 128),   # grey: S = 0, the HSV -> BGR shortcut
    (0, 0, 0),         # black: V = 0
    (255, 0, 0), (0, 255, 0), (0, 0, 255),   # the primaries
    (200, 200, 40),    # B == G tie at the maximum
    (60, 170, 170),    # G == R tie at the maximum
    (90, 20, 90),      # B == R tie at the maximum
    (254, 253, 255),   # near white
    (3, 1, 2),         # dark
    (10, 0, 255),      # H just under 360: wraps with a positive hue delta
    (0, 6, 250),       # H just over 0: wraps with a negative hue delta
]


def palette_image(h=8, w=8, seed=0):
    """uint8 (h, w, 3) BGR: the palette first, seeded noise after it."""
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (h * w, 3)).astype(np.uint8)
    img[:len(PALETTE)] = np.asarray(PALETTE, np.uint8)
    return img.reshape(h, w, 3)


BOXES = np.array([[1, 1, 6, 5], [3, 2, 8, 8]], np.float32)
LABELS = np.array([3, 7], np.int64)
IGNORE = np.zeros((0, 4), np.float32)

PMD = dict(type='PhotoMetricDistortion', brightness_delta=32,
           contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5),
           hue_delta=18)
LOAD = [dict(type='LoadImageFromFile', to_float32=True),
        dict(type='LoadAnnotations', with_bbox=True)]
BUNDLE = [dict(type='DefaultFormatBundle'),
          dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]
SSD_NORM = dict(mean=[123.675, 116.28, 103.53], std=[1, 1, 1], to_rgb=True)
YOLO_NORM = dict(mean=[0, 0, 0], std=[255., 255., 255.], to_rgb=True)

# configs/ssd/ssd300_coco.py at toy size: the same steps in the same order
SSD = [
    PMD,
    dict(type='Expand', mean=SSD_NORM['mean'], to_rgb=SSD_NORM['to_rgb'],
         ratio_range=(1, 4)),
    dict(type='MinIoURandomCrop', min_ious=(0.1, 0.3, 0.5, 0.7, 0.9),
         min_crop_size=0.3),
    dict(type='Resize', img_scale=(12, 12), keep_ratio=False),
    dict(type='Normalize', **SSD_NORM),
    dict(type='RandomFlip', flip_ratio=0.5),
]
# configs/yolo/yolov3_d53_mstrain-416_273e_coco.py at toy size
YOLO = [
    dict(type='PhotoMetricDistortion'),
    dict(type='Expand', mean=YOLO_NORM['mean'], to_rgb=YOLO_NORM['to_rgb'],
         ratio_range=(1, 2)),
    dict(type='MinIoURandomCrop', min_ious=(0.4, 0.5, 0.6, 0.7, 0.8, 0.9),
         min_crop_size=0.3),
    dict(type='Resize', img_scale=[(10, 10), (14, 14)], keep_ratio=True),
    dict(type='RandomFlip', flip_ratio=0.5),
    dict(type='Normalize', **YOLO_NORM),
    dict(type='Pad', size_divisor=4),
]
FULL = dict(ssd=SSD, yolo=YOLO)

# the reference configs whose train_pipeline the golden stores (settings only)
STOCK = [
    'configs/ssd/ssd300_coco.py',
    'configs/ssd/ssd512_coco.py',
    'configs/pascal_voc/ssd300_voc0712.py',
    'configs/pascal_voc/ssd512_voc0712.py',
    'configs/yolo/yolov3_d53_320_273e_coco.py',
    'configs/yolo/yolov3_d53_mstrain-416_273e_coco.py',
    'configs/yolo/yolov3_d53_mstrain-608_273e_coco.py',
    'configs/_base_/datasets/wider_face.py',
    'configs/legacy_1.x/ssd300_coco_v1.py',
    'configs/yolact/yolact_r50_1x8_coco.py',
]


def from_json(obj):
    """A pipeline read back from JSON: a list of numbers was a tuple or is
    used as one (img_scale, mean); lists of anything else stay lists."""
    if isinstance(obj, dict):
        return {k: from_json(v) for k, v in obj.items()}
    if isinstance(obj, list):
        if obj and all(isinstance(v, (int, float)) and
                       not isinstance(v, bool) for v in obj):
            return tuple(obj)
        return [from_json(v) for v in obj]
    return obj


def photo_of(gold, name):
    """The stored draws of case ``name`` as ``photometric_draw`` returns
    them."""
    flags = gold[name + '_flags']   # brightness, contrast, sat, hue, perm
    vals = gold[name + '_draws']    # delta, alpha, saturation, hue (float64)
    keys = ('delta', 'alpha', 'saturation', 'hue')
    d = {k: (float(v) if f else None)
         for k, v, f in zip(keys, vals, flags[:4])}
    d['mode'] = int(gold[name + '_mode'])
    d['perm'] = tuple(int(v) for v in gold[name + '_perm']) if flags[4] \
        else None
    return d
