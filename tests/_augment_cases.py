"""The seeded cases of the augmentation plans: tools/gen_golden_augment.py runs
the reference's own transform classes on them under ``np.random.seed(seed)``
and stores what they return in tests/golden/augment.npz;
tests/test_augment_host.py builds ``DevicePipeline.from_cfg(steps)`` from the
same table and compares its plans.

A case is ``(name, seed, (h, w), boxes, labels, ignore, steps)``; ``steps`` is
a reference ``train_pipeline`` list without the loading / formatting entries.
What each case is there for is in its name; the generator asserts the edges
on the reference's own outputs (``check_coverage``), so a seed that stops
covering its edge fails the regeneration instead of passing silently.
"""
import numpy as np

NORM = dict(type='Normalize', mean=[123.675, 116.28, 103.53],
            std=[58.395, 57.12, 57.375], to_rgb=True)
FLIP = dict(type='RandomFlip', flip_ratio=0.5)


def jitter_crop(crop=None, pad=None, **resize):
    """The nas_fpn recipe at toy size: scale jitter, fixed crop, fixed pad."""
    return [
        dict(dict(type='Resize', img_scale=(160, 160), ratio_range=(0.8, 1.2),
                  keep_ratio=True), **resize),
        dict(dict(type='RandomCrop', crop_size=(64, 64)), **(crop or {})),
        FLIP, NORM,
        dict(type='Pad', **(pad or dict(size=(64, 64)))),
    ]


def zoom(expand=None, min_iou=None, tail=()):
    """The VOC / SSD zoom-out, zoom-in pair in front of a fixed-size resize."""
    steps = []
    if expand is not None:
        steps.append(dict(dict(type='Expand', mean=NORM['mean'], to_rgb=True,
                               ratio_range=(1, 4)), **expand))
    if min_iou is not None:
        steps.append(dict(dict(type='MinIoURandomCrop',
                               min_ious=(0.1, 0.3, 0.5, 0.7, 0.9),
                               min_crop_size=0.3), **min_iou))
    return steps + [dict(type='Resize', img_scale=(64, 64), keep_ratio=False),
                    *tail, NORM, FLIP]


def _f(rows):
    return np.asarray(rows, np.float32).reshape(-1, 4)


BOXES = _f([[12, 20, 90, 77], [60, 10, 100, 95], [5.7, 40.2, 48.9, 88.5]])
LABELS = np.array([6, 14, 11], np.int64)
IGNORE = _f([[1, 1, 30, 30]])
NONE = _f([])
CORNER = _f([[2, 2, 9, 8]])          # a crop rarely keeps it
FULL = _f([[0, 0, 130, 100]])        # a patch of IoU >= 0.9 exists

RANGE_PAD = dict(size_divisor=32)

CASES = [
    # -- Resize(ratio_range) -> RandomCrop -> RandomFlip -> Pad(size) ---------
    ('jitter_s0', 0, (100, 130), BOXES, LABELS, IGNORE, jitter_crop()),
    ('jitter_s1', 1, (100, 130), BOXES, LABELS, IGNORE, jitter_crop()),
    ('jitter_s2', 2, (120, 80), BOXES[:2], LABELS[:2], NONE, jitter_crop()),
    ('jitter_rejected', 3, (100, 130), CORNER, LABELS[:1], IGNORE,
     jitter_crop()),
    ('jitter_no_boxes_rejected', 4, (100, 130), NONE, LABELS[:0], NONE,
     jitter_crop()),
    ('jitter_small_image', 5, (24, 40), _f([[2, 2, 30, 20]]), LABELS[:1],
     NONE, jitter_crop(img_scale=(48, 48))),
    ('jitter_negative_empty', 3, (100, 130), CORNER, LABELS[:1], IGNORE,
     jitter_crop(crop=dict(allow_negative_crop=True))),
    ('jitter_no_clip', 6, (100, 130), BOXES, LABELS, IGNORE,
     jitter_crop(crop=dict(bbox_clip_border=False))),
    # -- the other crop types, Pad(size_divisor) -------------------------------
    ('crop_absolute_range', 7, (100, 130), BOXES, LABELS, IGNORE,
     jitter_crop(crop=dict(crop_size=(30, 50), crop_type='absolute_range'),
                 pad=RANGE_PAD)),
    ('crop_relative', 8, (100, 130), BOXES, LABELS, IGNORE,
     jitter_crop(crop=dict(crop_size=(0.6, 0.7), crop_type='relative'),
                 pad=RANGE_PAD)),
    ('crop_relative_range', 9, (100, 130), BOXES, LABELS, IGNORE,
     jitter_crop(crop=dict(crop_size=(0.5, 0.4), crop_type='relative_range'),
                 pad=RANGE_PAD)),
    ('crop_value_scales', 10, (100, 130), BOXES, LABELS, NONE,
     jitter_crop(img_scale=[(96, 64), (80, 48)], ratio_range=None,
                 multiscale_mode='value',
                 crop=dict(crop_size=(40, 56)), pad=dict(size=(64, 64),
                                                         pad_val=1.5))),
]

# -- Expand -> MinIoURandomCrop -> Resize(keep_ratio=False) -> RandomFlip ------
# the seeds were searched so that the last mode drawn covers (1, 0.1, 0.3, 0.5,
# 0.7, 0.9, 0) and Expand is both taken and skipped
ZOOM_SEEDS = (1, 8, 9, 10, 21)
for _s in ZOOM_SEEDS:
    CASES.append((f'zoom_s{_s}', _s, (100, 130), BOXES, LABELS, IGNORE,
                  zoom(expand={}, min_iou={})))
MINIOU_FULL_SEEDS = (0, 1, 3, 5, 9, 10)
for _s in MINIOU_FULL_SEEDS:
    CASES.append((f'miniou_full_s{_s}', _s, (100, 130), FULL, LABELS[:1],
                  NONE, zoom(min_iou={})))
CASES += [
    # seed 9 accepts the patch x 57 .. 129, y 24 .. 89 in mode 0; the second
    # box has its centre at x = 57 exactly: `center > patch[0]` drops it
    ('miniou_center_on_border', 9, (100, 130),
     _f([[60, 30, 120, 80], [40, 30, 74, 80]]), LABELS[:2], NONE,
     zoom(min_iou={})),
    ('miniou_no_clip', 9, (100, 130), BOXES, LABELS, IGNORE,
     zoom(min_iou=dict(bbox_clip_border=False))),
    ('miniou_no_boxes', 3, (100, 130), NONE, LABELS[:0], NONE,
     zoom(expand=dict(prob=1.0, ratio_range=(2, 3)), min_iou={})),
    # everything at once: zoom, then jitter-free crop and a fixed pad
    ('all_steps', 9, (100, 130), BOXES, LABELS, IGNORE,
     zoom(expand=dict(prob=1.0), min_iou={},
          tail=(dict(type='RandomCrop', crop_size=(48, 40),
                     allow_negative_crop=True),)) +
     [dict(type='Pad', size=(64, 64))]),
    ('jitter_negative_ignore_kept', 9, (100, 130), CORNER, LABELS[:1], IGNORE,
     jitter_crop(crop=dict(allow_negative_crop=True))),
]
