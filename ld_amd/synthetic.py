"""Deterministic synthetic inputs for the LD train step.

There is no dataset and no checkpoint on the GPU box, so the bench, the smoke
test and the parity fixtures all use:

* images: ~N(0,1) (normalised-image statistics), columns past ``img_shape``
  zero-filled exactly as ``Pad(size_divisor=32)`` would
  (reference: mmdet/datasets/pipelines/transforms.py:481-509);
* GT boxes: centre uniform in the image, ``w, h = 16 + 584 u^3`` (small-skewed, like a log-uniform law)
  clipped to the image, non-integer xyxy fp32 (avoids ATSS distance ties),
  labels ``randint(0, 80)``;
* weights: :func:`seeded_state_dict` -- every tensor of a ``state_dict`` is
  filled from a CPU ``torch.Generator`` whose seed is derived from the *key
  name*, so the reference model (under ``oracle/ref_shim``) and the HIP model
  receive bit-identical parameters as long as their key names agree (which is
  itself part of the drop-in contract, SURVEY.md section 5 "checkpoint").

Everything is generated on the CPU generator (bit-reproducible across
machines for one torch build) and moved to the device afterwards.
"""
import math
import zlib
from collections import OrderedDict

import numpy as np
import torch

__all__ = ['synthetic_batch', 'seeded_state_dict', 'synthetic_head_inputs']


def _gen(seed):
    g = torch.Generator(device='cpu')
    g.manual_seed(int(seed))
    return g


def _normal(shape, gen):
    """~N(0, 1) as a scaled sum of three uniforms.  Only IEEE-exact ops
    (rand, +, *) are used anywhere in this module: torch.randn / exp / log go
    through vendor-specific SIMD math and differ by an ulp between the build
    container's Xeon and the GPU box's EPYC, which would make 'identical
    inputs' not identical."""
    u = torch.rand(shape, generator=gen) + torch.rand(shape, generator=gen) \
        + torch.rand(shape, generator=gen)
    return (u - 1.5) * 2.0


def synthetic_boxes(num_gt, img_h, img_w, gen, min_size=16.0, max_size=600.0):
    """(num_gt, 4) xyxy fp32 boxes, (num_gt,) int64 labels."""
    cx = torch.rand(num_gt, generator=gen) * img_w
    cy = torch.rand(num_gt, generator=gen) * img_h
    # sizes skewed to small boxes (u^3 stands in for a log-uniform law)
    uw = torch.rand(num_gt, generator=gen)
    uh = torch.rand(num_gt, generator=gen)
    w = min_size + (max_size - min_size) * (uw * uw * uw)
    h = min_size + (max_size - min_size) * (uh * uh * uh)
    x1 = (cx - w / 2).clamp(0.0, img_w - 2.0)
    y1 = (cy - h / 2).clamp(0.0, img_h - 2.0)
    x2 = torch.maximum((cx + w / 2).clamp(0.0, float(img_w)), x1 + 1.7)
    y2 = torch.maximum((cy + h / 2).clamp(0.0, float(img_h)), y1 + 1.3)
    boxes = torch.stack([x1, y1, x2, y2], dim=1).float()
    # knock the coordinates off any integer/half-integer lattice
    boxes = boxes + torch.rand(num_gt, 4, generator=gen) * 0.37 + 0.011
    labels = torch.randint(0, 80, (num_gt, ), generator=gen)
    return boxes.contiguous(), labels


def synthetic_batch(num_imgs=2,
                    img_shape=(800, 1333),
                    pad_shape=(800, 1344),
                    num_gt=7,
                    seed=1234,
                    device='cpu'):
    """One LD training batch in the mmdet batch contract
    (reference: mmdet/models/detectors/kd_one_stage.py:46-65).

    ``num_gt`` may be an int or a per-image list.
    """
    gen = _gen(seed)
    h, w = img_shape
    hp, wp = pad_shape
    img = torch.zeros(num_imgs, 3, hp, wp)
    img[:, :, :h, :w] = _normal((num_imgs, 3, h, w), gen)
    if isinstance(num_gt, int):
        num_gt = [num_gt] * num_imgs
    gt_bboxes, gt_labels = [], []
    for g in num_gt:
        b, l = synthetic_boxes(g, h, w, gen)
        gt_bboxes.append(b.to(device))
        gt_labels.append(l.to(device))
    img_metas = [
        dict(
            img_shape=(h, w, 3),
            pad_shape=(hp, wp, 3),
            ori_shape=(h, w, 3),
            scale_factor=1.0,
            flip=False) for _ in range(num_imgs)
    ]
    return dict(
        img=img.to(device),
        img_metas=img_metas,
        gt_bboxes=gt_bboxes,
        gt_labels=gt_labels)


def _key_seed(key, seed):
    return (zlib.crc32(key.encode()) ^ (seed * 2654435761)) & 0x7FFFFFFF


def seeded_state_dict(reference_sd, seed=0, reg_std=0.05, cls_std=0.02):
    """Fill every entry of ``reference_sd`` (name -> tensor, used for shape and
    dtype only) with deterministic values keyed on the entry's *name*.

    The value distributions keep activations of a randomly initialised
    ResNet-FPN-GFL stack well conditioned (no overflow, non-degenerate
    softmaxes) so fp32 parity thresholds stay meaningful.
    """
    out = OrderedDict()
    for key, ref in reference_sd.items():
        g = _gen(_key_seed(key, seed))
        shape = tuple(ref.shape)
        leaf = key.rsplit('.', 1)[-1]
        parent = key.rsplit('.', 2)[-2] if key.count('.') >= 1 else ''
        if leaf == 'num_batches_tracked':
            v = torch.zeros(shape, dtype=ref.dtype)
        elif leaf == 'running_mean':
            v = torch.rand(shape, generator=g) * 0.2 - 0.1
        elif leaf == 'running_var':
            v = torch.rand(shape, generator=g) * 0.4 + 0.8
        elif leaf == 'project':  # Integral buffer, gfl_head.py:29-30
            v = torch.linspace(0, shape[0] - 1, shape[0])
        elif leaf == 'scale':  # mmcv Scale
            v = torch.rand(shape, generator=g) * 0.4 + 0.8
        elif len(shape) == 4:  # conv weight
            fan_in = shape[1] * shape[2] * shape[3]
            if parent == 'gfl_cls':
                std = cls_std
            elif parent in ('gfl_reg', 'reg_conf'):
                std = reg_std
            elif 'lateral_convs' in key:
                std = 0.5 * math.sqrt(1.0 / fan_in)
            elif 'fpn_convs' in key:
                std = math.sqrt(1.0 / fan_in)
            else:
                std = math.sqrt(2.0 / fan_in)
            v = _normal(shape, g) * std
        elif leaf == 'weight':  # norm affine
            block = key.rsplit('.', 2)[0]
            last = 'bn3' if block + '.bn3.weight' in reference_sd else 'bn2'
            is_last_bn = ('.layer' in key and parent == last) or \
                key.endswith('downsample.1.weight')
            if is_last_bn:
                v = torch.rand(shape, generator=g) * 0.2 + 0.2
            else:
                v = torch.rand(shape, generator=g) * 0.4 + 0.8
        elif leaf == 'bias':
            if parent == 'gfl_cls':
                v = torch.rand(shape, generator=g) * 0.5 - 3.5
            else:
                v = torch.rand(shape, generator=g) * 0.2 - 0.1
        else:
            v = _normal(shape, g) * 0.1
        out[key] = v.to(ref.dtype).reshape(shape)
    return out


def level_shapes(pad_shape, strides=(8, 16, 32, 64, 128)):
    """Feature-map sizes of FPN P3..P7 for a padded input. P3..P5 follow the
    ResNet stride-2 convs (ceil for even pads), P6/P7 the 3x3 s2 pad-1 extra
    convs (reference: mmdet/models/necks/fpn.py:129-160)."""
    hp, wp = pad_shape

    def down(x):  # 3x3 stride 2 pad 1  ==  ceil(x / 2)
        return (x + 1) // 2

    h, w = hp, wp
    sizes = []
    for i in range(7):
        h, w = down(h), down(w)
        if i >= 2:
            sizes.append((h, w))
    assert len(sizes) == len(strides)
    return sizes


def synthetic_head_inputs(num_imgs,
                          featmap_sizes,
                          seed=0,
                          num_classes=80,
                          reg_max=16,
                          feat_channels=256,
                          device='cpu',
                          num_anchors=1):
    """Random student/teacher head outputs and FPN features for loss-block
    parity tests: logits ~ 3*randn (reg), cls ~ 1.2*randn - 4, features ~ randn.
    ``num_anchors`` > 1: anchor-major channel blocks (RetinaGFLHead).

    Returns dict of lists (one tensor per level, NCHW).
    """
    gen = _gen(seed)
    out = dict(cls=[], reg=[], t_cls=[], t_reg=[], x=[], t_x=[])
    na = num_anchors
    for (h, w) in featmap_sizes:
        out['cls'].append(
            _normal((num_imgs, na * num_classes, h, w), gen) * 1.2 - 4.0)
        out['reg'].append(
            _normal((num_imgs, na * 4 * (reg_max + 1), h, w), gen) * 3.0)
        out['t_cls'].append(
            _normal((num_imgs, na * num_classes, h, w), gen) * 1.2 - 4.0)
        out['t_reg'].append(
            _normal((num_imgs, na * 4 * (reg_max + 1), h, w), gen) * 3.0)
        out['x'].append(
            _normal((num_imgs, feat_channels, h, w), gen))
        out['t_x'].append(
            _normal((num_imgs, feat_channels, h, w), gen))
    return {k: [t.to(device) for t in v] for k, v in out.items()}


# ---------------------------------------------------------------------------
# inference cases (GFLHead.get_bboxes parity, tests/golden/infer.npz)
# ---------------------------------------------------------------------------
# name, pad, img_shapes, scale_factors, seed, nms_pre, cls_scale, cls_shift,
# store_all.  The class logits of synthetic_head_inputs are re-scaled to
# cls * cls_scale + cls_shift so the number of (anchor, class) pairs above
# score_thr = 0.05 lands on either side of batched_nms' split_thr = 10000.
INFER_CASES = [
    ('small', (128, 160), [(128, 160, 3), (120, 150, 3)],
     [[1.0, 1.0, 1.0, 1.0], [1.25, 1.25, 1.25, 1.25]], 51, 1000, 1.25, -1.0,
     True),
    ('small_topk', (128, 160), [(128, 160, 3), (100, 140, 3)],
     [[0.5, 0.5, 0.5, 0.5], [2.0, 2.0, 2.0, 2.0]], 52, 50, 1.25, -1.0, True),
    ('c2', (800, 1344), [(800, 1333, 3), (750, 1344, 3)],
     [[1.6675, 1.6675, 1.6675, 1.6675], [1.0, 1.0, 1.0, 1.0]], 53, 1000, 1.25,
     -1.0, False),
    ('c2_dense', (800, 1344), [(800, 1333, 3), (800, 1344, 3)],
     [[1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0]], 54, 1000, 1.0, 0.0, False),
]


def infer_inputs_clustered(pad, num_imgs, seed, device='cpu'):
    """Head outputs whose neighbouring anchors predict nearly the same box (one
    sharp distribution per side shared by all positions of a level plus small
    noise), so that score voting has clusters to average: the case the
    'voting_cluster_diounms' branch exists for.  IEEE-exact ops only."""
    sizes = level_shapes(pad)
    gen = _gen(seed)
    bins = torch.arange(17, dtype=torch.float32)
    cls, reg = [], []
    for li, (h, w) in enumerate(sizes):
        c = _normal((num_imgs, 80, h, w), gen) * 1.25 - 6.0
        c[:, 3] += 5.0   # two classes fire on every anchor: dense clusters of
        c[:, 17] += 5.0  # near-identical same-class boxes
        cls.append(c)
        centre = torch.tensor([5.0, 4.0, 6.0, 5.0]) + float(li % 2)
        peak = -((bins[None, :] - centre[:, None]) ** 2) * 2.0  # (4, 17)
        base = peak.reshape(1, 68, 1, 1).expand(num_imgs, 68, h, w)
        reg.append((base + _normal((num_imgs, 68, h, w), gen) * 0.3)
                   .contiguous())
    return [c.to(device) for c in cls], [r.to(device) for r in reg]


def synthetic_centerness(num_imgs, featmap_sizes, seed=0, device='cpu'):
    """Centerness logits ~ 1.5 * randn for the ATSS heads (a separate stream:
    the draw order of synthetic_head_inputs is part of the older goldens)."""
    gen = _gen(seed + 7919)
    return [(_normal((num_imgs, 1, h, w), gen) * 1.5).to(device)
            for (h, w) in featmap_sizes]


def grad_probe(n, seed):
    """Deterministic pseudo-random direction in [-0.5, 0.5)^n (integer hash,
    exact on every platform): gradient fingerprints dot(grad, probe) that --
    unlike a norm -- see sign flips, permutations and transposed layouts."""
    import numpy as np
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(seed * 40503 + 12345)) & \
        np.uint64(0xFFFFFFFF)
    h = (h ^ (h >> np.uint64(15))) * np.uint64(2246822519) & np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(13))
    return h.astype(np.float64) / 4294967296.0 - 0.5


def grad_sample_idx(n, k=256, seed=7):
    """k deterministic flat indices into a gradient of n elements (all of them
    when n <= k): integer hash, exact on every platform, so the fixture and the
    test address the same elements without storing the indices."""
    import numpy as np
    if n <= k:
        return np.arange(n, dtype=np.int64)
    i = np.arange(k, dtype=np.uint64)
    h = (i * np.uint64(2246822519) + np.uint64(seed * 3266489917 % (1 << 32))) & \
        np.uint64(0xFFFFFFFF)
    h = (h ^ (h >> np.uint64(16))) * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(13))
    return (h % np.uint64(n)).astype(np.int64)


VOTING_CASES = [
    # name, pad, img_shapes, scale factors, seed, nms_pre, clustered
    ('v_small', (128, 160), [(128, 160, 3), (120, 150, 3)],
     [[1.0, 1.0, 1.0, 1.0], [1.25, 1.25, 1.25, 1.25]], 61, 1000, False),
    ('v_clustered', (128, 160), [(128, 160, 3), (128, 150, 3)],
     [[1.0, 1.0, 1.0, 1.0], [2.0, 2.0, 2.0, 2.0]], 62, 1000, True),
    ('v_clustered_topk', (256, 320), [(256, 320, 3), (250, 300, 3)],
     [[1.0, 1.0, 1.0, 1.0], [0.5, 0.5, 0.5, 0.5]], 63, 60, True),
]


def voting_inputs(case, device='cpu'):
    import numpy as np
    name, pad, img_shapes, sfs, seed, nms_pre, clustered = case
    if clustered:
        cls, reg = infer_inputs_clustered(pad, len(img_shapes), seed, device)
    else:
        hi = synthetic_head_inputs(len(img_shapes), level_shapes(pad),
                                   seed=seed)
        cls = [(c * 1.25 - 1.0).to(device) for c in hi['cls']]
        reg = [r.to(device) for r in hi['reg']]
    metas = [dict(img_shape=s_, pad_shape=tuple(pad) + (3, ),
                  scale_factor=np.array(f, dtype=np.float32))
             for s_, f in zip(img_shapes, sfs)]
    return cls, reg, metas


def infer_inputs(case, device='cpu'):
    """(cls_scores, bbox_preds, img_metas) of an INFER_CASES row."""
    import numpy as np
    name, pad, img_shapes, sfs, seed, nms_pre, cs, sh, store = case
    sizes = level_shapes(pad)
    hi = synthetic_head_inputs(len(img_shapes), sizes, seed=seed)
    cls = [(c * cs + sh).to(device) for c in hi['cls']]
    reg = [r.to(device) for r in hi['reg']]
    metas = [dict(img_shape=s_, pad_shape=tuple(pad) + (3, ),
                  scale_factor=np.array(f, dtype=np.float32))
             for s_, f in zip(img_shapes, sfs)]
    return cls, reg, metas


# ---------------------------------------------------------------------------
# GFocalHead.get_bboxes (GFLv2: the maps already hold probabilities, 81
# channels because use_sigmoid=False -> cls_out_channels = num_classes + 1)
# ---------------------------------------------------------------------------
INFER_V2_CASES = ['small', 'small_topk', 'c2']


def infer_inputs_prob(case, device='cpu'):
    """(cls_scores as probabilities (N, 81, H, W), bbox_preds, img_metas) of an
    INFER_CASES row: sigmoid of 81-channel synthetic logits (the sigmoid is
    part of the INPUT here, both paths receive the same floats)."""
    import numpy as np
    name, pad, img_shapes, sfs, seed, nms_pre, cs, sh, store = case
    sizes = level_shapes(pad)
    hi = synthetic_head_inputs(len(img_shapes), sizes, seed=seed + 1000,
                               num_classes=81)
    cls = [torch.sigmoid(c * cs + sh).to(device) for c in hi['cls']]
    reg = [r.to(device) for r in hi['reg']]
    metas = [dict(img_shape=s_, pad_shape=tuple(pad) + (3, ),
                  scale_factor=np.array(f, dtype=np.float32))
             for s_, f in zip(img_shapes, sfs)]
    return cls, reg, metas


def infer_inputs_retina(case, device='cpu'):
    """(cls_scores (N, 9 * 80, H, W), bbox_preds (N, 9 * 68, H, W), img_metas)
    of an INFER_CASES row for the 9-anchor RetinaGFL head."""
    import numpy as np
    name, pad, img_shapes, sfs, seed, nms_pre, cs, sh, store = case
    sizes = level_shapes(pad)
    hi = synthetic_head_inputs(len(img_shapes), sizes, seed=seed + 2000,
                               num_anchors=9)
    cls = [(c * cs + sh).to(device) for c in hi['cls']]
    reg = [r.to(device) for r in hi['reg']]
    metas = [dict(img_shape=s_, pad_shape=tuple(pad) + (3, ),
                  scale_factor=np.array(f, dtype=np.float32))
             for s_, f in zip(img_shapes, sfs)]
    return cls, reg, metas


# ---------------------------------------------------------------------------
# test-time augmentation (BBoxTestMixin.aug_test_bboxes, tests/golden/augtest.npz)
# ---------------------------------------------------------------------------
# name, head kind, views, seed, nms_pre, cls_scale, cls_shift, nms type, store.
# A view is (pad, img_shape, scale factor, flip, flip_direction): the image is
# one original picture seen at the view's scale, so that img_shape = round(
# original * scale_factor).  Every view gets its own seeded head maps.
_HFLIP = [((128, 160), (128, 160, 3), 1.0, False, None),
          ((128, 160), (128, 160, 3), 1.0, True, 'horizontal')]
AUG_CASES = [
    ('gfl_small', 'gfl', _HFLIP, 71, 1000, 1.25, -1.0, 'nms', True),
    ('gfl_split', 'gfl',
     [((640, 1024), (600, 1000, 3), 1.25, False, None),
      ((640, 1024), (600, 1000, 3), 1.25, True, 'horizontal'),
      ((320, 512), (300, 500, 3), 0.625, False, None),
      ((320, 512), (300, 500, 3), 0.625, True, 'horizontal')],
     72, 1000, 1.0, 0.0, 'nms', False),
    ('gfl_flips', 'gfl',
     [((128, 160), (120, 150, 3), 1.25, False, None),
      ((128, 160), (120, 150, 3), 1.25, True, 'horizontal'),
      ((128, 160), (120, 150, 3), 1.25, True, 'vertical'),
      ((128, 160), (120, 150, 3), 1.25, True, 'diagonal')],
     73, 50, 1.25, -1.0, 'nms', True),
    ('gfl_voting', 'gfl_clustered', _HFLIP, 74, 1000, 1.0, 0.0,
     'voting_cluster_diounms', True),
    ('atss_small', 'atss', _HFLIP, 75, 1000, 1.25, -1.0, 'nms', True),
    ('fcos_small', 'fcos', _HFLIP, 76, 1000, 1.25, -1.0, 'nms', True),
    ('v2_small', 'v2', _HFLIP, 77, 1000, 1.25, -1.0, 'nms', True),
    ('retina_small', 'retina', _HFLIP, 78, 1000, 1.25, -1.0, 'nms', True),
]


def aug_view_outs(case, v, device='cpu'):
    """The head outputs (the tuple the head's forward returns) of view ``v`` of
    an AUG_CASES row, for one image."""
    name, kind, views, seed, nms_pre, cs, sh, nms_type, store = case
    pad = views[v][0]
    sizes = level_shapes(pad)
    vs = seed * 100 + v
    if kind == 'gfl_clustered':
        cls, reg = infer_inputs_clustered(pad, 1, vs, device)
        return cls, reg
    hi = synthetic_head_inputs(1, sizes, seed=vs,
                               num_classes=81 if kind == 'v2' else 80,
                               num_anchors=9 if kind == 'retina' else 1)
    cls = [c * cs + sh for c in hi['cls']]
    if kind == 'v2':
        cls = [torch.sigmoid(c) for c in cls]
    out = ([c.to(device) for c in cls], [r.to(device) for r in hi['reg']])
    if kind in ('atss', 'fcos'):
        out += (synthetic_centerness(1, sizes, seed=vs, device=device), )
    if kind == 'v2':
        out += (None, )  # GFocalHead's cls_feat slot
    return out


def aug_view_metas(case):
    """img_metas (outer list = views, inner = the one image) of an AUG_CASES
    row, with the keys bbox_mapping_back reads."""
    import numpy as np
    metas = []
    for pad, shape, sf, flip, direction in case[2]:
        metas.append([dict(img_shape=shape, pad_shape=tuple(pad) + (3, ),
                           scale_factor=np.array([sf] * 4, dtype=np.float32),
                           flip=flip, flip_direction=direction)])
    return metas


# ---------------------------------------------------------------- eval_map ----
# (name, seed, num_imgs, num_classes, scale_ranges, ignored GTs, empty cases,
#  hand-made boundary image).  Scores are a permutation of distinct fp32
#  values: tie-free inside every class, so the reference's unstable argsort
#  has one answer (tests/golden/eval_map.npz, tools/gen_golden_evalmap.py).
EVAL_CASES = [
    ('base', 11, 60, 20, None, False, False, False),
    ('scales', 12, 40, 6, [(0, 32), (32, 96), (96, 1e5)], False, False, False),
    ('ignore', 13, 40, 5, None, True, False, False),
    ('ignore_scales', 13, 40, 5, [(0, 48), (48, 1e5)], True, False, False),
    ('empty', 14, 30, 8, None, False, True, False),
    ('exact', 15, 12, 3, [(0, 32), (32, 64), (64, 1e5)], True, False, True),
]
# which (dataset, iou_thr) runs of eval_map each case is scored with
EVAL_RUNS = {
    'base': [(None, 0.5), ('voc07', 0.5), (None, 0.75), ('voc07', 0.75)],
    'scales': [(None, 0.5), ('voc07', 0.5)],
    'ignore': [(None, 0.5), (None, 0.75)],
    'ignore_scales': [(None, 0.5), ('voc07', 0.5)],
    'empty': [(None, 0.5), ('voc07', 0.5)],
    'exact': [(None, 0.5), ('voc07', 0.5)],
}


def _eval_boxes(rng, n, lo=4.0, hi=150.0):
    xy = rng.uniform(0, 400, size=(n, 2))
    wh = rng.uniform(lo, hi, size=(n, 2))
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def eval_map_inputs(case):
    """An EVAL_CASES row -> (det_results, annotations) in the reference's form:
    ``det_results[i][c]`` (k, 5) float32, ``annotations[i]`` with ``bboxes``
    (n, 4) float32 / ``labels`` int64 (+ ``bboxes_ignore`` / ``labels_ignore``
    when the case has ignored GTs)."""
    name, seed, num_imgs, C, _, ign, empty, special = case
    rng = np.random.RandomState(seed)
    gt_classes = C - 3 if empty else C  # 'empty': the last 3 classes lack GTs
    imgs = []
    for i in range(num_imgs):
        ngt = 0 if empty and i % 5 == 0 else rng.randint(0, 7)
        gts = _eval_boxes(rng, ngt)
        gl = rng.randint(0, gt_classes, size=ngt).astype(np.int64)
        nig = rng.randint(0, 3) if ign else 0
        igs = _eval_boxes(rng, nig)
        il = rng.randint(0, C, size=nig).astype(np.int64)
        rows, labs = [], []
        for box, lab in zip(np.concatenate([gts, igs]),
                            np.concatenate([gl, il])):
            w, h = box[2] - box[0], box[3] - box[1]
            for _ in range(rng.randint(0, 4)):
                jit = rng.normal(0, 0.12, size=4) * np.array([w, h, w, h])
                rows.append(box + jit.astype(np.float32))
                labs.append(lab if rng.uniform() < 0.85 else
                            rng.randint(0, C))
        nfp = rng.randint(0, 5)
        rows += list(_eval_boxes(rng, nfp))
        labs += list(rng.randint(0, C, size=nfp))
        if empty and i == 0:  # an image with neither GTs nor detections
            gts, gl, rows, labs = gts[:0], gl[:0], [], []
        dets = np.array(rows, dtype=np.float32).reshape(-1, 4)
        labs = np.array(labs, dtype=np.int64)
        if empty:  # the last class has no detections at all
            labs[labs == C - 1] = 0
        imgs.append([dets, labs, gts, gl, igs, il])
    if special:
        # fp32 IoU exactly 0.5 ([0,0,10,5] in [0,0,10,10]), and areas on the
        # range bounds: a GT of area 32**2 and a detection of area 64**2
        imgs.insert(0, [
            np.array([[0, 0, 10, 5], [100, 100, 132, 132],
                      [200, 200, 264, 264], [0, 0, 10, 5]], np.float32),
            np.array([0, 1, 2, 1], np.int64),
            np.array([[0, 0, 10, 10], [100, 100, 132, 132],
                      [0, 0, 10, 10]], np.float32),
            np.array([0, 1, 1], np.int64),
            np.zeros((0, 4), np.float32), np.zeros((0, ), np.int64)])
    total = sum(len(x[1]) for x in imgs)
    scores = ((rng.permutation(total) + 1) / (total + 1)).astype(np.float32)
    assert len(np.unique(scores)) == total
    det_results, annotations, k = [], [], 0
    for dets, labs, gts, gl, igs, il in imgs:
        n = len(labs)
        d5 = np.concatenate([dets, scores[k:k + n, None]], 1)
        k += n
        det_results.append([d5[labs == c] for c in range(C)])
        ann = {'bboxes': gts, 'labels': gl}
        if ign:
            ann['bboxes_ignore'], ann['labels_ignore'] = igs, il
        annotations.append(ann)
    return det_results, annotations


# per-image mAP ranking (tests/golden/analyze_results.npz,
# tools/gen_golden_analyze_results.py): the EVAL_CASES rows named here, image by
# image, and the rows of IMAGE_MAP_CASES: (name, seed, num_classes, GTs of each
# image, extra false positives of each image, ignored GTs).  'crowd' has images
# above what the per-image kernel keeps in LDS (256 detections / 128 GTs) and
# one image whose GTs cover all 12 classes (-1: one GT of every class).
IMAGE_MAP_EVAL_CASES = ('base', 'ignore', 'empty', 'exact')
IMAGE_MAP_CASES = [
    ('crowd', 31, 12, (3, 150, 5, -1, 0, 40, 2, 140, 6, 1, 24, 9),
     (2, 10, 300, 4, 3, 0, 1, 150, 0, 2, 5, 280), True),
]


def image_map_inputs(case):
    """A row of EVAL_CASES or IMAGE_MAP_CASES -> (det_results, annotations,
    num_classes) in the reference's form; scores are distinct fp32 values."""
    if len(case) == 8:
        det_results, annotations = eval_map_inputs(case)
        return det_results, annotations, case[3]
    name, seed, C, gts_per_img, fps_per_img, ign = case
    rng = np.random.RandomState(seed)
    imgs = []
    for ngt, nfp in zip(gts_per_img, fps_per_img):
        if ngt < 0:
            gl = np.arange(C, dtype=np.int64)
        else:
            gl = rng.randint(0, C, size=ngt).astype(np.int64)
        gts = _eval_boxes(rng, len(gl))
        nig = rng.randint(0, 4) if ign else 0
        igs = _eval_boxes(rng, nig)
        il = rng.randint(0, C, size=nig).astype(np.int64)
        rows, labs = [], []
        for box, lab in zip(np.concatenate([gts, igs]),
                            np.concatenate([gl, il])):
            w, h = box[2] - box[0], box[3] - box[1]
            for _ in range(rng.randint(0, 5)):
                jit = rng.normal(0, 0.1, size=4) * np.array([w, h, w, h])
                rows.append(box + jit.astype(np.float32))
                labs.append(lab if rng.uniform() < 0.85 else
                            rng.randint(0, C))
        rows += list(_eval_boxes(rng, nfp))
        labs += list(rng.randint(0, C, size=nfp))
        perm = rng.permutation(len(labs))
        dets = np.array(rows, dtype=np.float32).reshape(-1, 4)[perm]
        labs = np.array(labs, dtype=np.int64)[perm]
        imgs.append([dets, labs, gts, gl, igs, il])
    total = sum(len(x[1]) for x in imgs)
    scores = ((rng.permutation(total) + 1) / (total + 1)).astype(np.float32)
    assert len(np.unique(scores)) == total
    det_results, annotations, k = [], [], 0
    for dets, labs, gts, gl, igs, il in imgs:
        n = len(labs)
        d5 = np.concatenate([dets, scores[k:k + n, None]], 1)
        k += n
        det_results.append([d5[labs == c] for c in range(C)])
        ann = {'bboxes': gts, 'labels': gl}
        if ign:
            ann['bboxes_ignore'], ann['labels_ignore'] = igs, il
        annotations.append(ann)
    return det_results, annotations, C


def image_map_cases():
    """Every case of the per-image fixture, by name."""
    by_name = {c[0]: c for c in EVAL_CASES}
    return [by_name[n] for n in IMAGE_MAP_EVAL_CASES] + IMAGE_MAP_CASES


def eval_map_scale_inputs(num_imgs=4952, num_classes=20, dets_per_img=100,
                          seed=21):
    """VOC07-test sized input in packed form: per image (100, 5) detections
    with labels and a few GTs.  Scores are quantised to 1/512 so that equal
    scores are common inside a class (the stable tie rule decides)."""
    rng = np.random.RandomState(seed)
    ngt = rng.randint(1, 8, size=num_imgs)
    gts = _eval_boxes(rng, int(ngt.sum()))
    gl = rng.randint(0, num_classes, size=len(gts)).astype(np.int64)
    goff = np.concatenate([[0], np.cumsum(ngt)])
    N = num_imgs * dets_per_img
    src = goff[:-1].repeat(dets_per_img) + (
        rng.randint(0, 1 << 30, size=N) % ngt.repeat(dets_per_img))
    box = gts[src]
    wh = np.concatenate([box[:, 2:] - box[:, :2]] * 2, 1)
    dets = box + (rng.normal(0, 0.2, size=(N, 4)) * wh).astype(np.float32)
    lab = np.where(rng.uniform(size=N) < 0.7, gl[src],
                   rng.randint(0, num_classes, size=N)).astype(np.int64)
    score = (rng.randint(0, 512, size=N) / np.float32(512)).astype(np.float32)
    dets = np.concatenate([dets, score[:, None]], 1).astype(np.float32)
    return dict(dets=dets.reshape(num_imgs, dets_per_img, 5),
                labels=lab.reshape(num_imgs, dets_per_img), gts=gts,
                gt_labels=gl, gt_off=goff)


# --------------------------------------------------------------- coco eval ----
# (name, seed, num_imgs, category ids in file order, GTs / image, dets / GT,
#  false positives / image, score grid (0: distinct scores), evaluate kwargs).
#  Image and category ids are deliberately unsorted and non-contiguous; json
#  areas differ from the box areas (segment areas); ~6% crowds
#  (tests/golden/coco_eval.npz, tools/gen_golden_coco.py).
COCO_CASES = [
    ('base', 31, 40, [3, 7, 1, 12, 5], 6, 3, 4, 0, {}),
    ('ties', 32, 30, [2, 9, 4], 5, 4, 6, 16, {}),
    ('maxdet', 33, 12, [1, 2], 14, 4, 10, 0,
     dict(proposal_nums=(12, 3, 8))),
    ('thrs', 34, 25, [8, 6, 4, 0], 5, 3, 3, 0,
     dict(iou_thrs=[0.5, 0.75, 0.6])),
]


def coco_eval_inputs(case):
    """A COCO_CASES row -> (dataset, results, classes, kwargs): ``dataset`` a
    COCO annotation dict (json-ready), ``results[i][c]`` (k, 5) float32 per
    image (file order) and class (label c = the c-th category of the file)."""
    name, seed, num_imgs, cat_ids, gpi, dpg, fpi, grid, kw = case
    rng = np.random.RandomState(seed)
    K = len(cat_ids)
    img_ids = [int(x) for x in rng.choice(10 * num_imgs, num_imgs,
                                          replace=False)]
    cats = [dict(id=c, name=f'cls{c}', supercategory='x') for c in cat_ids]
    images = [dict(id=i, width=640, height=480, file_name=f'{i}.jpg')
              for i in img_ids]
    anns, results, next_id = [], [], 1
    for n, img in enumerate(img_ids):
        ng = rng.randint(0, gpi + 1)
        xy = rng.uniform(0, 400, size=(ng, 2))
        wh = np.exp(rng.uniform(np.log(6), np.log(200), size=(ng, 2)))
        labs = rng.randint(0, K, size=ng)
        crowd = rng.uniform(size=ng) < 0.06
        rows = [[] for _ in range(K)]
        for g in range(ng):
            box = [float(xy[g, 0]), float(xy[g, 1]), float(wh[g, 0]),
                   float(wh[g, 1])]
            anns.append(dict(id=next_id, image_id=img,
                             category_id=cat_ids[labs[g]], bbox=box,
                             area=float(box[2] * box[3] *
                                        rng.uniform(0.45, 1.0)),
                             iscrowd=int(crowd[g])))
            next_id += 1
            x1, y1, x2, y2 = box[0], box[1], box[0] + box[2], box[1] + box[3]
            for _ in range(rng.randint(0, dpg + 1)):
                j = rng.normal(0, 0.1, size=4) * [box[2], box[3], box[2],
                                                   box[3]]
                lab = labs[g] if rng.uniform() < 0.85 else rng.randint(0, K)
                rows[lab].append([x1 + j[0], y1 + j[1], x2 + j[2], y2 + j[3]])
        for _ in range(rng.randint(0, fpi + 1)):
            x, y = rng.uniform(0, 450, size=2)
            w, h = np.exp(rng.uniform(np.log(4), np.log(150), size=2))
            rows[rng.randint(0, K)].append([x, y, x + w, y + h])
        res = []
        for c in range(K):
            r = np.array(rows[c], np.float32).reshape(-1, 4)
            s = rng.uniform(0.05, 1.0, size=len(r))
            if grid:
                s = np.round(s * grid) / grid
            res.append(np.concatenate([r, s[:, None]], 1).astype(np.float32))
        results.append(res)
    if name == 'ties':
        # annotation id 0 (a custom dataset's first id), an image without
        # detections, a category without GTs
        anns[0]['id'] = 0
        results[1] = [np.zeros((0, 5), np.float32) for _ in range(K)]
        anns = [a for a in anns if a['category_id'] != cat_ids[-1]]
    dataset = dict(images=images, annotations=anns, categories=cats)
    return dataset, results, [c['name'] for c in cats], dict(kw)


# ----------------------------------------------------------- eval_recalls ----
# (name, seed, GTs of each image (None: no GT entry), proposals of each image,
#  score column).  Proposals are GT boxes jittered by a few amplitudes plus
#  random distractors (uniformly random boxes alone recall nothing), shuffled,
#  with pairwise distinct scores inside an image: the reference's argsort has
#  one answer (tests/golden/recall.npz, tools/gen_golden_recall.py).  'mixed'
#  has an image without a GT entry, an empty one, one without proposals and one
#  with fewer proposals than GTs; 'big' one image above what the kernel keeps
#  in LDS (1500 proposals, cut to 1000, and 130 GTs); 'ties' is hand-made.
RECALL_CASES = [
    ('mixed', 41, (3, None, 0, 7, 5, 1), (40, 12, 9, 0, 3, 25), True),
    ('noscore', 42, (4, 0, 6, 2, None, 7), (30, 5, 40, 0, 11, 4), False),
    ('equal', 43, (5, 5, 5, 5), (30, 30, 30, 30), True),
    ('big', 44, (130, 4, 2), (1500, 20, 1), True),
    ('nogt', 45, (None, 0, 0), (6, 0, 9), True),
    ('ties', 0, None, None, True),
]
_RECALL_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1,
                           endpoint=True)
# (tag, case, proposal_nums, iou_thrs, through eval_recalls whole, recalls
#  must lie strictly between 0 and 1 at several entries)
RECALL_RUNS = [
    ('mixed', 'mixed', (5, 20, 100), _RECALL_THRS, False, True),
    ('unsorted_nums', 'mixed', (12, 3, 8), _RECALL_THRS, False, True),
    ('ties', 'ties', (2, 4, 6, 20), (0.5, 0.75, 1.0), False, False),
    ('noscore', 'noscore', (5, 20, 100), _RECALL_THRS, False, True),
    ('equal', 'equal', (5, 10, 30), [0.5, 0.7, 0.9], True, True),
    ('equal_int_float', 'equal', 10, 0.75, True, False),
    ('equal_none', 'equal', [20], None, True, False),
    ('big', 'big', (100, 300, 1000), _RECALL_THRS, False, True),
    ('nogt', 'nogt', (5, 20), (0.5, 0.75), False, False),
]


def recall_is_interior(recalls):
    """The generator's assertion: at least three entries (all of them in a
    smaller table) lie strictly between 0 and 1."""
    r = np.asarray(recalls)
    return int(((r > 0) & (r < 1)).sum()) >= min(3, r.size)


def _recall_ties():
    a, b = [10, 10, 50, 50], [100, 100, 160, 140]
    gts = [
        # duplicated GTs, a GT every proposal misses (twice), a plain one
        np.array([a, b, a, [300, 300, 340, 340], [200, 200, 260, 260],
                  [600, 20, 640, 60]], np.float32),
        np.array([a, a, a], np.float32),  # more equal GTs than proposals
    ]
    props = [
        np.array([[12, 11, 52, 49], a, [104, 98, 158, 143], a, b,
                  [104, 98, 158, 143], [205, 204, 262, 258],
                  [205, 204, 262, 258], [400, 400, 420, 420],
                  [14, 14, 46, 50]], np.float32),
        np.array([[12, 12, 50, 50], a], np.float32),
    ]
    scores = [np.array([.9, .3, .8, .7, .2, .6, .5, .4, .95, .1], np.float32),
              np.array([.5, .4], np.float32)]
    return gts, [np.concatenate([p, s[:, None]], 1)
                 for p, s in zip(props, scores)]


def recall_inputs(case):
    """A RECALL_CASES row -> (gts, proposals): ``gts[i]`` (n, 4) float32 or
    None, ``proposals[i]`` (k, 5) float32, or (k, 4) for a case without the
    score column."""
    name, seed, gts_per_img, props_per_img, with_score = case
    if name == 'ties':
        return _recall_ties()
    rng = np.random.RandomState(seed)
    gts, proposals = [], []
    for ngt, k in zip(gts_per_img, props_per_img):
        g = _eval_boxes(rng, ngt or 0)
        rows = []
        if len(g):
            wh = np.concatenate([g[:, 2:] - g[:, :2]] * 2, 1)
            for amp in (0.03, 0.08, 0.2):
                src = rng.permutation(len(g))[:max(1, (2 * len(g)) // 3)]
                jit = rng.normal(0, amp, size=(len(src), 4)) * wh[src]
                rows.append(g[src] + jit.astype(np.float32))
        near = np.concatenate(rows) if rows else np.zeros((0, 4), np.float32)
        near = near[rng.permutation(len(near))[:(2 * k) // 3]]
        p = np.concatenate([near, _eval_boxes(rng, k - len(near))])
        p = p[rng.permutation(k)].astype(np.float32)
        if with_score:
            s = ((rng.permutation(k) + 1) / (k + 1)).astype(np.float32)
            assert len(np.unique(s)) == k
            p = np.concatenate([p, s[:, None]], 1)
        gts.append(None if ngt is None else g)
        proposals.append(p)
    return gts, proposals


def recall_cases():
    """Every run of the recall fixture -> (tag, gts, proposals, proposal_nums,
    iou_thrs, whole, interior)."""
    by_name = {c[0]: c for c in RECALL_CASES}
    inputs = {}
    out = []
    for tag, name, nums, thrs, whole, interior in RECALL_RUNS:
        if name not in inputs:
            inputs[name] = recall_inputs(by_name[name])
        out.append((tag, ) + inputs[name] + (nums, thrs, whole, interior))
    return out


def recall_scale_inputs(num_imgs=5000, props_per_img=1000, seed=46):
    """val2017-sized input in packed form: per image (1000, 5) proposals
    around and away from its 1..13 (about 7) GTs, distinct scores."""
    rng = np.random.RandomState(seed)
    ngt = rng.randint(1, 14, size=num_imgs)
    gts = _eval_boxes(rng, int(ngt.sum()))
    goff = np.concatenate([[0], np.cumsum(ngt)])
    N = num_imgs * props_per_img
    src = goff[:-1].repeat(props_per_img) + (
        rng.randint(0, 1 << 30, size=N) % ngt.repeat(props_per_img))
    box = gts[src]
    wh = np.concatenate([box[:, 2:] - box[:, :2]] * 2, 1)
    amp = rng.choice([0.03, 0.1, 0.3, 1.0], size=(N, 1))
    props = box + (rng.normal(0, 1, size=(N, 4)) * amp * wh).astype(np.float32)
    score = np.stack([rng.permutation(props_per_img)
                      for _ in range(num_imgs)]).reshape(-1)
    score = ((score + 1) / np.float32(props_per_img + 1)).astype(np.float32)
    props = np.concatenate([props, score[:, None]], 1).astype(np.float32)
    return dict(proposals=props.reshape(num_imgs, props_per_img, 5), gts=gts,
                gt_off=goff)


def box_loss_rows(n, seed=31, img_h=160, img_w=224):
    """``n`` (pred, target) box pairs for the row box losses: seeded targets
    and predictions jittered around them by up to +-0.4 of the target's size per
    coordinate (so the pairs overlap partly, by little or not at all, and the
    predicted width and height stay positive)."""
    gen = _gen(seed)
    target, _ = synthetic_boxes(n, img_h, img_w, gen, min_size=2.0,
                                max_size=120.0)
    size = (target[:, 2:] - target[:, :2]).repeat(1, 2)
    pred = target + (torch.rand(n, 4, generator=gen) - 0.5) * 0.8 * size
    return pred.contiguous(), target


# ---------------------------------------------------------------------------
# plain ATSSHead / RetinaHead (tests/golden/plain_heads.npz,
# tools/gen_golden_plain_heads.py)
# ---------------------------------------------------------------------------
# Geometry of every plain-head case: 2 images padded to 128 x 128, the five
# levels 16^2 .. 1^2 of strides 8 .. 128, 4 classes.
PLAIN_PAD = (128, 128)
PLAIN_CLASSES = 4
PLAIN_FEAT = 8
PLAIN_CODERS = dict(atss=((0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)),
                    retina=((0., 0., 0., 0.), (1., 1., 1., 1.)))
# Hand-written GT boxes (x1, y1, x2, y2, label) per image.  'multi': the 64 px
# box IS the ATSS anchor of level 0, cell (6, 6) (image 0) and the 32 px box the
# RetinaNet anchor of ratio 1, scale 4 (base 3) of that cell (image 1) -- the two
# positives whose predicted dw is set beyond the clamp (PLAIN_CLAMP); the larger
# boxes, one of them reaching past the image, put positives on levels 1 to 3.
PLAIN_CASES = OrderedDict(
    multi=[[(16., 16., 80., 80., 1), (-62., -66., 190., 194., 3)],
           [(32., 32., 64., 64., 0), (4., 8., 124., 120., 2),
            (70.5, 3.25, 127., 41.5, 1)]],
    empty_img=[[(16., 16., 80., 80., 1), (3., 60., 99., 126., 0)], []],
    no_pos=[[], []])
PLAIN_SEEDS = dict(multi=71, empty_img=72, no_pos=73)
# (head, image, level, y, x, base anchor, delta value): reg channel base * 4 + 2
PLAIN_CLAMP = dict(atss=(0, 0, 6, 6, 0, 30.0), retina=(1, 0, 6, 6, 3, 6.0))
PLAIN_INFER = dict(seed=81, nms_pre=100,
                   img_shapes=[(128, 128, 3), (120, 110, 3)],
                   scale_factors=[[1.0, 1.0, 1.0, 1.0],
                                  [1.25, 1.25, 1.25, 1.25]])


# The pyramid whose levels end in partly filled blocks AFTER a full one: pad
# (8, 2056) gives one-row levels of 257, 129, 65, 33 and 17 cells, so the last
# cell of level 0 is the first of a second 256-wide block and the last cells of
# levels 0 to 2 sit in the second (third, fifth) 64-wide block.  Image 0: a
# 62 px and a 250 px box around x = 2048, the far end of every level (positives
# in cell 256 of level 0 and cell 64 of level 2 for the ATSS, MaxIoU and FCOS
# assigners alike), and a 60 px box near x = 500; image 1 has no GT.
RAGGED_PAD = (8, 2056)
RAGGED_GT = [[(2018., -30., 2080., 32., 1), (1925., -125., 2175., 125., 3),
              (470., -28., 530., 30., 0)], []]
RAGGED_SEED = 74


def plain_batch(case, device='cpu'):
    """gt_bboxes / gt_labels / img_metas of a PLAIN_CASES entry, or of the
    RAGGED_PAD pyramid (``case`` 'ragged')."""
    ragged = case == 'ragged'
    gtb, gtl = [], []
    for rows in (RAGGED_GT if ragged else PLAIN_CASES[case]):
        a = torch.tensor([r[:4] for r in rows], dtype=torch.float32)
        gtb.append(a.reshape(-1, 4).to(device))
        gtl.append(torch.tensor([int(r[4]) for r in rows],
                                dtype=torch.long).to(device))
    h, w = RAGGED_PAD if ragged else PLAIN_PAD
    metas = [dict(img_shape=(h, w, 3), pad_shape=(h, w, 3),
                  ori_shape=(h, w, 3), scale_factor=1.0, flip=False)
             for _ in gtb]
    return dict(gt_bboxes=gtb, gt_labels=gtl, img_metas=metas)


def plain_head_inputs(kind, seed, num_imgs=2, device='cpu', clamp=True,
                      pad=PLAIN_PAD):
    """Head outputs of a plain head on the ``pad`` pyramid: ``kind`` 'atss'
    -> cls (N, 4, h, w), reg (N, 4, h, w) ~ 4 * randn (in units of the coder's
    stds 0.1 / 0.2), ctr; 'retina' -> cls (N, 36, h, w), reg (N, 36, h, w) ~
    0.5 * randn.  ``clamp``: the PLAIN_CLAMP positive's dw is set beyond
    |log(wh_ratio_clip)|."""
    gen = _gen(seed)
    B = 1 if kind == 'atss' else 9
    amp = 4.0 if kind == 'atss' else 0.5
    out = dict(cls=[], reg=[])
    for (h, w) in level_shapes(pad):
        out['cls'].append(
            _normal((num_imgs, B * PLAIN_CLASSES, h, w), gen) * 1.2 - 3.0)
        out['reg'].append(_normal((num_imgs, B * 4, h, w), gen) * amp)
    if clamp:
        n, l, y, x, b, v = PLAIN_CLAMP[kind]
        out['reg'][l][n, b * 4 + 2, y, x] = v
    if kind == 'atss':
        out['ctr'] = synthetic_centerness(num_imgs, level_shapes(pad),
                                          seed=seed)
    return {k: [t.to(device) for t in v] for k, v in out.items()}


def plain_infer_inputs(kind, device='cpu'):
    """get_bboxes inputs: class logits lifted so that a few hundred (anchor,
    class) pairs pass score_thr, metas with a second image smaller than the
    pad (the decode clips to img_shape) and a scale factor."""
    cfg = PLAIN_INFER
    hi = plain_head_inputs(kind, cfg['seed'], len(cfg['img_shapes']), device)
    hi['cls'] = [c * 1.25 + 1.0 for c in hi['cls']]
    metas = [dict(img_shape=s, pad_shape=PLAIN_PAD + (3, ), ori_shape=s,
                  scale_factor=np.array(f, dtype=np.float32), flip=False)
             for s, f in zip(cfg['img_shapes'], cfg['scale_factors'])]
    return hi, metas


# ---------------------------------------------------------------------------
# plain FCOSHead (tests/golden/fcos_head.npz, tools/gen_golden_fcos_head.py):
# the PLAIN_* geometry, cases and seeds with the default regress_ranges
# ---------------------------------------------------------------------------
FCOS_STRIDES = (8, 16, 32, 64, 128)
# the per-level Scale parameters the loss cases run with (the reference starts
# them at 1.0; distinct values make the per-level scale gradient tell levels
# apart)
FCOS_SCALES = (1.0, 0.75, 1.25, 0.5, 1.5)
# head variants: constructor arguments on top of the reference's defaults
FCOS_VARIANTS = OrderedDict(
    plain={},
    center=dict(center_sampling=True),
    tricks=dict(center_sampling=True, norm_on_bbox=True,
                centerness_on_reg=True,
                loss_bbox=dict(type='GIoULoss', loss_weight=1.0)),
    # not a config of the reference: relu distances under the default IoULoss,
    # where a zero-area box costs -log(eps)
    norm_iou=dict(norm_on_bbox=True))
# ReLU variants, case 'multi': two positives of the 64 px box of image 0 (with
# and without center_sampling), (image, level, y, x): ``all`` has four negative
# pre-activations -- a zero-area box with a zero gradient --, ``one`` exactly one
# (channel FCOS_NEG_CH)
FCOS_NEG = dict(all=(0, 0, 5, 5), one=(0, 0, 6, 6))
FCOS_NEG_CH = 2


def fcos_head_inputs(seed, num_imgs=2, device='cpu', relu=False,
                     pad=PLAIN_PAD):
    """Outputs of the plain FCOS head's convs on the ``pad`` pyramid: cls
    (N, 4, h, w) and ctr as for plain_head_inputs('atss'), ``raw`` (N, 4, h, w)
    ~ 0.5 * randn -- the box maps BEFORE Scale and exp / relu, so exp stays in
    range.  ``relu`` (the norm_on_bbox variants): every pre-activation is moved
    0.125 away from zero and the FCOS_NEG cells get their negative ones.  The
    reference adds stride-unit distances to PIXEL points (fcos_head.py:233-236):
    a distance of 1e-3 next to a coordinate of 80 keeps 7 bits in fp32, and
    seed 71 draws such a positive (0.0006 on level 2), whose IoU gradient the
    reference's own fp32 then gets 0.4 % wrong.  The kink itself is the business
    of FCOS_NEG and of the activation kernels' own test."""
    gen = _gen(seed)
    out = dict(cls=[], raw=[])
    for (h, w) in level_shapes(pad):
        out['cls'].append(
            _normal((num_imgs, PLAIN_CLASSES, h, w), gen) * 1.2 - 3.0)
        out['raw'].append(_normal((num_imgs, 4, h, w), gen) * 0.5)
    if relu:
        out['raw'] = [r + 0.125 * torch.sign(r) for r in out['raw']]
        n, l, y, x = FCOS_NEG['all']
        out['raw'][l][n, :, y, x] = -out['raw'][l][n, :, y, x].abs() - 0.125
        n, l, y, x = FCOS_NEG['one']
        out['raw'][l][n, :, y, x] = out['raw'][l][n, :, y, x].abs() + 0.125
        out['raw'][l][n, FCOS_NEG_CH, y, x] *= -1.0
    out['ctr'] = synthetic_centerness(num_imgs, level_shapes(pad),
                                      seed=seed)
    return {k: [t.to(device) for t in v] for k, v in out.items()}


def fcos_activate(raw, scales=FCOS_SCALES, norm_on_bbox=False, training=True):
    """fcos_head.py:145-153 on per-level raw maps with torch ops (any dtype,
    differentiable): what the head's forward returns for them."""
    out = []
    for r, s, stride in zip(raw, scales, FCOS_STRIDES):
        u = r * s
        if not norm_on_bbox:
            out.append(u.exp())
        else:
            u = torch.relu(u)
            out.append(u if training else u * stride)
    return out


def fcos_infer_inputs(device='cpu'):
    """get_bboxes inputs of the plain FCOS head: lifted class logits and the
    metas of plain_infer_inputs, ``reg`` = distances in pixels (exp of the raw
    maps times the stride, what an eval-mode forward returns)."""
    cfg = PLAIN_INFER
    hi = fcos_head_inputs(cfg['seed'], len(cfg['img_shapes']), device)
    hi['cls'] = [c * 1.25 + 1.0 for c in hi['cls']]
    hi['reg'] = [r.exp() * s for r, s in zip(hi.pop('raw'), FCOS_STRIDES)]
    metas = [dict(img_shape=s, pad_shape=PLAIN_PAD + (3, ), ori_shape=s,
                  scale_factor=np.array(f, dtype=np.float32), flip=False)
             for s, f in zip(cfg['img_shapes'], cfg['scale_factors'])]
    return hi, metas


def fcos_feats(seed=5, num_imgs=2, device='cpu'):
    """Neck outputs (N, PLAIN_FEAT, h, w) for the forward tests of the small
    head."""
    gen = _gen(seed)
    return [_normal((num_imgs, PLAIN_FEAT, h, w), gen).to(device)
            for (h, w) in level_shapes(PLAIN_PAD)]


DELTA_ROWS = 257  # two 128-thread blocks and one row
# hand-written coder rows: (anchor, gt box, deltas to decode)
DELTA_HAND = [
    # a degenerate anchor, 1 pixel wide / 1 pixel high
    ((10., 20., 11., 84.), (8., 18., 30., 90.), (0.5, -0.25, 1.0, 0.1)),
    ((40., 7., 104., 8.), (38., 2., 110., 20.), (-0.3, 2.0, -0.2, 3.0)),
    # dw / dh beyond the wh_ratio_clip clamp on both sides, for both std sets
    ((16., 16., 80., 80.), (0., 0., 128., 128.), (0.0, 0.0, 30.0, -30.0)),
    ((16., 16., 80., 80.), (20., 20., 60., 70.), (1.0, -1.0, -25.0, 22.0)),
    ((32., 32., 64., 64.), (30., 30., 70., 60.), (0.1, 0.2, 4.5, -4.5)),
    ((32., 32., 64., 64.), (33., 31., 63., 65.), (-0.1, 0.3, -4.2, 4.2)),
    # exactly at the clamp of the unit-std coder: |log(16 / 1000)|
    ((0., 0., 32., 32.), (1., 1., 31., 31.),
     (0.0, 0.0, 4.135166556742356, -4.135166556742356)),
    # decoded boxes that cross max_shape on every side
    ((-20., -30., 44., 34.), (-10., -10., 50., 40.), (-1.0, -1.0, 0.5, 0.5)),
    ((100., 90., 164., 154.), (90., 100., 170., 150.), (1.0, 1.0, 0.8, 0.9)),
    ((60., 60., 68., 68.), (0., 0., 128., 128.), (0.0, 0.0, 3.5, 3.5)),
]
DELTA_MAX_SHAPE = (120, 110, 3)


def delta_coder_rows(n=DELTA_ROWS, seed=91):
    """(anchors, gts, deltas), each (n, 4): DELTA_HAND first, then seeded rows
    -- anchors and GT boxes in and around a 128 px image, deltas ~ randn with
    every ninth row's dw / dh scaled past the clamp."""
    gen = _gen(seed)
    m = n - len(DELTA_HAND)
    anchors, _ = synthetic_boxes(m, 128, 128, gen, min_size=4.0, max_size=128.0)
    gts, _ = synthetic_boxes(m, 128, 128, gen, min_size=2.0, max_size=128.0)
    anchors = anchors + (torch.rand(m, 4, generator=gen) - 0.5) * 40.0
    anchors[:, 2:] = torch.maximum(anchors[:, 2:], anchors[:, :2] + 1.0)
    deltas = _normal((m, 4), gen)
    deltas[::9, 2:] = deltas[::9, 2:] * 25.0
    hand = [torch.tensor([r[i] for r in DELTA_HAND], dtype=torch.float32)
            for i in range(3)]
    return (torch.cat([hand[0], anchors]).contiguous(),
            torch.cat([hand[1], gts]).contiguous(),
            torch.cat([hand[2], deltas]).contiguous())
