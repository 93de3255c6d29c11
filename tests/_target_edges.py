"""Crafted inputs for the target-assignment kernels (ld_amd/csrc/targets.hip):
the ties, thresholds and GT-count edges that `synthetic.synthetic_batch`'s
continuous random boxes never produce.

Every box coordinate is a small integer or a dyadic fraction, so distances,
areas and the targeted IoUs are exact in fp32 and a tie is a tie in every
implementation.  Pyramids are tiny: pad (64, 96) gives the levels 8x12, 4x6,
2x3, 1x2, 1x1 (129 cells); RAGGED is an image whose valid region is one cell
wide on the coarse levels.

Each case is a named builder returning a dict:
  sizes, strides   pyramid geometry
  metas            per image: img_shape / pad_shape (the valid region)
  boxes, labels    per image: (G, 4) float32, (G,) int64
  claims           what edge the case contains, as counts; the host test
                   (tests/test_target_edges_host.py) recomputes every one of
                   them with oracle/ld_oracle.py alone and fails a case that
                   does not contain its edge
plus `topk` (ATSS), `assigner` (MaxIoU thresholds) or nothing (FCOS: both
centre-sampling modes are always run).  Plain numpy; no GPU code.  The only
builder that needs torch is `stress_cases`, whose seeded draws are torch's."""
import functools

import numpy as np

F32 = np.float32
PAD = (64, 96)
SIZES = [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]
STRIDES = [8, 16, 32, 64, 128]
RAGGED = (24, 56)   # valid cells per level: 3x7, 2x4, 1x2, 1x1, 1x1


def _meta(shape=PAD):
    return dict(img_shape=tuple(shape) + (3, ), pad_shape=tuple(shape) + (3, ))


def _b(rows):
    return np.asarray(rows, dtype=F32).reshape(-1, 4)


def _l(vals):
    return np.asarray(vals, dtype=np.int64).reshape(-1)


def _case(boxes, labels, metas=None, sizes=SIZES, strides=STRIDES, **kw):
    boxes = [_b(b) for b in boxes]
    labels = [_l(v) for v in labels]
    assert [b.shape[0] for b in boxes] == [v.shape[0] for v in labels]
    metas = metas or [_meta() for _ in boxes]
    return dict(sizes=list(sizes), strides=list(strides), metas=metas,
                boxes=boxes, labels=labels, **kw)


def crowd_boxes(n=130):
    """n distinct boxes whose centres are generic: cx = m + 1/64, cy = n + 1/8
    with integer m, n.  Two cells of a level, p cells apart in x and q in y,
    are equidistant from such a centre only if p / 64 + q / 8 is an integer,
    i.e. |p| >= 8: never among the nearest 16, so no tie at a k-th place."""
    out = []
    for i in range(n):
        cx = 15 + (i * 37) % 73 + 1 / 64.0    # 15 .. 87
        cy = 13 + (i * 53) % 38 + 1 / 8.0     # 13 .. 50
        w = 6 + (i * 7) % 41                  # full width, integer
        h = 5 + (i * 11) % 33
        out.append([cx - w / 2.0, cy - h / 2.0, cx + w / 2.0, cy + h / 2.0])
    return _b(out)


# ------------------------------------------------------------------- ATSS ---
def atss_dup_gt():
    """The same box two and three times under different labels, interleaved
    with other boxes: every positive of a duplicated box sees bit-equal IoUs
    from all its copies and must go to the first (64-bit atomicMax key)."""
    A = [5.125, 10, 37.125, 42]      # centres off the symmetric spots: no
    B = [43.125, 13, 89.125, 51]     # distance tie at the 9th, 12th or 16th
    C = [17.25, 21, 62.25, 48]       # place (checked by the host test)
    D = [61.125, 3, 90.125, 22]
    return _case(
        [[A, C, B, A, D, B, A], [B, B, C]],
        [[1, 11, 2, 5, 12, 3, 9], [21, 22, 23]],
        metas=[_meta(), _meta(RAGGED)], topk=9,
        claims=dict(dup_pairs=5, gt_iou_tie_anchors=12, kth_ties=0))


def atss_iou_tie():
    """Two different GTs mirrored about an anchor centre: x-mirrored about the
    level-0 anchor at (40, 32) in image 0, y-mirrored about (48, 32) in image
    1.  Each pair lies inside the anchors of the mirror column (row), so the
    two IoUs there are bit-equal and both pass their GT's threshold."""
    return _case(
        [[[10.125, 18, 58.125, 42], [21.875, 18, 69.875, 42]],
         [[28.125, 6, 68.125, 46], [28.125, 18, 68.125, 58]]],
        [[7, 3], [30, 40]], topk=9,
        claims=dict(gt_iou_tie_anchors=6, kth_ties=0))


def atss_dist_tie(topk=9):
    """GT centres on cell corners and edge midpoints of several levels: 2 or 4
    anchors tie at the k-th place of the top-k.  k = 9, and k = 1 and k = 4
    where the tie decides which anchors are candidates at all."""
    img0 = [[16, 8, 56, 48],      # centre (36, 28): level-0 corner
            [52, 16, 84, 48],     # centre (68, 32): level-0 edge midpoint
            [8, 8, 40, 40],       # centre (24, 24): level-1 corner
            [60, 32, 84, 56]]     # centre (72, 44): level-0 edge, level-1 edge
    img1 = [[4, 2, 36, 22],       # centre (20, 12) in the ragged image
            [16, 0, 48, 24]]      # centre (32, 12)
    return _case([img0, img1], [[1, 2, 3, 4], [5, 6]],
                 metas=[_meta(), _meta(RAGGED)], topk=topk,
                 claims=dict(kth_ties={9: 6, 4: 4, 1: 6}[topk]))


def atss_gt_is_anchor():
    """GT boxes that ARE anchors: the level-0 anchor at (32, 32) and the
    level-2 anchor at (64, 32): IoU exactly 1."""
    return _case([[[0, 0, 64, 64], [-64, -96, 192, 160]]], [[4, 8]], topk=9,
                 claims=dict(iou_one=2, kth_ties=0))


def atss_flat_iou():
    """One 2x2 level; the GT is centred between the four anchors, so every
    candidate has the same IoU: std = 0 and `ciou >= thr` compares a value
    with itself."""
    return _case([[[-2, -2, 10, 10]]], [[6]], metas=[_meta((16, 16))],
                 sizes=[(2, 2)], strides=[8], topk=9,
                 claims=dict(flat_gts=1, positives=4))


def atss_one_candidate():
    """Valid region 1x1 on a one-level geometry: ncand == 1, the unbiased std
    is NaN, so is the threshold, and nothing can be positive or VLR."""
    return _case([[[-2, -2, 6, 6]]], [[6]], metas=[_meta((8, 8))],
                 sizes=[(2, 2)], strides=[8], topk=9,
                 claims=dict(nan_thr=1, positives=0))


def atss_g130(topk=9):
    """130 GTs in image 0 (a second trip through the 128-GT chunk loop of the
    dense kernel), none in image 1, one in image 2 (max_gt padding)."""
    cb = crowd_boxes(130)
    return _case([cb, np.zeros((0, 4), F32), [[17.25, 21, 62.25, 48]]],
                 [np.arange(130) % 80, [], [33]], topk=topk,
                 claims=dict(max_gt=130, empty_images=1, kth_ties=0))


def atss_all_empty():
    """No image has a GT box (max_gt == 0): the select kernel is not launched."""
    z = np.zeros((0, 4), F32)
    return _case([z, z], [[], []], metas=[_meta(), _meta(RAGGED)], topk=9,
                 claims=dict(max_gt=0))


def atss_topk(topk=16):
    """top-k 12 and 16: the scan kernel's 16-slot instantiation."""
    c = atss_dup_gt()
    c.update(topk=topk, claims=dict(dup_pairs=5, gt_iou_tie_anchors=12,
                               kth_ties=0))
    return c


STRESS_GEOMETRIES = [((800, 1344), (800, 1333)), ((800, 1344), (611, 1000)),
                     ((128, 160), (128, 150)), ((64, 96), (40, 50)),
                     ((32, 32), (20, 9))]


@functools.lru_cache(maxsize=None)
def stress_cases():
    """The window-stress boxes of test_windowed_select_equals_full_scan: centres
    on and next to the image border, in the corners, boxes a few pixels wide,
    boxes that cover the whole image, half-cell centre offsets (distance
    ties), on two images (the second with the padded valid region).  One
    seeded torch generator is drawn from across the five geometries, as the
    test always did.  -> tuple of cases, one per STRESS_GEOMETRIES entry."""
    import torch
    from ld_amd import synthetic
    gen = torch.Generator().manual_seed(1234)
    out = []
    for pad, shape in STRESS_GEOMETRIES:
        sizes = synthetic.level_shapes(pad)
        H, W = shape
        boxes = []
        for i in range(60):
            kind = i % 6
            if kind == 0:    # anywhere, any size
                cx, cy = float(torch.rand(1, generator=gen)) * W, float(torch.rand(1, generator=gen)) * H
                w = float(torch.exp(torch.rand(1, generator=gen) * 6.0)) + 2.0
                h = float(torch.exp(torch.rand(1, generator=gen) * 6.0)) + 2.0
            elif kind == 1:  # hugging a border / corner
                cx = [1.5, W - 1.5, W / 2.0][i % 3]
                cy = [1.25, H - 1.25][(i // 3) % 2]
                w, h = 3.0, 2.5
            elif kind == 2:  # centre exactly on a cell boundary of the coarse levels
                cx, cy = 64.0 * (1 + i % 3), 64.0 * (1 + i % 2)
                w, h = 40.0 + i, 30.0 + i
            elif kind == 3:  # the whole image
                cx, cy, w, h = W / 2.0, H / 2.0, float(W), float(H)
            elif kind == 4:  # tiny
                cx = float(torch.rand(1, generator=gen)) * W
                cy = float(torch.rand(1, generator=gen)) * H
                w, h = 2.0, 2.0
            else:            # long and thin
                cx = float(torch.rand(1, generator=gen)) * W
                cy = float(torch.rand(1, generator=gen)) * H
                w, h = (float(W), 6.0) if i % 2 else (6.0, float(H))
            x1, y1 = max(cx - w / 2, 0.0), max(cy - h / 2, 0.0)
            x2, y2 = min(cx + w / 2, float(W)), min(cy + h / 2, float(H))
            if x2 - x1 >= 1.0 and y2 - y1 >= 1.0:
                boxes.append([x1, y1, x2, y2])
        # float32 exactly as torch.tensor(list of Python floats) rounds them
        gtb = [torch.tensor(boxes[:len(boxes) // 2]).numpy(),
               torch.tensor(boxes[len(boxes) // 2:]).numpy()]
        gtl = [np.arange(b.shape[0], dtype=np.int64) % 80 for b in gtb]
        metas = [dict(img_shape=(H, W, 3), pad_shape=(H, W, 3)),
                 dict(img_shape=(H, W, 3), pad_shape=pad + (3, ))]
        # whole-image boxes repeat; the half-cell centres tie at the 9th
        # place on every geometry but the smallest
        claims = dict(dup_pairs=40)
        if pad != (32, 32):
            claims['kth_ties'] = 18
        out.append(_case(gtb, gtl, metas=metas, sizes=sizes, topk=9,
                         pad=pad, shape=shape, claims=claims))
    return tuple(out)


def _stress(i):
    return stress_cases()[i]


ATSS_CASES = {
    'dup_gt': atss_dup_gt,
    'iou_tie': atss_iou_tie,
    'dist_tie_k9': functools.partial(atss_dist_tie, 9),
    'dist_tie_k4': functools.partial(atss_dist_tie, 4),
    'dist_tie_k1': functools.partial(atss_dist_tie, 1),
    'gt_is_anchor': atss_gt_is_anchor,
    'flat_iou': atss_flat_iou,
    'one_candidate': atss_one_candidate,
    'g130': atss_g130,
    'all_empty': atss_all_empty,
    'topk12': functools.partial(atss_topk, 12),
    'topk16': functools.partial(atss_topk, 16),
}
# cases where a distance tie at the k-th place decides the candidate set: the
# reference's torch.topk order among equals is unspecified, the oracle's
# documented rule (lower anchor index) is the definition
ATSS_TOPK_TIE_CASES = ('dist_tie_k9', 'dist_tie_k4', 'dist_tie_k1')
# the explicit-anchor API (ATSSAssigner over ld_atss_targets_ex), per image
ATSS_EXPLICIT_CASES = ('dist_tie_k9', 'dist_tie_k4', 'dist_tie_k1', 'iou_tie')
STRESS_CASES = {f'stress{i}': functools.partial(_stress, i)
                for i in range(len(STRESS_GEOMETRIES))}


# ----------------------------------------------------------------- MaxIoU ---
DEFAULT_ASSIGNER = dict(pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0.0)


def maxiou_pos_edge():
    """A GT that is exactly the right half of the square 64x64 base anchor of
    level 1 at (48, 32): IoU = 2048 / 4096 = 0.5, positive at pos_iou_thr =
    0.5.  A taller level-0 anchor fits the GT better, so the 0.5 anchor is
    positive through `mx >= pos_thr` alone, not as a low-quality match.  The
    GT centre (64, 32) is a cell centre of levels 0 to 3: no distance tie."""
    return _case([[[48, 0, 80, 64]]], [[5]], assigner=dict(DEFAULT_ASSIGNER),
                 claims=dict(iou_at_pos_thr=1))


def maxiou_neg_edge():
    """A 16x16 GT: a quarter of the square 32x32 base anchors of level 0 that
    contain it, IoU = 256 / 1024 = 0.25 = neg_iou_thr.  `mx < neg_thr` is
    false, the anchor is ignored (label_weight 0).  min_pos_iou = 0.5 keeps
    the low-quality match out of the way."""
    return _case([[[56, 24, 72, 40]]], [[5]],
                 assigner=dict(pos_iou_thr=0.5, neg_iou_thr=0.25,
                               min_pos_iou=0.5),
                 claims=dict(iou_at_neg_thr=1))


def maxiou_lowq_override():
    """Image 0: the two GTs are the top and the bottom seven eighths of the
    square level-0 anchor at (64, 32): that one anchor is the best of both
    (IoU 0.875 each) and the later GT must win it.  Image 1: the GT sits
    midway between two cells: two anchors attain its maximum and both must
    match."""
    return _case([[[48, 16, 80, 44], [48, 20, 80, 48]], [[64, 20, 88, 44]]],
                 [[1, 2], [3]], assigner=dict(DEFAULT_ASSIGNER),
                 claims=dict(shared_best_anchors=1, multi_argmax_gts=1))


def maxiou_dup_gt():
    A = [5, 10, 37, 42]
    B = [43, 13, 89, 51]
    C = [17, 21, 62, 48]
    return _case([[A, C, B, A, B, A], [B, B, C]],
                 [[1, 11, 2, 5, 3, 9], [21, 22, 23]],
                 metas=[_meta(), _meta(RAGGED)],
                 assigner=dict(DEFAULT_ASSIGNER), claims=dict(dup_pairs=5))


def maxiou_g130():
    return _case([crowd_boxes(130), [[17, 21, 62, 48]]],
                 [np.arange(130) % 80, [33]], assigner=dict(DEFAULT_ASSIGNER),
                 claims=dict(max_gt=130))


def maxiou_empty_beside_full():
    return _case([np.zeros((0, 4), F32), [[17, 21, 62, 48], [5, 10, 37, 42]]],
                 [[], [33, 34]], metas=[_meta(RAGGED), _meta()],
                 assigner=dict(DEFAULT_ASSIGNER),
                 claims=dict(empty_images=1))


MAXIOU_CASES = {
    'pos_edge': maxiou_pos_edge,
    'neg_edge': maxiou_neg_edge,
    'lowq_override': maxiou_lowq_override,
    'dup_gt': maxiou_dup_gt,
    'g130': maxiou_g130,
    'empty_beside_full': maxiou_empty_beside_full,
}


# ------------------------------------------------------------------- FCOS ---
# points: level l at (x * s + s // 2, y * s + s // 2)
def fcos_on_edge():
    """Integer boxes whose edges pass through level-0 points (x = 4, 36) and
    level-1 points (x = 8, 72): min(l, t, r, b) == 0 there, and `> 0` is
    strict."""
    return _case([[[4, 4, 36, 36]], [[8, 8, 72, 56]]], [[1], [2]],
                 claims=dict(on_edge=8))


def fcos_range_bound():
    """max(l, t, r, b) exactly on a regress-range bound; both ends are
    inclusive.  64: the level-0 points (4, 20) and (4, 28) of image 0 (upper
    end of level 0), the level-1 point (24, 24) of image 1 (lower end of level
    1).  128: the level-1 point (24, 24) of image 2 (upper end), the level-2
    point (48, 16) of image 3 (lower end).  Each of these points lies within
    the sampling radius of its box centre, so it counts with centre sampling
    on as well as off."""
    return _case([[[-60, 8, 64, 40]], [[-40, 8, 80, 40]],
                  [[-104, 8, 136, 40]], [[-80, 0, 160, 32]]],
                 [[1], [2], [3], [4]],
                 claims=dict(on_bound_64=2, on_bound_128=2))


def fcos_area_tie():
    """A 16x64 and a 32x32 box, area 1024 both, around the same centre."""
    return _case([[[32, 0, 48, 64], [24, 16, 56, 48]]], [[1, 2]],
                 claims=dict(area_tie_points=4))


def fcos_sample_clamp():
    """GTs narrower than 2 * stride * radius = 24 at level 0: the centre box
    is clamped to the GT edge (c0..c3), and level-0 points within the radius
    but outside the thin box must stay out."""
    return _case([[[34, 10, 46, 54]], [[38, 10, 46, 54], [10, 27, 30, 35]]],
                 [[1], [2, 3]], claims=dict(clamped_out=4))


def fcos_empty():
    z = np.zeros((0, 4), F32)
    return _case([z, [[24, 16, 56, 48]], z], [[], [7], []],
                 claims=dict(empty_images=2))


def fcos_all_empty():
    z = np.zeros((0, 4), F32)
    return _case([z, z], [[], []], claims=dict(max_gt=0))


def fcos_g130():
    return _case([crowd_boxes(130), [[24, 16, 56, 48]]],
                 [np.arange(130) % 80, [7]], claims=dict(max_gt=130))


FCOS_CASES = {
    'on_edge': fcos_on_edge,
    'range_bound': fcos_range_bound,
    'area_tie': fcos_area_tie,
    'sample_clamp': fcos_sample_clamp,
    'empty': fcos_empty,
    'all_empty': fcos_all_empty,
    'g130': fcos_g130,
}


# ------------------------------------------------- oracle runs and goldens ---
def oracle_atss(O, c):
    return O.get_targets(c['sizes'], c['metas'], c['boxes'], c['labels'],
                         strides=tuple(c['strides']), topk=c['topk'])


def oracle_maxiou(O, c):
    return O.retina_targets(c['sizes'], c['metas'], c['boxes'], c['labels'],
                            strides=tuple(c['strides']), **c['assigner'])


def oracle_fcos(O, c, center_sampling):
    return O.fcos_targets(c['sizes'], c['boxes'], c['labels'],
                          strides=tuple(c['strides']),
                          center_sampling=center_sampling)


def inside_anchors(O, c, n, per_level):
    """Image n's valid anchors and their per-level counts, as the reference
    hands them to its assigners; `per_level`: list of (A_l, 4) arrays."""
    B = per_level[0].shape[0] // (c['sizes'][0][0] * c['sizes'][0][1])
    flags = [np.repeat(f, B) for f in O.valid_flags(
        c['sizes'], c['metas'][n]['pad_shape'], tuple(c['strides']))]
    nl = [int(f.sum()) for f in flags]
    inside = np.concatenate(flags)
    return np.concatenate(per_level)[inside], nl, inside


def kth_ties(O, anchors, num_level, gts, topk):
    """Number of (GT, level) pairs whose k-th and (k+1)-th smallest centre
    distances are equal, k = min(topk, level size): there the tie rule decides
    which anchors are candidates."""
    gts = np.asarray(gts, F32).reshape(-1, 4)
    if gts.shape[0] == 0:
        return 0
    _, dist = O._candidates(anchors, num_level, gts, topk)
    n, s = 0, 0
    for m in num_level:
        k = min(topk, m)
        if 0 < k < m:
            d = np.sort(dist[s:s + m], axis=0)
            n += int((d[k - 1] == d[k]).sum())
        s += m
    return n


def maxiou_vlr_is_stored(O, c, n):
    """The reference's VLR region of MaxIoU image n is deterministic: there is
    a GT box and no distance tie at the 9th place of a level."""
    per_level = O.retina_grid_anchors(c['sizes'], tuple(c['strides']))
    anc, nl, _ = inside_anchors(O, c, n, per_level)
    return len(c['boxes'][n]) > 0 and \
        kth_ties(O, anc, nl, c['boxes'][n], 9) == 0


def oracle_atss_assign(O, c, n):
    """The assigner's own outputs (gt_inds, max_overlaps) on image n's valid
    anchors."""
    per_level = O.grid_anchors(c['sizes'], tuple(c['strides']))
    anc, nl, _ = inside_anchors(O, c, n, per_level)
    return O.atss_assign(anc, nl, c['boxes'][n], c['topk'])


def atss_from_golden(O, c, g, name):
    """Dense (N, A) labels / label_weights / bbox_targets / vlr rebuilt from
    the reference assigner's recorded gt_inds and VLR region (valid anchors
    only, as the reference runs it).  An image without GT boxes is the
    project's definition (the reference crashes there): all background."""
    per_level = O.grid_anchors(c['sizes'], tuple(c['strides']))
    A = sum(a.shape[0] for a in per_level)
    N = len(c['boxes'])
    out = dict(labels=np.full((N, A), 80, np.int64),
               label_weights=np.zeros((N, A), F32),
               bbox_targets=np.zeros((N, A, 4), F32),
               vlr=np.zeros((N, A), F32))
    for n in range(N):
        _, _, inside = inside_anchors(O, c, n, per_level)
        out['label_weights'][n][inside] = 1
        if len(c['boxes'][n]) == 0:
            continue
        gi = g[f'atss_{name}_gt_inds_{n}'].astype(np.int64)
        pos = gi > 0
        idx = np.nonzero(inside)[0]
        out['labels'][n][idx[pos]] = c['labels'][n][gi[pos] - 1]
        out['bbox_targets'][n][idx[pos]] = c['boxes'][n][gi[pos] - 1]
        out['vlr'][n][idx] = g[f'atss_{name}_vlr_{n}']
    return out
