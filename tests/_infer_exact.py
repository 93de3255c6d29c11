"""Head outputs on which the device post-processing (ld_amd/csrc/infer.hip) and
the numpy oracle (oracle/ld_oracle.py) do IDENTICAL fp32 arithmetic, so their
detections can be compared bit for bit -- and on which scores tie, which
continuous random logits never do.

 * class maps are probabilities (prob=True, the GFocalHead path: no sigmoid)
   from a small dyadic set; entries equal to 0 never pass a threshold
 * box maps are one-hot logits: 0 at the chosen bin, -200 elsewhere, so
   expf(-200) == 0, z == 1 and the Integral is the integer bin; every box
   coordinate is an integer multiple of the stride
 * centerness logits are 0 or 100: the factors are exactly 0.5 and 1.0
 * scale factors are powers of two

Two box layouts: `cell` (bins 0, 0, 1, 1: disjoint boxes, NMS keeps everything
and the output IS the sorted candidate list) and `group-of-16` (left bin
x % 16, right bin 16 - x % 16, top 0, bottom 1: 16 horizontally adjacent
anchors predict the identical box, IoU 1).

Tie patterns come from an integer hash of the anchor index, so a run of equal
scores spreads over the whole index range.  Plain numpy; no GPU code."""
import functools

import numpy as np

F32 = np.float32
OFF = -200.0  # logit of every bin but the chosen one
DYADIC = (0.0, 0.25, 0.5, 0.625, 0.75, 0.875, 1.0)
# value -> share of the anchors in sixteenths: a small top, two long tie runs
SHARES = ((0.75, 1), (0.5, 7), (0.25, 8))


def hash32(idx, seed):
    """Integer hash (as synthetic.grad_probe) of an index array -> uint32."""
    i = np.asarray(idx).astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    h = (i * np.uint64(2654435761) + np.uint64(seed * 40503 + 12345)) & m
    h = ((h ^ (h >> np.uint64(15))) * np.uint64(2246822519)) & m
    h = ((h ^ (h >> np.uint64(13))) * np.uint64(3266489917)) & m
    return (h ^ (h >> np.uint64(16))).astype(np.uint32)


def pick(idx, seed, shares=SHARES):
    """One value per index: `shares` = ((value, sixteenths), ...)."""
    u = (hash32(idx, seed) >> np.uint32(9)) % np.uint32(16)
    out = np.zeros(u.shape, F32)
    lo = 0
    for v, n in shares:
        out[(u >= lo) & (u < lo + n)] = v
        lo += n
    assert lo == 16
    return out


def rows_to_nchw(rows, H, W, B=1):
    """(N, H*W*B, K) rows, cell-major with the base anchor fastest ->
    (N, B*K, H, W) with channel b * K + k."""
    N, A, K = rows.shape
    assert A == H * W * B
    return np.ascontiguousarray(
        rows.reshape(N, H, W, B, K).transpose(0, 3, 4, 1, 2)
        .reshape(N, B * K, H, W))


def box_map(bins, H, W, B=1):
    """bins (N, A, 4) integers in 0..16 -> one-hot logits (N, B*68, H, W)."""
    bins = np.asarray(bins, np.int64)
    N, A, _ = bins.shape
    assert bins.min() >= 0 and bins.max() <= 16
    oh = np.full((N, A, 4, 17), OFF, F32)
    np.put_along_axis(oh, bins[..., None], F32(0), axis=-1)
    return rows_to_nchw(oh.reshape(N, A, 68), H, W, B)


def cell_bins(N, H, W, B=1):
    return np.tile(np.array([0, 0, 1, 1]), (N, H * W * B, 1))


def group16_bins(N, H, W):
    assert W % 16 == 0
    x = np.tile(np.arange(W), H)
    b = np.stack([x % 16, 0 * x, 16 - x % 16, 0 * x + 1], 1)
    return np.tile(b[None], (N, 1, 1))


def group16_ids(H, W):
    a = np.arange(H * W)
    return (a // W) * (W // 16) + (a % W) // 16


def one_class_rows(N, A, C, seed, shares=SHARES, groups=None):
    """(N, A, C) scores: one non-zero class per anchor, its value picked by the
    hash of the anchor, its label by the hash of the anchor (or of its group,
    so that duplicates share a class)."""
    rows = np.zeros((N, A, C), F32)
    a = np.arange(A)
    g = a if groups is None else groups
    for n in range(N):
        lab = hash32(g, seed + 101 * n + 1) % np.uint32(C)
        rows[n, a, lab] = pick(a, seed + 101 * n, shares)
    return rows


class Case:
    """Per-level NCHW numpy maps + the get_bboxes settings of one case."""

    def __init__(self, cls, reg, img_shapes, ctr=None, scale_factors=None,
                 nms_pre=1000, score_thr=0.05, iou_thr=0.6, max_per_img=1024,
                 points=False, num_base=1, voting=False):
        self.cls, self.reg, self.ctr = cls, reg, ctr
        self.img_shapes, self.scale_factors = img_shapes, scale_factors
        self.strides = (8, 16, 32, 64, 128)[:len(cls)]
        self.settings = dict(nms_pre=nms_pre, score_thr=score_thr,
                             iou_thr=iou_thr, max_per_img=max_per_img)
        self.variant = dict(points=points, num_base=num_base)
        self.voting = voting
        self._memo = {}

    def pre_nms(self):
        """Oracle: per image (boxes (K, 4), scores (K, C)[, factors (K,)]),
        unscaled."""
        import ld_oracle as O
        if 'pre' not in self._memo:
            self._memo['pre'] = O.get_bboxes_pre_nms(
                self.cls, self.reg, self.img_shapes, self.settings['nms_pre'],
                prob=True, centernesses=self.ctr, **self.variant)
        return self._memo['pre']

    def oracle(self, **over):
        """Oracle detections, per image (dets (k, 5), labels (k,)); computed
        once per distinct settings."""
        import ld_oracle as O
        s = dict(self.settings, **over)
        key = tuple(sorted(s.items()))
        if key not in self._memo:
            self._memo[key] = O.get_bboxes(
                self.cls, self.reg, self.img_shapes, self.scale_factors,
                rescale=self.scale_factors is not None, voting=self.voting,
                prob=True, centernesses=self.ctr, **self.variant, **s)
        return self._memo[key]

    def level_keys(self, l, n=0):
        """The top-k key of every anchor row of level l, image n: the max class
        score (times the centerness factor), rows cell * B + b."""
        B = self.variant['num_base']
        m = self.cls[l][n]
        C = m.shape[0] // B
        key = m.reshape(B, C, -1).max(1).T
        if self.ctr is not None:
            fac = np.where(self.ctr[l][n].reshape(-1) == 0, F32(0.5), F32(1))
            key = (key * fac[:, None]).astype(F32)
        return key.reshape(-1)

    def candidates(self, n=0):
        """Image n's candidate list in the order the NMS walks it: (scores,
        boxes, labels) sorted by score, ties in (slot, class) order."""
        pre = self.pre_nms()[n]
        bb, sc = pre[0], pre[1]
        C = sc.shape[1]
        valid = np.nonzero(sc.reshape(-1) > F32(self.settings['score_thr']))[0]
        s = sc.reshape(-1)[valid]
        if len(pre) > 2:
            s = (s * pre[2][valid // C]).astype(F32)
        order = np.argsort(-s, kind='stable')
        valid = valid[order]
        return s[order], bb[valid // C], valid % C


def _single(H, W, N, C, seed, layout='cell', shares=SHARES, img_hw=None, **kw):
    """One stride-8 level, one class per anchor."""
    groups = None
    if layout == 'cell':
        bins = cell_bins(N, H, W)
    else:
        bins, groups = group16_bins(N, H, W), group16_ids(H, W)
    rows = one_class_rows(N, H * W, C, seed, shares, groups)
    shape = img_hw or (H * 8, W * 8)
    return Case([rows_to_nchw(rows, H, W)], [box_map(bins, H, W)],
                [shape + (3, )] * N, **kw)


THREE_PATH_LEVELS = ((72, 64), (36, 32), (18, 16), (9, 8), (5, 4))


@functools.lru_cache(maxsize=None)
def three_paths():
    """Pad (576, 512), nms_pre 1000: level 0 (4608 anchors) takes the radix
    select, level 1 (1152) the LDS sort, the rest are unsorted; two images
    with different tie patterns."""
    N, C = 2, 3
    cls, reg = [], []
    for l, (H, W) in enumerate(THREE_PATH_LEVELS):
        cls.append(rows_to_nchw(one_class_rows(N, H * W, C, 7 + 13 * l), H, W))
        reg.append(box_map(cell_bins(N, H, W), H, W))
    return Case(cls, reg, [(576, 512, 3)] * N, nms_pre=1000)


# name -> (H, W, nms_pre[, shares]): A == nms_pre, nms_pre + 1, 4096 and 4097
# anchors; and a tie run so long that the keys at or above the k-th score do
# not fit the 4096-wide LDS sort, so the radix passes over the index bytes
# alone decide which of them are selected
LONG_RUN = ((0.75, 1), (0.5, 15))
BOUNDARY_LEVELS = {'A_eq_k': (36, 32, 1152), 'A_eq_k_plus_1': (36, 32, 1151),
                   'A_4096': (64, 64, 1000), 'A_4097': (17, 241, 1000),
                   'A_4608_long_run': (72, 64, 1000, LONG_RUN)}


@functools.lru_cache(maxsize=None)
def boundary(name):
    H, W, k = BOUNDARY_LEVELS[name][:3]
    # max_per_img 1024 < nms_pre for the first two: the pre-NMS rows show the
    # whole selection there
    return _single(H, W, 1, 3, 31 + H, nms_pre=k,
                   shares=(BOUNDARY_LEVELS[name] + (SHARES, ))[3])


@functools.lru_cache(maxsize=None)
def topk_4500():
    """nms_pre 4500 > 4096 on the 4608-anchor level: the global-memory bitonic
    sort of the level's keys, no environment switch needed."""
    return _single(72, 64, 1, 3, 5, nms_pre=4500)


@functools.lru_cache(maxsize=None)
def topk_reference_level():
    """The single 72x64 level with nms_pre 1000 (the closed-form premise)."""
    return _single(72, 64, 1, 3, 7, nms_pre=1000)


@functools.lru_cache(maxsize=None)
def window():
    """More candidates than the best-4096 window, most of them suppressed
    duplicates, fewer keeps than max_per_img: 72x64, group-of-16, two classes
    per anchor (the same two inside a group).  A (group, class) pair has a base
    score; every second anchor (by hash) carries it, the others the lowest
    value, so the window's edge falls inside the long run of lowest scores."""
    H, W, C, A = 72, 64, 4, 72 * 64
    g = group16_ids(H, W)
    a = np.arange(A)
    rows = np.zeros((1, A, C), F32)
    c1 = hash32(g, 3) % np.uint32(C)
    c2 = (c1 + np.uint32(1) + hash32(g, 4) % np.uint32(C - 1)) % np.uint32(C)
    for j, lab in enumerate((c1, c2)):
        base = pick(g * 2 + j, 11)
        carries = (hash32(a * 2 + j, 12) >> np.uint32(7)) & np.uint32(1)
        rows[0, a, lab] = np.where(carries == 1, base, F32(0.25))
    return Case([rows_to_nchw(rows, H, W)],
                [box_map(group16_bins(1, H, W), H, W)], [(576, 512, 3)],
                nms_pre=A, max_per_img=1024)


@functools.lru_cache(maxsize=None)
def keep_limits():
    """Cell layout, 1152 candidates in long tie runs: max_per_img and the
    256-wide NMS chunk."""
    return _single(36, 32, 1, 3, 17, nms_pre=2000)


def _tiny(entries, C=3, img_hw=(32, 32), **kw):
    """4x4 stride-8 level; entries = ((x, y, bins, label, score), ...)."""
    H = W = 4
    rows = np.zeros((1, H * W, C), F32)
    bins = cell_bins(1, H, W)
    for x, y, b, lab, s in entries:
        rows[0, y * W + x, lab] = s
        bins[0, y * W + x] = b
    return Case([rows_to_nchw(rows, H, W)], [box_map(bins, H, W)],
                [img_hw + (3, )], **kw)


IOU_THR_BELOW_HALF = float(np.nextafter(F32(0.5), F32(0)))


@functools.lru_cache(maxsize=None)
def iou_half():
    """[0, 0, 16, 16] and [0, 0, 16, 8], class 1: IoU exactly 0.5."""
    return _tiny(((0, 0, (0, 0, 2, 2), 1, 0.75), (1, 0, (1, 0, 1, 1), 1, 0.5)),
                 iou_thr=0.5)


SCORE_ABOVE_THR = float(np.nextafter(F32(0.25), F32(1)))


@functools.lru_cache(maxsize=None)
def score_thr_edge():
    """score_thr 0.25: scores equal to it are out, 0.25 + 1 ulp is in."""
    cells = [(x, y) for y in range(4) for x in range(4)]
    vals = [0.25, SCORE_ABOVE_THR, 0.5, 0.25, SCORE_ABOVE_THR, 0.25, 0.75,
            SCORE_ABOVE_THR]
    return _tiny([(x, y, (0, 0, 1, 1), (x + y) % 3, v)
                  for (x, y), v in zip(cells, vals)], score_thr=0.25)


@functools.lru_cache(maxsize=None)
def zero_area():
    """Image 32 x 16 under a 32 x 32 pad: the boxes of the columns x >= 2 are
    clamped to the zero-area line x = 16.  They are kept, and the 0 / 0 = NaN
    overlap of two of them (same class) suppresses nothing."""
    return _tiny(((3, 0, (0, 0, 1, 1), 2, 0.75), (3, 1, (0, 0, 1, 1), 2, 0.5),
                  (2, 0, (0, 0, 1, 1), 2, 0.5), (3, 0, (0, 0, 1, 1), 0, 0.5),
                  (0, 2, (0, 0, 1, 1), 2, 0.625)), img_hw=(32, 16))


def many_images_count(n):
    return 7 * (n % 9)


@functools.lru_cache(maxsize=None)
def many_images():
    """65 images of one 8x8 level, 7 * (n % 9) candidates in image n."""
    N, H, W, C = 65, 8, 8, 3
    rows = one_class_rows(N, H * W, C, 23, ((0.75, 2), (0.5, 7), (0.25, 7)))
    for n in range(N):
        rank = np.argsort(hash32(np.arange(H * W), 500 + n), kind='stable')
        rows[n, rank[many_images_count(n):]] = 0
    return Case([rows_to_nchw(rows, H, W)],
                [box_map(cell_bins(N, H, W), H, W)], [(64, 64, 3)] * N,
                nms_pre=1000, max_per_img=100)


CTR_SCORE_THR = 0.3


@functools.lru_cache(maxsize=None)
def ctr_product_ties():
    """Centerness factors 0.5 / 1.0 on scores 0.5 / 0.75 / 1.0: the top-k key
    and the NMS order tie across different (score, factor) pairs
    (0.5 * 1.0 == 1.0 * 0.5), and 0.5 * 0.5 = 0.25 < score_thr = 0.3 stays a
    candidate because the threshold tests the score, not the product."""
    N, H, W, C = 2, 16, 16, 3
    rows = one_class_rows(N, H * W, C, 41, ((1.0, 4), (0.75, 4), (0.5, 8)))
    half = np.stack([(hash32(np.arange(H * W), 43 + n) >> np.uint32(11)) &
                     np.uint32(1) for n in range(N)])
    ctr = np.where(half == 1, F32(0), F32(100)).astype(F32)
    return Case([rows_to_nchw(rows, H, W)],
                [box_map(cell_bins(N, H, W), H, W)], [(128, 128, 3)] * N,
                ctr=[ctr.reshape(N, 1, H, W)], nms_pre=230,
                score_thr=CTR_SCORE_THR)


@functools.lru_cache(maxsize=None)
def fcos_points():
    """points=True: centres (x, y) * 8 + 4; with top-k."""
    return _single(16, 16, 2, 3, 47, nms_pre=100, points=True)


@functools.lru_cache(maxsize=None)
def nine_anchors():
    """num_base = 9: rows cell * 9 + b, channels b * C + c / b * 68 + ...; the
    nine anchors of a cell share one score (ties between base anchors) and one
    box, their labels differ.  The device takes the cell origin as the centre
    of all nine; the reference averages its fp32 anchor corners, which lands
    one ulp off the origin for a few (cell, base anchor) pairs.  Those pairs
    score 0 here (never a candidate), so both sides decode integers."""
    import ld_oracle as O
    N, H, W, C, B = 1, 8, 8, 3, 9
    A = H * W * B
    a = np.arange(A)
    rows = np.zeros((N, A, C), F32)
    rows[0, a, hash32(a, 53) % np.uint32(C)] = pick(a // B, 54)
    anc = O.retina_grid_anchors([(H, W)], (8, ))[0]
    centre = (anc[:, :2] + anc[:, 2:]) / F32(2)
    rows[0, ~(centre == np.round(centre)).all(1)] = 0
    return Case([rows_to_nchw(rows, H, W, B)],
                [box_map(cell_bins(N, H, W, B), H, W, B)], [(64, 64, 3)],
                nms_pre=300, num_base=B)


@functools.lru_cache(maxsize=None)
def scaled():
    """rescale=True with scale factors 0.5 and 2."""
    return _single(16, 16, 2, 3, 59, nms_pre=100,
                   scale_factors=[[0.5] * 4, [2.0] * 4])


@functools.lru_cache(maxsize=None)
def voting():
    """One 36x32 level, group-of-16, both of two classes on every anchor
    (2304 candidates: the oracle's dense matrix stays near 20 MB)."""
    H, W, C = 36, 32, 2
    a = np.arange(H * W)
    rows = np.stack([pick(a, 61), pick(a, 62)], 1)[None].astype(F32)
    return Case([rows_to_nchw(rows, H, W)],
                [box_map(group16_bins(1, H, W), H, W)], [(288, 256, 3)],
                nms_pre=2000, max_per_img=100, voting=True)


AUG_SETTINGS = dict(score_thr=0.05, iou_thr=0.6, max_per_img=1024)


@functools.lru_cache(maxsize=None)
def aug_views():
    """Two views of one 256 x 256 image holding the same tied rows: view 0 at
    scale 2, view 1 at scale 4 and flipped horizontally.  -> (views as numpy
    dicts for lossblock.aug_merge_nms, merged boxes (2K, 4), merged scores
    (2K, C)): mapped back, both views give the same integer boxes.  A row of
    view 1 either duplicates view 0's (IoU 1, equal score: the lower merged
    index, view 0's, wins) or, for the rows `aug_moved()` marks, carries the
    score on the next class and survives -- behind every view-0 row of its
    score, because ties are ordered view-major."""
    H = W = 16
    C, K = 3, H * W
    a = np.arange(K)
    x, y = (a % W).astype(F32) * 16, (a // W).astype(F32) * 16
    base = np.stack([x, y, x + 16, y + 16], 1).astype(F32)
    scores = one_class_rows(1, K, C, 67)[0]
    views = []
    for sf, flip in ((2.0, False), (4.0, True)):
        b = (base * F32(sf)).astype(F32)
        w = F32(256 * sf)
        if flip:
            b = np.stack([w - b[:, 2], b[:, 1], w - b[:, 0], b[:, 3]], 1)
        sc = scores.copy()
        if flip:
            sc[aug_moved(K)] = np.roll(scores[aug_moved(K)], 1, axis=1)
        views.append(dict(
            boxes=b.astype(F32), scores=sc,
            img_shape=(int(256 * sf), int(256 * sf), 3),
            scale_factor=np.array([sf] * 4, F32), flip=flip,
            flip_direction='horizontal' if flip else None))
    return views, np.concatenate([map_back(v) for v in views]), \
        np.concatenate([v['scores'] for v in views])


def aug_moved(K):
    return ((hash32(np.arange(K), 71) >> np.uint32(5)) & np.uint32(3)) == 0


def map_back(view):
    """bbox_mapping_back in fp32: un-flip in the view's frame, then a true
    division by the view's scale factor."""
    b = view['boxes'].astype(F32)
    if view['flip']:
        w = F32(view['img_shape'][1])
        b = np.stack([w - b[:, 2], b[:, 1], w - b[:, 0], b[:, 3]], 1)
    return (b / view['scale_factor'][None]).astype(F32)
