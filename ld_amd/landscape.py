"""The AP landscape and the teacher-student discrepancy numbers of the LD
paper's journal version ("logit mimicking vs. feature imitation"), the
reference's top-level ``AP_landscape/`` tool, run by landscape.hip
(``ld_levels_mix``, ``ld_levels_abs_err``, ``ld_levels_pearson``).

The reference (AP_landscape/detectors/single_stage.py:113-121,
AP_landscape/apis/test.py:100-103) runs two detectors on every image and feeds
the second one's head ``0.9 * x_own + 0.7 * x_other`` on each FPN level; the
two constants are edited in the source and the whole test re-run for the next
point of the landscape.  ``FeatureLandscape`` takes the list of points: both
backbones and necks run once per image, every chunk of grid points is mixed
by ONE launch into the level-concatenated (N, C, P) tensor the head towers
consume, stacked on the batch axis, and the head, ``get_bboxes`` and the
evaluators see a batch of ``chunk * N``.

``TeacherStudentDiscrepancy`` is the block of apis/test.py:105-177 that the
reference's author switches on by hand: the average error of the FPN features,
of the cls and of the bbox outputs -- per level ``abs(t - s).mean(1).sum()``,
summed over the levels and divided by the number of positions -- and the mean
Pearson correlation of the channel maps of a level (the reference looks at
``x[2]``, P5).  The |t - s| are fp32 as in the reference; every sum is
float64.  A channel map that is constant in either model has no correlation
(torch gives NaN): it is left out of the mean and counted.
"""
import ctypes as C

import numpy as np
import torch

from . import layers as Y
from . import lib as L
from .lossblock import workspace

__all__ = ['mix_levels', 'repeat_metas', 'TeacherStudentDiscrepancy',
           'FeatureLandscape']


# ---------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------
def _levels_of(feats):
    return tuple((int(f.shape[2]), int(f.shape[3])) for f in feats)


def _check_levels(feats, what):
    if len(feats) == 0 or len(feats) > L.LD_MAX_LEVELS:
        raise ValueError(f'{what}: 1..{L.LD_MAX_LEVELS} levels, got '
                         f'{len(feats)}')
    f0 = feats[0]
    for f in feats:
        if f.dim() != 4 or f.shape[:2] != f0.shape[:2]:
            raise ValueError(f'{what}: every level must be (N, C, H, W) with '
                             f'one N and C, got {[tuple(g.shape) for g in feats]}')
        if f.dtype != torch.float32:
            raise ValueError(f'{what}: fp32 maps, got {f.dtype}')


def _check_pair(a, la, b, lb, what):
    """Two packed shapes (N, C, P) with their levels must agree."""
    if tuple(la) != tuple(lb):
        raise ValueError(f'{what}: level shapes differ between the two '
                         f'models: {tuple(la)} and {tuple(lb)}')
    if tuple(a) != tuple(b):
        raise ValueError(f'{what}: shapes differ between the two models: '
                         f'{tuple(a)} and {tuple(b)} (N, C, P)')


def _packed_shape(x, levels, what):
    """(shape (N, C, P), levels) of a level tuple or of a packed tensor,
    checked; nothing touches the data."""
    if isinstance(x, torch.Tensor):
        if levels is None:
            raise ValueError(f'{what}: a packed (N, C, P) tensor needs its '
                             'levels=((H, W), ...)')
        levels = tuple((int(h), int(w)) for h, w in levels)
        if x.dim() != 3 or x.dtype != torch.float32:
            raise ValueError(f'{what}: a packed tensor is (N, C, P) fp32, got '
                             f'{tuple(x.shape)} {x.dtype}')
        if not 1 <= len(levels) <= L.LD_MAX_LEVELS or \
                any(h <= 0 or w <= 0 for h, w in levels) or \
                sum(h * w for h, w in levels) != x.shape[2]:
            raise ValueError(f'{what}: levels {levels} do not sum to P = '
                             f'{x.shape[2]}')
        return tuple(x.shape), levels
    x = tuple(x)
    _check_levels(x, what)
    lv = _levels_of(x)
    if levels is not None and tuple(map(tuple, levels)) != lv:
        raise ValueError(f'{what}: levels {tuple(levels)} given for maps of '
                         f'{lv}')
    return (int(x[0].shape[0]), int(x[0].shape[1]),
            sum(h * w for h, w in lv)), lv


def _pack(x, levels):
    """-> the contiguous (N, C, P) device tensor of a level tuple (the views of
    one packed buffer are taken as that buffer, anything else is packed by one
    launch) or of a packed tensor."""
    if isinstance(x, torch.Tensor):
        x3 = x.detach()
    else:
        x = [f.detach() for f in x]
        N, c = int(x[0].shape[0]), int(x[0].shape[1])
        x3 = Y._common_buffer(x, levels, N, c)
        if x3 is None:
            for f in x:
                L.require_device(f, torch.float32, 'level map')
            with torch.no_grad():
                x3, _ = Y.pack_levels(tuple(x))
    L.require_device(x3, torch.float32, 'packed levels')
    return x3 if x3.is_contiguous() else x3.contiguous()


def repeat_metas(img_metas, k):
    """The image metas of a batch stacked ``k`` times, grid point major -- the
    order of the batch axis of ``mix_levels``' output."""
    return [m for _ in range(k) for m in img_metas]


def _coefs(coefs):
    try:
        out = [(float(a), float(b)) for a, b in coefs]
    except (TypeError, ValueError):
        raise ValueError('coefs: a list of (a, b) pairs') from None
    if not out:
        raise ValueError('coefs: at least one (a, b) pair')
    return out


# ---------------------------------------------------------------------------
# the mix
# ---------------------------------------------------------------------------
def mix_levels(own, other, coefs, levels=None):
    """``out[k * N + n] = a_k * own[n] + b_k * other[n]`` for the K pairs of
    ``coefs``.  ``own`` / ``other``: the per-level (N, C, H_l, W_l) maps of two
    models, or packed (N, C, P) tensors with ``levels``.  -> the packed
    ``(K * N, C, P)`` tensor (grid point major) and ``levels``: what
    ``forward_packed`` of a dense head takes.  fp32 multiply, multiply, add:
    the bits of torch's ``a * x + b * y``.  One launch per
    ``LD_LEVELS_MIX_MAX_K`` grid points."""
    coefs = _coefs(coefs)
    sa, la = _packed_shape(own, levels, 'mix_levels: own')
    sb, lb = _packed_shape(other, levels, 'mix_levels: other')
    _check_pair(sa, la, sb, lb, 'mix_levels')
    a3, b3 = _pack(own, la), _pack(other, la)
    if a3.device != b3.device:
        raise ValueError('mix_levels: own and other are on different devices')
    N, c, P = sa
    K, n = len(coefs), N * c * P
    out = torch.empty((K * N, c, P), dtype=torch.float32, device=a3.device)
    lib, cap = L.get_lib(), L.LD_LEVELS_MIX_MAX_K
    for k0 in range(0, K, cap):
        part = coefs[k0:k0 + cap]
        flat = (C.c_float * (2 * len(part)))(*[v for ab in part for v in ab])
        L.check(lib.ld_levels_mix(
            L.ptr(a3), L.ptr(b3), n, len(part), C.cast(flat, C.c_void_p),
            L.ptr(out[k0 * N:]), L.stream_ptr(a3.device)), 'ld_levels_mix')
    return out, la


# ---------------------------------------------------------------------------
# the discrepancy numbers
# ---------------------------------------------------------------------------
def levels_abs_err(t3, s3, levels):
    """(N, C, P) pair -> (N, L) float64 device tensor: per image and level the
    sum over the level's positions of the channel mean of |t - s|."""
    N, c, P = t3.shape
    lv = Y.levels_desc(levels)
    lib = L.get_lib()
    need = lib.ld_levels_abs_err_workspace_bytes(C.byref(lv), N, c, P)
    if need == 0:
        raise L.LdError('ld_levels_abs_err_workspace_bytes: bad sizes')
    ws = workspace(t3.device, need, 'levels_abs_err')
    out = torch.empty((N, len(levels)), dtype=torch.float64, device=t3.device)
    L.check(lib.ld_levels_abs_err(
        C.byref(lv), L.ptr(t3), L.ptr(s3), N, c, P, L.ptr(out), L.ptr(ws),
        ws.numel(), L.stream_ptr(t3.device)), 'ld_levels_abs_err')
    return out


def levels_pearson(t3, s3, levels):
    """(N, C, P) pair -> (r_sum (N, L) float64, counts (N, L, 2) int32 [valid,
    degenerate]) device tensors: Pearson r of every (n, c) row of every level
    segment, summed over the valid rows."""
    N, c, P = t3.shape
    lv = Y.levels_desc(levels)
    lib = L.get_lib()
    need = lib.ld_levels_pearson_workspace_bytes(C.byref(lv), N, c, P)
    if need == 0:
        raise L.LdError('ld_levels_pearson_workspace_bytes: bad sizes')
    ws = workspace(t3.device, need, 'levels_pearson')
    r_sum = torch.empty((N, len(levels)), dtype=torch.float64,
                        device=t3.device)
    counts = torch.empty((N, len(levels), 2), dtype=torch.int32,
                         device=t3.device)
    L.check(lib.ld_levels_pearson(
        C.byref(lv), L.ptr(t3), L.ptr(s3), N, c, P, L.ptr(r_sum),
        L.ptr(counts), L.ptr(ws), ws.numel(), L.stream_ptr(t3.device)),
        'ld_levels_pearson')
    return r_sum, counts


def _teacher_of(student, teacher):
    if teacher is None:
        teacher = getattr(student, 'teacher_model', None)
        if teacher is None:
            raise ValueError(
                'no teacher given and the student has no teacher_model (it is '
                'not a KnowledgeDistillationSingleStageDetector)')
    return teacher


_FAMILIES = ('feature', 'cls', 'bbox')


class TeacherStudentDiscrepancy:
    """Streaming teacher-student discrepancy: ``add`` batches of images, then
    ``compute``.  ``teacher=None`` takes ``student.teacher_model``.  Both
    models are used as they are (put them in ``eval()`` mode, as the
    reference's test loop does)."""

    def __init__(self, student, teacher=None):
        self.student, self.teacher = student, _teacher_of(student, teacher)
        self.levels = None
        self._err = {f: [] for f in _FAMILIES}   # per add (N, L) float64
        self._pos = []                           # per add: positions per level
        self._r, self._cnt = [], []

    def add(self, img, img_metas=None):
        """One batch (N, 3, H, W): both ``extract_feat`` calls and both heads
        under ``no_grad``, then one abs-err launch pair per family (features,
        ``outs[0]``, ``outs[1]``) and one Pearson launch pair on the features.
        ``img_metas`` is not needed (padded area is part of the numbers, as in
        the reference)."""
        with torch.no_grad():
            xs = self.student.extract_feat(img)
            xt = self.teacher.extract_feat(img)
            outs_s = self.student.bbox_head(xs)
            outs_t = self.teacher.bbox_head(xt)
        self.add_outputs(xs, xt, outs_s, outs_t)

    def add_outputs(self, xs, xt, outs_s, outs_t):
        """``add`` for features and head outputs that are already there."""
        pairs = {}
        for fam, s, t in (('feature', xs, xt), ('cls', outs_s[0], outs_t[0]),
                          ('bbox', outs_s[1], outs_t[1])):
            what = f'TeacherStudentDiscrepancy ({fam})'
            ss, ls = _packed_shape(tuple(s), None, what)
            st, lt = _packed_shape(tuple(t), None, what)
            _check_pair(ss, ls, st, lt, what)
            pairs[fam] = (s, t, ls)
        levels = pairs['feature'][2]
        if any(p[2] != levels for p in pairs.values()):
            raise ValueError('TeacherStudentDiscrepancy: the head outputs and '
                             'the features have different levels')
        if self.levels is not None and len(levels) != len(self.levels):
            raise ValueError(f'TeacherStudentDiscrepancy: {len(levels)} levels '
                             f'after {len(self.levels)}')
        self.levels = levels
        for fam, (s, t, lv) in pairs.items():
            s3, t3 = _pack(tuple(s), lv), _pack(tuple(t), lv)
            self._err[fam].append(levels_abs_err(t3, s3, lv))
            if fam == 'feature':
                r, cnt = levels_pearson(t3, s3, lv)
                self._r.append(r)
                self._cnt.append(cnt)
        self._pos.append([h * w for h, w in levels])

    @property
    def num_images(self):
        return sum(int(e.shape[0]) for e in self._err['feature'])

    def compute(self):
        """-> dict: ``feature_error`` / ``cls_error`` / ``bbox_error`` (per
        image the level sums over the image's positions, averaged over the
        images: the reference's numbers at its samples_per_gpu = 1),
        ``*_error_levels`` ((L,): per image the level sum over the level's
        positions, averaged), ``pearson`` ((L,): the mean over the images of
        the per-image mean r over the valid rows; index 2 is the reference's
        P5 number; an image without a valid row at a level is left out, NaN
        without any), ``degenerate_rows`` ((L,) int64) and ``num_images``."""
        if not self._pos:
            raise ValueError('TeacherStudentDiscrepancy.compute: nothing '
                             'was added')
        out = {}
        for fam in _FAMILIES:
            tot, lev = [], []
            for e, pos in zip(self._err[fam], self._pos):
                e = e.cpu().numpy()
                tot.append(e.sum(axis=1) / float(sum(pos)))
                lev.append(e / np.asarray(pos, dtype=np.float64)[None, :])
            out[f'{fam}_error'] = float(np.concatenate(tot).mean())
            out[f'{fam}_error_levels'] = np.concatenate(lev).mean(axis=0)
        r = np.concatenate([x.cpu().numpy() for x in self._r])
        cnt = np.concatenate([x.cpu().numpy() for x in self._cnt]).astype(
            np.int64)
        valid = cnt[..., 0]
        with np.errstate(invalid='ignore', divide='ignore'):
            per_img = np.where(valid > 0, r / valid, np.nan)
            has = (valid > 0).sum(axis=0)
            out['pearson'] = np.where(
                has > 0, np.nansum(per_img, axis=0) / has, np.nan)
        out['degenerate_rows'] = cnt[..., 1].sum(axis=0)
        out['num_images'] = int(r.shape[0])
        return out


# ---------------------------------------------------------------------------
# the AP landscape
# ---------------------------------------------------------------------------
class _Grid(list):
    """The A x B list of ``FeatureLandscape.grid``, row major."""
    shape = None


class FeatureLandscape:
    """AP (or mAP, or recall) at every point ``(a, b)`` of ``coefs``: the head
    of ``head`` ('student' or 'teacher') is fed ``a * x_own + b * x_other`` on
    every level, ``x_own`` the features of the head's own model and
    ``x_other`` those of the other one.  ``coefs=[(0.9, 0.7)]`` is the point
    the reference ships.  ``evaluator_factory()`` returns a fresh
    ``CocoEvaluator``, ``MapAccumulator`` or ``RecallAccumulator``; there is
    one per grid point.  ``chunk``: grid points per head forward (default: as
    many as keep the head's batch ``chunk * N <= 16``).  An ``LDHead`` student
    ignores its teacher here, as ``simple_test`` does."""
    MAX_HEAD_BATCH = 16

    def __init__(self, student, teacher=None, coefs=((0.9, 0.7), ),
                 head='student', evaluator_factory=None, chunk=None):
        if head not in ('student', 'teacher'):
            raise ValueError(f"head: 'student' or 'teacher', got {head!r}")
        if evaluator_factory is None or not callable(evaluator_factory):
            raise ValueError('evaluator_factory: a callable that returns a '
                             'fresh evaluator')
        if chunk is not None and int(chunk) < 1:
            raise ValueError(f'chunk must be >= 1, got {chunk}')
        teacher = _teacher_of(student, teacher)
        self.own, self.other = (student, teacher) if head == 'student' else \
            (teacher, student)
        self.shape = getattr(coefs, 'shape', None)
        self.coefs = _coefs(coefs)
        self.chunk = None if chunk is None else int(chunk)
        self.evaluators = [evaluator_factory() for _ in self.coefs]

    @staticmethod
    def grid(alphas, betas):
        """The A x B points ``(a, b)``, ``a`` major; ``compute`` then returns
        an (A, B) array."""
        alphas, betas = list(alphas), list(betas)
        g = _Grid((float(a), float(b)) for a in alphas for b in betas)
        g.shape = (len(alphas), len(betas))
        if not g:
            raise ValueError('grid: no points')
        return g

    @classmethod
    def chunks(cls, K, N, chunk=None):
        """The ``(k0, k1)`` ranges of grid points that share a head forward
        for a batch of ``N`` images."""
        if chunk is None:
            chunk = max(1, cls.MAX_HEAD_BATCH // max(int(N), 1))
        chunk = max(1, min(int(chunk), L.LD_LEVELS_MIX_MAX_K))
        return [(k0, min(K, k0 + chunk)) for k0 in range(0, K, chunk)]

    def detect(self, img, img_metas, rescale=True):
        """-> per grid point the ``[(dets (k, 5), labels (k,)), ...]`` of the
        batch's images, device tensors."""
        N = int(img.shape[0])
        if len(img_metas) != N:
            raise ValueError(f'{N} images but {len(img_metas)} image metas')
        head = self.own.bbox_head
        with torch.no_grad():
            x_own = self.own.extract_feat(img)
            x_other = self.other.extract_feat(img)
            sa, la = _packed_shape(tuple(x_own), None, 'FeatureLandscape: own')
            sb, lb = _packed_shape(tuple(x_other), None,
                                   'FeatureLandscape: other')
            _check_pair(sa, la, sb, lb, 'FeatureLandscape')
            own3, other3 = _pack(tuple(x_own), la), _pack(tuple(x_other), la)
            out = []
            for k0, k1 in self.chunks(len(self.coefs), N, self.chunk):
                x3, _ = mix_levels(own3, other3, self.coefs[k0:k1], levels=la)
                outs = head.forward_packed(x3, la)
                boxes = head.get_bboxes(
                    *outs, repeat_metas(img_metas, k1 - k0), rescale=rescale)
                out.extend(boxes[j * N:(j + 1) * N] for j in range(k1 - k0))
        return out

    def add(self, img, img_metas, gt=None, rescale=True):
        """One batch: both backbones and necks once, per chunk of grid points
        one mix launch, one head forward and one ``get_bboxes``; each point's
        detections go to its evaluator as device tensors.  ``gt`` is what the
        evaluator's ``add`` takes besides the detections: the dataset indices
        of the images for a ``CocoEvaluator``, ``(gt_bboxes, gt_labels[,
        gt_bboxes_ignore, gt_labels_ignore])`` or a dict of them for a
        ``MapAccumulator``, the ``gt_bboxes`` list for a
        ``RecallAccumulator``."""
        for ev, boxes in zip(self.evaluators,
                             self.detect(img, img_metas, rescale)):
            _feed(ev, boxes, gt)

    def compute(self):
        """-> each evaluator's ``compute()``: a list in ``coefs`` order, or the
        (A, B) object array of a ``grid``."""
        res = [ev.compute() for ev in self.evaluators]
        if self.shape is None:
            return res
        arr = np.empty(len(res), dtype=object)
        for i, r in enumerate(res):
            arr[i] = r
        return arr.reshape(self.shape)


def _feed(ev, boxes, gt):
    from .coco_eval import _CocoStream
    from .evaluation import MapAccumulator
    from .recall import RecallAccumulator
    dets, labels = [b[0] for b in boxes], [b[1] for b in boxes]
    if isinstance(ev, _CocoStream):
        ev.add(gt, dets, labels)
    elif isinstance(ev, MapAccumulator):
        if isinstance(gt, dict):
            ev.add(dets, labels, **gt)
        else:
            ev.add(dets, labels, *gt)
    elif isinstance(ev, RecallAccumulator):
        ev.add(dets, gt)
    else:
        raise TypeError(
            f'FeatureLandscape: {type(ev).__name__} is not a CocoEvaluator, '
            'MapAccumulator or RecallAccumulator')
