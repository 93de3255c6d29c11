"""Host plumbing that the device evaluators share (``evaluation``,
``analyze_results``, ``coco_eval``, ``coco_analysis``, ``recall``): the device
and rank guards, the logger choice, the conversion and packing of per-image
lists, the reference's result lists, and the growing record buffers.  Nothing
here launches a kernel; the device side of the family is
``csrc/eval_common.h``.
"""
import logging

import numpy as np
import torch

from . import lib as L

ADD_STEP = 512  # images per ``add`` of the list interfaces


def eval_device(device, who):
    """``device`` (default: the current HIP device) as a torch.device; any
    other kind of device is refused."""
    dev = torch.device(device) if device is not None else \
        torch.device('cuda', torch.cuda.current_device())
    if dev.type != 'cuda':
        raise L.LdError(f'{who}: device {dev} is not a HIP device (there is '
                        'no CPU path)')
    return dev


def eval_logger(logger, default):
    """A Logger as it is, a logger name looked up, anything else (None,
    'silent') -> ``default``, the calling module's logger."""
    if isinstance(logger, logging.Logger):
        return logger
    if isinstance(logger, str) and logger != 'silent':
        return logging.getLogger(logger)
    return default


def check_one_rank(who):
    """Results are not gathered across ranks: refuse a multi-rank run."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and \
            dist.get_world_size() > 1:
        raise NotImplementedError(
            f'{who}: results are not gathered across ranks (world size '
            f'{dist.get_world_size()}); evaluate on one rank, or gather the '
            'detections there first')


def as_boxes(x, dev, last):
    """-> fp32 (n, last) on ``dev``; anything empty is (0, last)."""
    t = torch.as_tensor(x)
    if t.numel() == 0:
        t = t.reshape(0, last)
    return t.to(device=dev, dtype=torch.float32).reshape(-1, last)


def as_labels(x, dev):
    """-> int64 (n,) on ``dev``."""
    return torch.as_tensor(x).to(device=dev, dtype=torch.int64).reshape(-1)


def pack_rows(rows, dev, who='pack_rows'):
    """Per-image tensors of one trailing shape -> (their concatenation,
    int32 offsets (len(rows) + 1,) on ``dev``, host list of the counts).
    Rows may be empty, all of them too; 2**31 rows or more are refused."""
    counts = [r.shape[0] for r in rows]
    if sum(counts) >= 2 ** 31:
        raise L.LdError(f'{who}: batch too large')
    off = np.zeros(len(counts) + 1, dtype=np.int32)
    off[1:] = np.cumsum(counts)
    return torch.cat(rows).contiguous(), torch.from_numpy(off).to(dev), counts


_BATCH_KEYS = ('dets', 'det_labels', 'det_off', 'gts', 'gt_labels', 'gt_off',
               'ign', 'ign_labels', 'ign_off')


def pack_det_gt_batch(who, det_names, dets, labels, gt_bboxes, gt_labels,
                      gt_bboxes_ignore, gt_labels_ignore, dev):
    """The argument checks and the packing of ``MapAccumulator.add`` and
    ``ImageMapAnalyzer.add``: per-image lists of detections (n, 5) with labels
    (n,), GTs (g, 4) / (g,) and optionally ignored GTs -> the dict of nine
    device tensors that ``eval_batch`` reads, or None for no images.  ``who``
    and ``det_names`` (how the caller names ``dets`` and ``labels``) go into
    the messages."""
    B = len(dets)
    if not (len(labels) == len(gt_bboxes) == len(gt_labels) == B):
        raise ValueError(f'{who}: {det_names[0]}, {det_names[1]}, gt_bboxes '
                         'and gt_labels need one entry per image')
    if (gt_bboxes_ignore is None) != (gt_labels_ignore is None):
        raise ValueError(f'{who}: gt_bboxes_ignore and gt_labels_ignore go '
                         'together')
    if gt_bboxes_ignore is not None and not \
            len(gt_bboxes_ignore) == len(gt_labels_ignore) == B:
        raise ValueError(f'{who}: one ignored-GT entry per image')
    if B == 0:
        return None
    d = [as_boxes(x, dev, 5) for x in dets]
    dl = [as_labels(x, dev) for x in labels]
    g = [as_boxes(x, dev, 4) for x in gt_bboxes]
    gl = [as_labels(x, dev) for x in gt_labels]
    if gt_bboxes_ignore is None:
        ig = [torch.zeros((0, 4), dtype=torch.float32, device=dev)] * B
        il = [torch.zeros((0, ), dtype=torch.int64, device=dev)] * B
    else:
        ig = [as_boxes(x, dev, 4) for x in gt_bboxes_ignore]
        il = [as_labels(x, dev) for x in gt_labels_ignore]
    for boxes, labs, what in ((d, dl, 'detections'), (g, gl, 'GTs'),
                              (ig, il, 'ignored GTs')):
        for x, y in zip(boxes, labs):
            if x.shape[0] != y.shape[0]:
                raise ValueError(f'{who}: {what} and their labels differ in '
                                 'length')
    batch = {}
    for key, off, lab, boxes, labs in (
            ('dets', 'det_off', 'det_labels', d, dl),
            ('gts', 'gt_off', 'gt_labels', g, gl),
            ('ign', 'ign_off', 'ign_labels', ig, il)):
        batch[key], batch[off], _ = pack_rows(boxes, dev, who)
        batch[lab] = torch.cat(labs).contiguous()
    return batch


def eval_batch(batch):
    """The dict of ``pack_det_gt_batch`` -> ``L.EvalBatchT`` (pointers and
    counts; the dict keeps the tensors alive)."""
    b = L.EvalBatchT()
    for k in _BATCH_KEYS:
        setattr(b, k, L.ptr(batch[k]).value)
    b.num_imgs = batch['det_off'].numel() - 1
    b.num_dets = batch['dets'].shape[0]
    b.num_gts = batch['gts'].shape[0]
    b.num_ign = batch['ign'].shape[0]
    return b


def results_to_lists(results, annotations, num_classes, bbox_segm=False):
    """The reference's list forms -> the six per-image lists that the ``add``
    of ``MapAccumulator`` / ``ImageMapAnalyzer`` takes.  ``results[i][c]``:
    (k, 5) arrays per image and class; ``annotations[i]``: dicts of ``bboxes``
    / ``labels`` and optional ``bboxes_ignore`` / ``labels_ignore``.  With
    ``bbox_segm`` a ``(bbox, segm)`` tuple stands for its bbox part
    (analyze_results.py:33-34)."""
    if len(results) != len(annotations):
        raise ValueError('add_results: one annotation per image')
    dets, labels, gb, gl, ib, il = [], [], [], [], [], []
    for res, ann in zip(results, annotations):
        if bbox_segm and isinstance(res, tuple):
            res = res[0]
        if len(res) != num_classes:
            raise ValueError(f'add_results: {len(res)} class arrays, '
                             f'expected {num_classes}')
        rows = [np.asarray(r, dtype=np.float32).reshape(-1, 5) for r in res]
        dets.append(np.concatenate(rows))
        labels.append(np.concatenate([
            np.full((r.shape[0], ), c, dtype=np.int64)
            for c, r in enumerate(rows)]))
        gb.append(np.asarray(ann['bboxes'], dtype=np.float32).reshape(-1, 4))
        gl.append(np.asarray(ann['labels']).reshape(-1))
        # get_cls_results (mean_ap.py:258-262): labels_ignore decides
        if ann.get('labels_ignore', None) is not None:
            ib.append(np.asarray(ann['bboxes_ignore'],
                                 dtype=np.float32).reshape(-1, 4))
            il.append(np.asarray(ann['labels_ignore']).reshape(-1))
        else:
            ib.append(np.zeros((0, 4), dtype=np.float32))
            il.append(np.zeros((0, ), dtype=np.int64))
    return dets, labels, gb, gl, ib, il


class RecordBuffers:
    """Named 1-D device tensors of one length that grow together: ``n``
    records are written, ``reserve(extra)`` makes room for more, keeping what
    is written.  ``fields``: ``{name: dtype}``; ``floor``: the least capacity
    once anything is reserved."""

    def __init__(self, fields, device, floor):
        self.device, self.floor, self.n, self.capacity = \
            device, int(floor), 0, 0
        self._t = {name: torch.empty(0, dtype=dt, device=device)
                   for name, dt in fields.items()}

    def reserve(self, extra):
        need = self.n + extra
        if need <= self.capacity:
            return
        cap = self.capacity = max(need, 2 * self.capacity, self.floor)
        for name, old in self._t.items():
            new = torch.empty(cap, dtype=old.dtype, device=self.device)
            new[:self.n] = old[:self.n]
            self._t[name] = new

    def __getitem__(self, name):
        """The whole buffer of ``name`` (its first ``n`` entries are
        written)."""
        return self._t[name]

    def views(self, lo=0, hi=None):
        """{name: buffer[lo:hi]}; by default the written part."""
        hi = self.n if hi is None else hi
        return {name: t[lo:hi] for name, t in self._t.items()}
