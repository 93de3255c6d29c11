"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/augment.npz by EXECUTING THE
REFERENCE's train-time augmentations on the CPU (the reference package is
imported, unmodified, through oracle/ref_shim.py).  Run from the repo root in
the build container, never on the GPU machine:

    python tools/gen_golden_augment.py

Reference entry points exercised (file:line under the reference tree):
  mmdet/datasets/pipelines/transforms.py:916-1004   Expand
  mmdet/datasets/pipelines/transforms.py:1008-1144  MinIoURandomCrop
  mmdet/datasets/pipelines/transforms.py:26-315     Resize (scale draw, bboxes)
  mmdet/datasets/pipelines/transforms.py:588-768    RandomCrop
  mmdet/datasets/pipelines/transforms.py:319-472    RandomFlip
  mmdet/datasets/pipelines/transforms.py:476-543    Pad
  mmdet/core/evaluation/bbox_overlaps.py            (through MinIoURandomCrop)

The cases are tests/_augment_cases.py; each runs its ``steps`` in order under
``np.random.seed(seed)`` on a results dict as LoadAnnotations leaves it
(bbox_fields = [gt_bboxes_ignore, gt_bboxes]).  No pixels: the "image" is an
int32 array whose channels are (y, x, 1), so the first element of what a
transform returns tells where its window starts, and the place of the 1s tells
where Expand put the image.  Stubs that live here, not in ref_shim, restated
from mmcv's public behaviour and returning shapes only: ``mmcv.imrescale``
(rescale_size), ``imresize``, ``impad``, ``impad_to_multiple``, ``imflip``,
``is_list_of``.  Normalize is skipped (no draw, no geometry).

Stored per case ``C``: ``C_rejected``; ``C_next`` (np.random.random_sample()
after the run: the number of draws); when not rejected ``C_canvas`` (h, w,
top, left), ``C_window`` (y, x, h, w), ``C_resized`` (h, w), ``C_crop`` (y, x),
``C_img_shape``, ``C_pad_shape``, ``C_scale_factor``, ``C_flip``, ``C_mode``
(MinIoURandomCrop's last mode, -1 without it), ``C_gt_bboxes``,
``C_gt_labels``, ``C_gt_bboxes_ignore``, ``C_gt_labels_ignore``.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'oracle'))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)

import gen_golden as G  # noqa: E402,F401  (installs ref_shim)

import _augment_cases as AC  # noqa: E402


def coord_image(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([yy, xx, np.ones_like(yy)], -1).astype(np.int32)


def _rescale_size(old_size, scale):
    w, h = old_size
    factor = min(max(scale) / max(h, w), min(scale) / min(h, w))
    return int(w * float(factor) + 0.5), int(h * float(factor) + 0.5)


def _imrescale(img, scale, return_scale=False, **kw):
    h, w = img.shape[:2]
    new_w, new_h = _rescale_size((w, h), scale)
    out = np.zeros((new_h, new_w) + img.shape[2:], img.dtype)
    factor = min(max(scale) / max(h, w), min(scale) / min(h, w))
    return (out, factor) if return_scale else out


def _imresize(img, size, return_scale=False, **kw):
    h, w = img.shape[:2]
    out = np.zeros((size[1], size[0]) + img.shape[2:], img.dtype)
    return (out, size[0] / w, size[1] / h) if return_scale else out


def _impad(img, shape=None, pad_val=0, **kw):
    assert shape[0] >= img.shape[0] and shape[1] >= img.shape[1]
    out = np.zeros(tuple(shape[:2]) + img.shape[2:], img.dtype)
    out[:img.shape[0], :img.shape[1]] = img
    return out


def _impad_to_multiple(img, divisor, pad_val=0):
    pad_h = int(np.ceil(img.shape[0] / divisor)) * divisor
    pad_w = int(np.ceil(img.shape[1] / divisor)) * divisor
    return _impad(img, shape=(pad_h, pad_w), pad_val=pad_val)


def _imflip(img, direction='horizontal'):
    assert direction == 'horizontal'
    return np.flip(img, axis=1)


def _is_list_of(seq, expected_type):
    return isinstance(seq, list) and all(isinstance(x, expected_type)
                                         for x in seq)


def install_stubs():
    import mmcv
    mmcv.imrescale, mmcv.imresize = _imrescale, _imresize
    mmcv.impad, mmcv.impad_to_multiple = _impad, _impad_to_multiple
    mmcv.imflip, mmcv.is_list_of = _imflip, _is_list_of


def run_case(case):
    """The reference's transforms of ``case`` in order -> a dict of what they
    returned (see the module docstring)."""
    from mmdet.datasets.pipelines import transforms as T
    name, seed, (h, w), boxes, labels, ignore, steps = case
    results = dict(
        img=coord_image(h, w), img_shape=(h, w, 3), ori_shape=(h, w, 3),
        img_fields=['img'], gt_bboxes=boxes.copy(), gt_labels=labels.copy(),
        gt_bboxes_ignore=ignore.copy(),
        gt_labels_ignore=np.zeros(len(ignore), np.int64),
        bbox_fields=['gt_bboxes_ignore', 'gt_bboxes'], mask_fields=[],
        seg_fields=[])
    d = dict(canvas=(h, w, 0, 0), window=(0, 0, h, w), crop=(0, 0), mode=-1.0)
    np.random.seed(seed)
    for step in steps:
        kw = {k: v for k, v in step.items() if k != 'type'}
        t = step['type']
        if t == 'Normalize':
            continue
        if t == 'Expand':
            kw['mean'] = (0, 0, 0)  # the fill marks what is not image
            results = T.Expand(**kw)(results)
            img = results['img']
            top, left = [int(v[0]) for v in np.nonzero(img[..., 2])]
            d['canvas'] = (img.shape[0], img.shape[1], top, left)
            d['window'] = (0, 0, img.shape[0], img.shape[1])
            results['img'] = coord_image(*img.shape[:2])
        elif t == 'MinIoURandomCrop':
            tr = T.MinIoURandomCrop(**kw)
            results = tr(results)
            img = results['img']
            d['mode'] = float(tr.mode)
            d['window'] = (int(img[0, 0, 0]), int(img[0, 0, 1]), img.shape[0],
                           img.shape[1])
        elif t == 'Resize':
            results = T.Resize(**kw)(results)
            d['resized'] = results['img'].shape[:2]
            results['img'] = coord_image(*d['resized'])
        elif t == 'RandomCrop':
            results = T.RandomCrop(**kw)(results)
            if results is None:
                break
            img = results['img']
            d['crop'] = (int(img[0, 0, 0]), int(img[0, 0, 1]))
        elif t == 'RandomFlip':
            results = T.RandomFlip(**kw)(results)
        elif t == 'Pad':
            results = T.Pad(**kw)(results)
        else:
            raise KeyError(t)
    d['next'] = np.random.random_sample()
    d['rejected'] = results is None
    if results is not None:
        for k in ('img_shape', 'pad_shape', 'scale_factor', 'flip',
                  'gt_bboxes', 'gt_labels', 'gt_bboxes_ignore',
                  'gt_labels_ignore'):
            d[k] = results[k]
        d['img_shape'] = tuple(results['img_shape'])[:2] + (3,)
        d['pad_shape'] = tuple(results['pad_shape'])[:2] + (3,)
    return d


def check_coverage(runs):
    """The edges the cases are there for, on the reference's own outputs."""
    by = {c[0]: (c, r) for c, r in runs}
    assert by['jitter_rejected'][1]['rejected']
    assert by['jitter_no_boxes_rejected'][1]['rejected']
    r = by['jitter_negative_empty'][1]
    assert not r['rejected'] and len(r['gt_bboxes']) == 0
    r = by['jitter_small_image'][1]
    assert r['img_shape'][0] < 64 and r['img_shape'][1] < 64
    types = {s.get('crop_type', 'absolute') for c, _ in runs for s in c[6]
             if s['type'] == 'RandomCrop'}
    assert types == {'absolute', 'absolute_range', 'relative',
                     'relative_range'}, types
    modes = {r['mode'] for _, r in runs}
    assert modes >= {1.0, 0.1, 0.3, 0.5, 0.7, 0.9, 0.0}, modes
    expanded = {r['canvas'][:2] != c[2] for c, r in runs
                if any(s['type'] == 'Expand' for s in c[6])}
    assert expanded == {True, False}, expanded
    assert any(len(r['gt_bboxes_ignore']) for _, r in runs
               if not r['rejected'])
    # a box centre exactly on the patch border (strict comparison drops it)
    c, r = by['miniou_center_on_border']
    y, x, hh, ww = r['window']
    cx = (c[3][:, 0] + c[3][:, 2]) / 2
    assert (cx == x).any() and len(r['gt_bboxes']) == len(c[3]) - 1


def main():
    install_stubs()
    d, runs = {}, []
    for case in AC.CASES:
        r = run_case(case)
        runs.append((case, r))
        for k, v in r.items():
            d[f'{case[0]}_{k}'] = np.asarray(v)
        print(f'[augment] {case[0]}:', 'rejected' if r['rejected'] else
              f"canvas {r['canvas']} window {r['window']} resized "
              f"{r['resized']} crop {r['crop']} -> {r['img_shape'][:2]} "
              f"mode {r['mode']} flip {r['flip']} boxes "
              f"{len(r['gt_bboxes'])}+{len(r['gt_bboxes_ignore'])}",
              flush=True)
    check_coverage(runs)
    out = os.path.join(REPO, 'tests', 'golden', 'augment.npz')
    # np.savez stamps every member with the wall clock; fixed stamps make the
    # file itself, not only its arrays, a pure function of this script
    with zipfile.ZipFile(out, 'w', zipfile.ZIP_DEFLATED) as z:
        for k in sorted(d):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, d[k], allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print('[augment] wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
