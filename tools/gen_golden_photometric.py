"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/photometric.npz by EXECUTING
THE REFERENCE's PhotoMetricDistortion, Expand, MinIoURandomCrop, Resize,
RandomFlip, Normalize and Pad on the CPU (the reference package is imported,
unmodified, through oracle/ref_shim.py).  Run from the repo root in the build
container, never on the GPU machine:

    python tools/gen_golden_photometric.py

Reference entry points exercised (file:line under the reference tree):
  mmdet/datasets/pipelines/transforms.py:810-912    PhotoMetricDistortion
  mmdet/datasets/pipelines/transforms.py:916-1004   Expand
  mmdet/datasets/pipelines/transforms.py:1008-1144  MinIoURandomCrop
  mmdet/datasets/pipelines/transforms.py:26-315     Resize
  mmdet/datasets/pipelines/transforms.py:319-472    RandomFlip
  mmdet/datasets/pipelines/transforms.py:476-585    Pad, Normalize
  configs/...                                       the STOCK train_pipelines

mmcv and cv2 are absent, so the pixel functions the reference calls are stubs
that live HERE, restated from their published behaviour:
``mmcv.bgr2hsv`` / ``mmcv.hsv2bgr`` (the two conversions of
tests/_photometric_oracle.py), ``imresize`` / ``imrescale`` (its float
INTER_LINEAR), ``imnormalize``, ``impad``, ``impad_to_multiple``, ``imflip``.
So what this file PINS is what the reference's own classes decide: the order
of the draws, the order of the chain, how the drawn Python floats round when
numpy applies them to a float32 image, the hue wraps, the permutation, that
nothing clips, the float canvas fill, and the geometry after the photometric
draws.  It does NOT pin cv2's HSV conversions or float resize.

``transforms.random`` (numpy.random) is wrapped by a recorder, so the draws are
read from what the class itself called, in its order; the tool then checks
that the oracle chain with those draws gives the class's output bit for bit.

Stored per chain case ``pmd_s<seed>`` (the class alone on the 8 x 8 palette
image): ``_flags`` (brightness, contrast, saturation, hue, permutation taken),
``_draws`` (delta, alpha, saturation, hue as drawn, float64; 0 when skipped),
``_mode``, ``_perm``, ``_next`` (np.random.random_sample() after the run),
``_out`` (the pixels).  Per full case ``ssd_s<seed>`` / ``yolo_s<seed>`` the
same plus ``_out`` of the whole pipeline and the geometry fields of the
augment golden (``_canvas``, ``_window``, ``_resized``, ``_img_shape``,
``_pad_shape``, ``_scale_factor``, ``_flip``, ``_mode_iou``, ``_gt_bboxes``,
``_gt_labels``).  ``pmd_seeds`` / ``ssd_seeds`` / ``yolo_seeds``: the seeds.
``stock_names`` / ``stock_pipelines``: the STOCK configs' train_pipeline lists
as JSON strings (settings only).
"""
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'oracle'))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)

import ref_shim  # noqa: E402

ref_shim.install()

import _photometric_cases as PC  # noqa: E402
import _photometric_oracle as PO  # noqa: E402


# ---------------------------------------------------------------------------
# stubs of the mmcv pixel functions
# ---------------------------------------------------------------------------
def _rescale_size(old_size, scale):
    w, h = old_size
    factor = min(max(scale) / max(h, w), min(scale) / min(h, w))
    return int(w * float(factor) + 0.5), int(h * float(factor) + 0.5), factor


def _imrescale(img, scale, return_scale=False, **kw):
    h, w = img.shape[:2]
    new_w, new_h, factor = _rescale_size((w, h), scale)
    out = PO.resize_linear_f32(img, new_h, new_w)
    return (out, factor) if return_scale else out


def _imresize(img, size, return_scale=False, **kw):
    h, w = img.shape[:2]
    out = PO.resize_linear_f32(img, size[1], size[0])
    return (out, size[0] / w, size[1] / h) if return_scale else out


def _impad(img, shape=None, pad_val=0, **kw):
    assert shape[0] >= img.shape[0] and shape[1] >= img.shape[1]
    out = np.full(tuple(shape[:2]) + img.shape[2:], pad_val, img.dtype)
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
    mmcv.bgr2hsv, mmcv.hsv2bgr = PO.bgr2hsv, PO.hsv2bgr
    mmcv.imrescale, mmcv.imresize = _imrescale, _imresize
    mmcv.impad, mmcv.impad_to_multiple = _impad, _impad_to_multiple
    mmcv.imflip, mmcv.is_list_of = _imflip, _is_list_of
    mmcv.imnormalize = PO.normalize


class Recorder:
    """numpy.random with a log of (name, result) of every call."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        fn = getattr(np.random, name)

        def call(*a, **k):
            r = fn(*a, **k)
            self.log.append((name, r))
            return r
        return call


def read_draws(log):
    """The class's own calls -> flags and values.  The walk follows
    transforms.py:858-899 and fails when a call is not the one expected
    there, so it cannot invent an order."""
    it = iter(log)

    def take(name):
        n, r = next(it)
        assert n == name, (n, name)
        return r

    d = dict(delta=None, alpha=None, saturation=None, hue=None, perm=None)
    if take('randint'):
        d['delta'] = float(take('uniform'))
    d['mode'] = int(take('randint'))
    if d['mode'] == 1 and take('randint'):
        d['alpha'] = float(take('uniform'))
    if take('randint'):
        d['saturation'] = float(take('uniform'))
    if take('randint'):
        d['hue'] = float(take('uniform'))
    if d['mode'] == 0 and take('randint'):
        d['alpha'] = float(take('uniform'))
    if take('randint'):
        d['perm'] = tuple(int(v) for v in take('permutation'))
    assert next(it, None) is None, 'calls left over'
    return d


def store_photo(d, photo):
    keys = ('delta', 'alpha', 'saturation', 'hue')
    d['flags'] = np.array([photo[k] is not None for k in keys] +
                          [photo['perm'] is not None])
    d['draws'] = np.array([photo[k] or 0.0 for k in keys], np.float64)
    d['mode'] = np.int64(photo['mode'])
    d['perm'] = np.array(photo['perm'] or (0, 1, 2), np.int64)


def coord_image(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([yy, xx, np.ones_like(yy)], -1).astype(np.float32)


def run_chain(seed, step=PC.PMD):
    from mmdet.datasets.pipelines import transforms as T
    img = PC.palette_image().astype(np.float32)
    rec = Recorder()
    T.random = rec
    try:
        np.random.seed(seed)
        kw = {k: v for k, v in step.items() if k != 'type'}
        res = T.PhotoMetricDistortion(**kw)(dict(img=img.copy(),
                                                 img_fields=['img']))
        nxt = np.random.random_sample()
    finally:
        T.random = np.random
    photo = read_draws(rec.log)
    out = np.ascontiguousarray(res['img'])
    assert out.dtype == np.float32
    # the oracle chain with the class's draws is the class's output
    assert PO.chain(img, photo).tobytes() == out.tobytes(), seed
    d = dict(next=nxt, out=out)
    store_photo(d, photo)
    return d, photo, PO.hue_wraps(img, photo)


def run_full(kind, seed, pixels):
    """One full pipeline under ``seed``.  ``pixels``: the palette image all
    the way (the output pixels); else, after the distortion, the image is
    swapped for (y, x, 1) coordinates before every step, so that what a step
    returns tells where its window starts (the geometry)."""
    from mmdet.datasets.pipelines import transforms as T
    img = PC.palette_image().astype(np.float32)
    h, w = img.shape[:2]
    results = dict(
        img=img.copy(), img_shape=(h, w, 3), ori_shape=(h, w, 3),
        img_fields=['img'], gt_bboxes=PC.BOXES.copy(),
        gt_labels=PC.LABELS.copy(), gt_bboxes_ignore=PC.IGNORE.copy(),
        bbox_fields=['gt_bboxes_ignore', 'gt_bboxes'], mask_fields=[],
        seg_fields=[])
    d = dict(canvas=(h, w, 0, 0), window=(0, 0, h, w), mode_iou=-1.0)
    rec = Recorder()
    T.random = rec
    try:
        np.random.seed(seed)
        for step in PC.FULL[kind]:
            kw = {k: v for k, v in step.items() if k != 'type'}
            t = step['type']
            if t == 'PhotoMetricDistortion':
                results = T.PhotoMetricDistortion(**kw)(results)
                photo = read_draws(rec.log)
            elif t == 'Expand':
                if not pixels:
                    kw['mean'] = (0, 0, 0)  # the fill marks what is not image
                    results['img'] = coord_image(h, w)
                results = T.Expand(**kw)(results)
                if not pixels:
                    im = results['img']
                    top, left = [int(v[0]) for v in np.nonzero(im[..., 2])]
                    d['canvas'] = (im.shape[0], im.shape[1], top, left)
                    d['window'] = (0, 0, im.shape[0], im.shape[1])
            elif t == 'MinIoURandomCrop':
                if not pixels:
                    results['img'] = coord_image(*results['img'].shape[:2])
                tr = T.MinIoURandomCrop(**kw)
                results = tr(results)
                d['mode_iou'] = float(tr.mode)
                if not pixels:
                    im = results['img']
                    d['window'] = (int(im[0, 0, 0]), int(im[0, 0, 1]),
                                   im.shape[0], im.shape[1])
            elif t == 'Resize':
                results = T.Resize(**kw)(results)
                d['resized'] = results['img'].shape[:2]
            elif t in ('RandomFlip', 'Normalize', 'Pad'):
                results = getattr(T, t)(**kw)(results)
            else:
                raise KeyError(t)
        d['next'] = np.random.random_sample()
    finally:
        T.random = np.random
    for k in ('scale_factor', 'flip', 'gt_bboxes', 'gt_labels'):
        d[k] = results[k]
    d['img_shape'] = tuple(results['img_shape'])[:2] + (3,)
    d['pad_shape'] = tuple(results.get('pad_shape',
                                       results['img_shape']))[:2] + (3,)
    d['out'] = np.ascontiguousarray(results['img'])
    store_photo(d, photo)
    return d


def full_case(kind, seed):
    a, b = run_full(kind, seed, True), run_full(kind, seed, False)
    # the pixels do not steer a draw: both passes made the same ones
    assert a['next'] == b['next'] and a['img_shape'] == b['img_shape']
    np.testing.assert_array_equal(a['gt_bboxes'], b['gt_bboxes'])
    for k in ('canvas', 'window'):
        a[k] = b[k]
    assert a['out'].dtype == np.float32
    return a


def stock_pipelines():
    import mmcv
    from ref_shim import REFERENCE_ROOT
    names, texts = [], []
    for rel in PC.STOCK:
        cfg = mmcv.Config.fromfile(os.path.join(REFERENCE_ROOT, rel))
        steps = json.loads(json.dumps(cfg.train_pipeline))
        types = [s['type'] for s in steps]
        assert types[0] == 'LoadImageFromFile' and steps[0]['to_float32']
        assert 'PhotoMetricDistortion' in types, rel
        names.append(rel)
        texts.append(json.dumps(steps, sort_keys=True))
    return names, texts


def main():
    install_stubs()
    d = {}
    # -- the class alone: add seeds until every edge is reached -------------
    need = {'mode0', 'mode1', 'wrap_up', 'wrap_down', 'perm_identity',
            'perm_other'}
    for k in ('brightness', 'contrast', 'saturation', 'hue', 'perm'):
        need |= {k + '_taken', k + '_skipped'}
    seeds, seen = [], set()
    seed = 0
    while not need <= seen:
        assert seed < 200, sorted(need - seen)
        r, photo, (up, down) = run_chain(seed)
        new = {f'mode{photo["mode"]}'}
        for k, key in (('brightness', 'delta'), ('contrast', 'alpha'),
                       ('saturation', 'saturation'), ('hue', 'hue'),
                       ('perm', 'perm')):
            new.add(k + ('_taken' if photo[key] is not None else '_skipped'))
        if up:
            new.add('wrap_up')
        if down:
            new.add('wrap_down')
        if photo['perm'] is not None:
            new.add('perm_identity' if photo['perm'] == (0, 1, 2)
                    else 'perm_other')
        if not new <= seen:
            seen |= new
            seeds.append(seed)
            for k, v in r.items():
                d[f'pmd_s{seed}_{k}'] = np.asarray(v)
            print(f'[photometric] pmd_s{seed}: {photo} wraps {up, down}',
                  flush=True)
        seed += 1
    d['pmd_seeds'] = np.array(seeds, np.int64)
    # -- the two full pipelines: Expand taken and skipped, a crop patch ------
    for kind in ('ssd', 'yolo'):
        seeds, seen, seed = [], set(), 0
        need = {'expand', 'no_expand', 'patch', 'no_patch', 'flip', 'no_flip'}
        while not need <= seen:
            assert seed < 200, sorted(need - seen)
            r = full_case(kind, seed)
            h, w = PC.palette_image().shape[:2]
            new = {'expand' if r['canvas'][:2] != (h, w) else 'no_expand',
                   'patch' if r['window'][2:] != r['canvas'][:2]
                   else 'no_patch', 'flip' if r['flip'] else 'no_flip'}
            if not new <= seen:
                seen |= new
                seeds.append(seed)
                for k, v in r.items():
                    d[f'{kind}_s{seed}_{k}'] = np.asarray(v)
                print(f"[photometric] {kind}_s{seed}: canvas {r['canvas']} "
                      f"window {r['window']} resized {r['resized']} -> "
                      f"{r['pad_shape'][:2]} flip {r['flip']}", flush=True)
            seed += 1
        d[f'{kind}_seeds'] = np.array(seeds, np.int64)
    names, texts = stock_pipelines()
    d['stock_names'], d['stock_pipelines'] = np.array(names), np.array(texts)
    out = os.path.join(REPO, 'tests', 'golden', 'photometric.npz')
    with zipfile.ZipFile(out, 'w', zipfile.ZIP_DEFLATED) as z:
        for k in sorted(d):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, d[k], allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print('[photometric] wrote', out, os.path.getsize(out), 'bytes')
    assert os.path.getsize(out) < (1 << 20)


if __name__ == '__main__':
    main()
