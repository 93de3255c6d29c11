"""GPU tests (-m gpu) of the float-image mode of the input launch
(csrc/pipeline.hip, ``ld_preprocess_batch_photo``): PhotoMetricDistortion on
every tap, the float canvas fill, the float resize.  Everything is compared
bit for bit (as uint32 words) against the numpy float32 composition in
tests/_photometric_oracle.py: the kernel uses only correctly rounded fp32
+ - * /, compares, floors and int conversions, and is built with
-ffp-contract=off.

What the oracle itself is pinned on is in tests/test_photometric_host.py
(the reference's own classes for the order of everything; NOT cv2 for the two
HSV conversions and the float resize)."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _augment_oracle as AO  # noqa: E402
import _dataset_fixture as FX  # noqa: E402
import _photometric_cases as PC  # noqa: E402
import _photometric_oracle as PO  # noqa: E402

pytestmark = pytest.mark.gpu

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
DEV = 'cuda:0'
F = np.float32


def _pipe(**kw):
    from ld_amd.pipeline import DevicePipeline
    kw = dict(dict(mean=MEAN, std=STD, to_rgb=True, size_divisor=None,
                   flip_ratio=0.0, device=DEV, to_float32=True), **kw)
    return DevicePipeline(**kw)


def _plan(img, img_shape, flip=False, **rest):
    h, w = img.shape[:2]
    return dict(ori_shape=(h, w, 3), img_shape=tuple(img_shape) + (3,),
                scale_factor=np.ones(4, np.float32), flip=flip, **rest)


def _photo(delta=None, mode=0, alpha=None, saturation=None, hue=None,
           perm=None):
    return dict(delta=delta, mode=mode, alpha=alpha, saturation=saturation,
                hue=hue, perm=perm)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(pipe, imgs, plans):
    out = pipe(imgs, plans=plans)
    torch.cuda.synchronize()
    got = out['img'].cpu().numpy()
    _, _, Hp, Wp = got.shape
    for i, (im, p) in enumerate(zip(imgs, plans)):
        ref = PO.augment(im, p, pipe.mean, pipe.std, pipe.to_rgb, Hp, Wp,
                         pipe.pad_val)
        np.testing.assert_array_equal(_bits(got[i]), _bits(ref),
                                      err_msg=f'image {i}')
    return got, out


def _images(rs, shapes):
    out = []
    for h, w in shapes:
        yy, xx = np.mgrid[0:h, 0:w]
        base = (np.sin(yy / 7.0)[..., None] * 60 + np.cos(xx / 5.0)[..., None] *
                60 + 128 + rs.randn(h, w, 3) * 25)
        out.append(np.clip(base, 0, 255).astype(np.uint8))
    return out


# 1 ---------------------------------------------------------------------------
# (B, G, R): the edge pixels, then every pair of the values below (ties in
# every channel pair at both ends), then seeded noise
EDGES = PC.PALETTE + [
    (0, 0, 1), (255, 255, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255),
    (17, 17, 17), (1, 0, 0), (0, 1, 0), (254, 255, 255), (128, 127, 128)]


def _palette():
    img = PC.palette_image(16, 16, seed=11).reshape(-1, 3)
    img[:len(EDGES)] = np.asarray(EDGES, np.uint8)
    vals = (0, 30, 255)
    trip = np.asarray(list(itertools.product(vals, repeat=3)), np.uint8)
    img[len(EDGES):len(EDGES) + len(trip)] = trip
    return np.ascontiguousarray(img.reshape(16, 16, 3))


ALL = dict(delta=-31.7, alpha=1.49, saturation=1.5, hue=17.3, perm=(2, 0, 1))
PALETTE_CASES = dict(
    round_trip_only=_photo(),
    brightness_down=_photo(delta=-31.7),          # negative values
    brightness_up=_photo(delta=31.99),
    contrast_before=_photo(mode=1, alpha=1.49),   # above 255 into the HSV step
    contrast_after=_photo(mode=0, alpha=0.51),
    saturation_up=_photo(saturation=1.5),         # S > 1
    saturation_down=_photo(saturation=0.5),
    hue_up=_photo(hue=17.3),                      # wraps > 360
    hue_down=_photo(hue=-17.9),                   # wraps < 0
    hue_to_360_from_below_zero=_photo(hue=-1e-6),  # red: 0 - 1e-6 + 360 = 360
    hue_to_0_and_360=_photo(hue=-120.0),          # green -> 0, blue -> 120
    hue_to_360=_photo(hue=120.0),                 # blue: 240 + 120 = 360, kept
    all_mode0=_photo(mode=0, **ALL),
    all_mode1=_photo(mode=1, **ALL),
    **{'perm_%d%d%d' % p: _photo(perm=p)
       for p in itertools.permutations(range(3))})


@pytest.fixture(scope='module')
def palette_run():
    """All palette cases as ONE batch (one launch): the same 16 x 16 image,
    one descriptor per case, resize 1 : 1 (coefficients exactly 1 and 0)."""
    img = _palette()
    pipe = _pipe(mean=(0, 0, 0), std=(1, 1, 1), to_rgb=False)
    names = list(PALETTE_CASES)
    plans = [_plan(img, (16, 16), photo=PALETTE_CASES[n]) for n in names]
    out = pipe([img] * len(names), plans=plans)
    torch.cuda.synchronize()
    return img, pipe, dict(zip(names, out['img'].cpu().numpy()))


@pytest.mark.parametrize('name', list(PALETTE_CASES))
def test_palette(palette_run, name):
    img, pipe, got = palette_run
    photo = PALETTE_CASES[name]
    want = PO.chain(img.astype(np.float32), photo)     # (16, 16, 3), 1 : 1
    np.testing.assert_array_equal(_bits(got[name]),
                                  _bits(want.transpose(2, 0, 1)))
    # and through the whole composition (mean 0, std 1 change no bit but the
    # sign of a zero)
    ref = PO.augment(img, _plan(img, (16, 16), photo=photo), pipe.mean,
                     pipe.std, False, 16, 16)
    np.testing.assert_array_equal(got[name], ref)


def test_palette_reaches_the_edges(palette_run):
    """The properties the palette is there for, read from the oracle (which
    the kernel equals bit for bit in ``test_palette``)."""
    img, _, got = palette_run
    x = img.astype(np.float32)
    assert (x + F(-31.7)).min() < 0
    assert got['brightness_down'].min() < 0            # not clipped
    assert got['contrast_before'].max() > 255
    hsv = PO.bgr2hsv(x)
    assert (hsv[..., 1] * F(1.5)).max() > 1
    h = hsv[..., 0]
    assert (h == 0).any() and (h + F(17.3) > 360).any() and \
        (h + F(-17.9) < 0).any()

    def wrapped(d):
        v = h + F(d)
        v = np.where(v > 360, v - F(360), v)
        return np.where(v < 0, v + F(360), v)
    assert (wrapped(-1e-6) == 360).any()
    assert (wrapped(-120.0) == 0).any()
    assert (wrapped(120.0) == 360).any()
    # ties: every pair of channels equal at the maximum somewhere
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    v = x.max(-1)
    for p, q in ((b, g), (g, r), (b, r)):
        assert ((p == v) & (q == v) & (x.min(-1) < v)).any()
    # the round trip alone is not the identity in fp32
    assert not np.array_equal(got['round_trip_only'], x.transpose(2, 0, 1))
    # the six permutations are six different images
    perms = [got[n] for n in got if n.startswith('perm_')]
    assert len(perms) == 6
    assert len({p.tobytes() for p in perms}) == 6


# 2 ---------------------------------------------------------------------------
@pytest.mark.parametrize('new', [(29, 31), (7, 9), (13, 17)],
                         ids=['up', 'down', 'same'])
def test_float_mode_without_photo(new):
    """to_float32=True alone: no chain, no HSV round trip, the float resize.
    Against the 8-bit launch it differs wherever that one rounds."""
    from ld_amd.pipeline import DevicePipeline
    img = PC.palette_image(13, 17, seed=3)
    pipe = _pipe(pad_size=(32, 32))
    assert pipe.float_mode and pipe.photo is None and pipe.augmented
    plan = _plan(img, new, photo=None)
    got, _ = _check(pipe, [img], [plan])
    old = DevicePipeline(mean=MEAN, std=STD, to_rgb=True, size_divisor=None,
                         flip_ratio=0.0, device=DEV, pad_size=(32, 32))
    assert not old.float_mode
    plan8 = {k: v for k, v in plan.items() if k != 'photo'}
    got8 = old([img], plans=[plan8])['img'].cpu().numpy()
    np.testing.assert_array_equal(
        got8[0], AO.augment(img, plan8, MEAN, STD, True, 32, 32))
    if new == (13, 17):     # 1 : 1: nothing to round, the same bits
        np.testing.assert_array_equal(_bits(got), _bits(got8))
    else:
        assert (got != got8).any()
        # the 8-bit path rounds to a whole level before the normalisation
        lsb = 1.0 / min(STD)
        assert np.abs(got - got8).max() <= lsb


# 3 ---------------------------------------------------------------------------
@pytest.mark.parametrize('to_rgb', [True, False])
def test_geometry_batch_of_three(to_rgb):
    """Expand's float fill under a permuted image, a MinIoURandomCrop window,
    Resize(keep_ratio=False), flip, Pad(size, pad_val); three different
    descriptors in one launch."""
    rs = np.random.RandomState(5)
    imgs = _images(rs, [(21, 30), (40, 60), (33, 27)])
    imgs[2][:] = (40, 90, 200)                     # constant: see the seam
    fill = tuple(float(v) for v in np.asarray(MEAN[::-1], np.float32))
    pad_val = (1.5, -2.0, 0.25)
    pipe = _pipe(to_rgb=to_rgb, pad_size=(48, 64), pad_val=pad_val, photo={})
    ph = [_photo(mode=0, perm=(1, 2, 0), **{k: ALL[k] for k in
                                             ('delta', 'alpha', 'hue')}),
          _photo(mode=1, alpha=0.7, saturation=1.31, perm=(2, 1, 0)),
          _photo(delta=12.25, perm=(0, 2, 1))]
    plans = [
        # the whole canvas down: taps blend image and fill along the seam
        _plan(imgs[0], (45, 64), False, canvas=(52, 75, 31, 45), fill=fill,
              resized=(45, 64), photo=ph[0]),
        # a window across the image's top-left corner, up, flipped
        _plan(imgs[1], (48, 63), True, canvas=(90, 130, 20, 30), fill=fill,
              window=(14, 23, 27, 37), resized=(48, 63), photo=ph[1]),
        # a 4 x 4 window, half fill and half image, 8 x up: every tap pair
        # along the seam has the fill on one side and a pixel on the other
        _plan(imgs[2], (32, 32), False, canvas=(66, 54, 10, 10), fill=fill,
              window=(20, 8, 4, 4), resized=(32, 32), photo=ph[2]),
    ]
    got, out = _check(pipe, imgs, plans)
    assert got.shape == (3, 3, 48, 64)
    norm_pad = np.asarray(pad_val, np.float32)
    for i, p in enumerate(plans):
        oh, ow = p['img_shape'][:2]
        for c in range(3):                 # pad_val outside (out_h, out_w)
            assert (got[i, c, oh:, :] == norm_pad[c]).all()
            assert (got[i, c, :, ow:] == norm_pad[c]).all()
        assert out['img_metas'][i]['pad_shape'] == (48, 64, 3)
    # image 2: left of the seam the undistorted fill, right of it the
    # distorted constant pixel, between them strictly between
    px = PO.chain(imgs[2][:1, :1].astype(np.float32), ph[2])
    lo = PO.normalize(np.asarray(fill, np.float32)[None, None], MEAN, STD,
                      to_rgb)[0, 0]
    hi = PO.normalize(px, MEAN, STD, to_rgb)[0, 0]
    row = got[2, :, 16, :32]                        # (3, 32)
    for c in range(3):
        assert row[c, 0] == lo[c] and row[c, 31] == hi[c]
        a, b = min(lo[c], hi[c]), max(lo[c], hi[c])
        mid = row[c, 12:20]
        assert ((mid > a) & (mid < b)).any()
    # the fill is not permuted and not distorted: a pixel deep in the canvas
    # (four equal taps with 0 < f < 1: fill * (1 - f) + fill * f rounds three
    # times per pass, so within a few ulp of the fill, 124 * 2^-22 < 3e-5,
    # before the division by std >= 57)
    deep = got[0, :, 0, 0]
    np.testing.assert_allclose(deep, lo, rtol=0, atol=3e-5 / min(STD))


# 4 ---------------------------------------------------------------------------
def test_two_runs_are_bit_identical():
    rs = np.random.RandomState(8)
    imgs = _images(rs, [(37, 53), (40, 60)])
    pipe = _pipe(pad_size=(64, 64), photo={},
                 expand=dict(mean=MEAN, to_rgb=True), min_iou_crop={},
                 img_scale=(64, 64), keep_ratio=False, flip_ratio=0.5)
    boxes = [np.array([[3, 4, 30, 30]], np.float32),
             np.array([[5, 5, 40, 36]], np.float32)]
    labels = [np.array([1]), np.array([2])]
    plans = pipe.plan([im.shape[:2] for im in imgs],
                      np.random.RandomState(3), boxes, labels)
    a = pipe(imgs, boxes, labels, plans=plans)['img']
    b = pipe(imgs, boxes, labels, plans=plans)['img']
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    _check(pipe, imgs, plans)


# 5 ---------------------------------------------------------------------------
SSD300 = [
    dict(type='LoadImageFromFile', to_float32=True),
    dict(type='LoadAnnotations', with_bbox=True),
    PC.PMD,
    dict(type='Expand', mean=PC.SSD_NORM['mean'],
         to_rgb=PC.SSD_NORM['to_rgb'], ratio_range=(1, 4)),
    dict(type='MinIoURandomCrop', min_ious=(0.1, 0.3, 0.5, 0.7, 0.9),
         min_crop_size=0.3),
    dict(type='Resize', img_scale=(300, 300), keep_ratio=False),
    dict(type='Normalize', **PC.SSD_NORM),
    dict(type='RandomFlip', flip_ratio=0.5),
    dict(type='DefaultFormatBundle'),
    dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels']),
]


def test_loader_with_the_ssd300_pipeline(tmp_path):
    """build_dataloader needs nothing beyond what from_cfg returns: the
    batch is a function of (seed, epoch, index), photometric draws included,
    and its pixels are the oracle's."""
    from ld_amd import dataloader as DL
    from ld_amd import datasets as D
    root = FX.write_fixture(tmp_path)
    kw = dict(FX.dataset_kwargs(root)['voc_train'][1])
    kw['pipeline'] = SSD300
    ds = D.VOCDataset(**kw)
    assert len(ds) <= 8
    ld = DL.build_dataloader(ds, 2, 1, seed=5, device=DEV, num_threads=2)
    assert ld.pipeline.float_mode and ld.pipeline.photo is not None
    h = ld.host_batch(1, 1)
    again = ld.host_batch(1, 1)
    assert repr(h['plans']) == repr(again['plans'])
    assert all(p['photo'] is not None for p in h['plans'])
    a, b = ld.device_batch(h), ld.device_batch(again)
    torch.cuda.synchronize()
    assert tuple(a['img'].shape) == (len(h['indices']), 3, 300, 300)
    assert torch.equal(a['img'].view(torch.int32), b['img'].view(torch.int32))
    for x, y in zip(a['gt_bboxes'], b['gt_bboxes']):
        assert torch.equal(x, y)
    other = ld.host_batch(1, 0)
    assert repr(other['plans']) != repr(h['plans'])
    p = ld.pipeline
    ref = PO.augment(h['images'][0], h['plans'][0], p.mean, p.std, p.to_rgb,
                     300, 300)
    np.testing.assert_array_equal(_bits(a['img'][0].cpu().numpy()),
                                  _bits(ref))
    np.testing.assert_array_equal(a['gt_bboxes'][0].cpu().numpy(),
                                  h['plans'][0]['gt_bboxes'])
    m = a['img_metas'][0]
    assert m['img_shape'] == (300, 300, 3) and m['pad_shape'] == (300, 300, 3)
    ld.close()
