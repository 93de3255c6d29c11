"""CPU checks of the float-image mode's host half (ld_amd.pipeline:
``photometric_draw``, ``plan_image`` with PhotoMetricDistortion in front,
``from_cfg``, the ``ld_image_photo_t`` descriptor) and of the numpy oracle
(tests/_photometric_oracle.py) against what the reference's own classes
returned for the same seeds (tests/golden/photometric.npz,
tools/gen_golden_photometric.py).

Pinned on the reference's classes: the draw order, the order of the chain, the
float32 rounding of the drawn scalars, the hue wraps, the permutation, no
clipping, the float canvas fill and the geometry after the photometric draws.
NOT pinned: cv2's HSV conversions and float resize (the tool stubs them with
the oracle's restatement of the published formulas)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _photometric_cases as PC  # noqa: E402
import _photometric_oracle as PO  # noqa: E402

from ld_amd import pipeline as PL  # noqa: E402

GOLD = np.load(os.path.join(HERE, 'golden', 'photometric.npz'))
CHAIN = [f'pmd_s{s}' for s in GOLD['pmd_seeds']]
FULL = [(k, int(s)) for k in ('ssd', 'yolo') for s in GOLD[k + '_seeds']]
PMD_KW = {k: v for k, v in PC.PMD.items() if k != 'type'}


# ---------------------------------------------------------------------------
# draws and chain against the reference's own class
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', CHAIN)
def test_draw_and_chain_equal_reference(name):
    seed = int(name.split('_s')[1])
    want = PC.photo_of(GOLD, name)
    np.random.seed(seed)  # the module generator, as the reference draws
    photo = PL.photometric_draw(np.random, **PMD_KW)
    assert photo == want            # float64 draws: equal or not, no tolerance
    assert np.random.random_sample() == float(GOLD[name + '_next'])
    again = PL.photometric_draw(np.random.RandomState(seed), **PMD_KW)
    assert again == photo
    img = PC.palette_image().astype(np.float32)
    out = PO.chain(img, photo)
    assert out.dtype == np.float32
    assert out.tobytes() == GOLD[name + '_out'].tobytes()


def test_golden_covers_the_edges():
    photos = [PC.photo_of(GOLD, n) for n in CHAIN]
    assert {p['mode'] for p in photos} == {0, 1}
    for k in ('delta', 'alpha', 'saturation', 'hue', 'perm'):
        assert {p[k] is None for p in photos} == {True, False}, k
    perms = {p['perm'] for p in photos if p['perm'] is not None}
    assert (0, 1, 2) in perms and len(perms) > 1
    img = PC.palette_image().astype(np.float32)
    wraps = [PO.hue_wraps(img, p) for p in photos]
    assert any(w[0] for w in wraps) and any(w[1] for w in wraps)
    # nothing clips: values below 0 and above 255 are in the stored outputs
    outs = np.concatenate([GOLD[n + '_out'].ravel() for n in CHAIN])
    assert outs.min() < 0 and outs.max() > 255
    kinds = {k for k, _ in FULL}
    assert kinds == {'ssd', 'yolo'}
    assert any(tuple(GOLD[f'{k}_s{s}_canvas'][:2]) != (8, 8) for k, s in FULL)
    assert PC.palette_image().shape == (8, 8, 3)


# ---------------------------------------------------------------------------
# the full pipelines: the photometric draws come first and shift the others
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind,seed', FULL,
                         ids=[f'{k}_s{s}' for k, s in FULL])
def test_plan_and_pixels_equal_reference(kind, seed):
    name = f'{kind}_s{seed}'
    g = {k[len(name) + 1:]: GOLD[k] for k in GOLD.files
         if k.startswith(name + '_')}
    pipe = PL.DevicePipeline.from_cfg(PC.LOAD + PC.FULL[kind] + PC.BUNDLE,
                                      device='cpu')
    assert pipe.augmented and pipe.float_mode and pipe.photo is not None
    img = PC.palette_image()
    np.random.seed(seed)
    plan = pipe.plan([img.shape[:2]], gt_bboxes=[PC.BOXES],
                     gt_labels=[PC.LABELS], gt_bboxes_ignore=[PC.IGNORE])[0]
    assert np.random.random_sample() == float(g['next'])
    assert not plan['rejected']
    assert plan['photo'] == PC.photo_of(GOLD, name)
    for k in ('canvas', 'window', 'resized', 'img_shape'):
        np.testing.assert_array_equal(np.asarray(plan[k]), g[k], err_msg=k)
    assert plan['flip'] == bool(g['flip'])
    assert plan['mode'] == float(g['mode_iou'])
    np.testing.assert_array_equal(plan['scale_factor'], g['scale_factor'])
    assert plan['scale_factor'].dtype == g['scale_factor'].dtype
    for k in ('gt_bboxes', 'gt_labels'):
        np.testing.assert_array_equal(plan[k], g[k], err_msg=k)
        assert plan[k].dtype == g[k].dtype and plan[k].shape == g[k].shape
    # Expand's canvas value is the float mean in BGR order
    norm = PC.SSD_NORM if kind == 'ssd' else PC.YOLO_NORM
    assert plan['fill'] == tuple(
        float(v) for v in np.asarray(norm['mean'][::-1], np.float32))
    # the pixels: the oracle composition is what the reference's classes
    # (over the stubbed conversions and resize) produced
    ph, pw = pipe.batch_shape([plan])
    assert (ph, pw, 3) == tuple(g['pad_shape'])
    out = PO.augment(img, plan, pipe.mean, pipe.std, pipe.to_rgb, ph, pw,
                     pipe.pad_val)
    assert out.transpose(1, 2, 0).tobytes() == g['out'].tobytes()


# ---------------------------------------------------------------------------
# from_cfg
# ---------------------------------------------------------------------------
STOCK = list(zip(GOLD['stock_names'].tolist(),
                 GOLD['stock_pipelines'].tolist()))


@pytest.mark.parametrize('name,text', STOCK, ids=[n for n, _ in STOCK])
def test_from_cfg_builds_every_stock_pipeline(name, text):
    steps = PC.from_json(json.loads(text))
    assert steps[0] == dict(type='LoadImageFromFile', to_float32=True)
    pipe = PL.DevicePipeline.from_cfg(steps, device='cpu')
    assert pipe.float_mode and pipe.augmented
    pmd = [s for s in steps if s['type'] == 'PhotoMetricDistortion'][0]
    for k, v in pmd.items():
        if k != 'type':
            assert pipe.photo[k] == v
    assert pipe.photo['brightness_delta'] == 32 and \
        pipe.photo['hue_delta'] == 18      # the reference's defaults
    assert pipe.expand is not None and pipe.min_iou_crop is not None
    assert all(isinstance(v, float) for v in pipe.expand_fill)
    rs = np.random.RandomState(4)
    boxes = np.array([[30, 40, 200, 180], [100, 20, 310, 230]], np.float32)
    plan = pipe.plan_image((240, 320), rs, boxes, np.array([1, 2]))
    assert not plan['rejected'] and set(plan['photo']) == {
        'delta', 'mode', 'alpha', 'saturation', 'hue', 'perm'}
    resize = [s for s in steps if s['type'] == 'Resize'][0]
    if not resize['keep_ratio']:
        assert plan['img_shape'][:2] == tuple(resize['img_scale'])[::-1]
    if 'yolact' in name:  # FilterAnnotations: small boxes leave first
        assert pipe.min_gt_bbox_wh == (4.0, 4.0)
        tiny = np.array([[5, 5, 9, 30], [30, 40, 200, 180]], np.float32)
        p = pipe.plan_image((240, 320), np.random.RandomState(4), tiny,
                            np.array([1, 2]))
        assert 0 not in p['keep']
        rs = np.random.RandomState(4)
        none = pipe.plan_image((240, 320), rs, tiny[:1], np.array([1]))
        assert none['rejected']       # and no draw was made for it
        assert rs.random_sample() == np.random.RandomState(4).random_sample()


def test_to_float32_alone_selects_float_mode():
    steps = [dict(type='LoadImageFromFile', to_float32=True),
             dict(type='Resize', img_scale=(64, 48), keep_ratio=True),
             dict(type='Pad', size_divisor=32)]
    p = PL.DevicePipeline.from_cfg(steps, device='cpu')
    assert p.float_mode and p.augmented and p.photo is None
    rs = np.random.RandomState(0)
    plan = p.plan_image((30, 40), rs)
    assert plan['photo'] is None
    # no photometric draw was made: the draws are the 8-bit pipeline's
    q = PL.DevicePipeline.from_cfg(steps[1:], device='cpu')
    assert not q.float_mode and not q.augmented
    rq = np.random.RandomState(0)
    plain = q.plan([(30, 40)], rq)[0]
    assert (plan['flip'], plan['img_shape']) == (plain['flip'],
                                                 plain['img_shape'])
    assert rs.random_sample() == rq.random_sample()


@pytest.mark.parametrize('steps', [
    # no to_float32: the reference itself fails its float32 assertion
    [dict(type='LoadImageFromFile'), dict(type='PhotoMetricDistortion')],
    [dict(type='LoadImageFromFile', to_float32=False),
     dict(type='PhotoMetricDistortion')],
    [dict(type='PhotoMetricDistortion')],
    # after a geometry step
    [PC.LOAD[0], dict(type='Expand'), dict(type='PhotoMetricDistortion')],
    [PC.LOAD[0], dict(type='MinIoURandomCrop'),
     dict(type='PhotoMetricDistortion')],
    [PC.LOAD[0], dict(type='Resize', img_scale=(64, 64)),
     dict(type='PhotoMetricDistortion')],
    [PC.LOAD[0], dict(type='Resize', img_scale=(64, 64)),
     dict(type='RandomFlip', flip_ratio=0.5),
     dict(type='PhotoMetricDistortion')],
    # the loading step after it, and twice
    [dict(type='PhotoMetricDistortion'), PC.LOAD[0]],
    [PC.LOAD[0], dict(type='PhotoMetricDistortion'),
     dict(type='PhotoMetricDistortion')],
])
def test_photometric_distortion_refused_elsewhere(steps):
    with pytest.raises(NotImplementedError,
                       match='^pipeline step PhotoMetricDistortion$'):
        PL.DevicePipeline.from_cfg(steps, device='cpu')


def test_other_steps_stay_refused():
    for t in ('CutOut', 'RandomCenterCropPad', 'AutoAugment', 'Albu',
              'Corrupt'):
        with pytest.raises(NotImplementedError, match=f'^pipeline step {t}$'):
            PL.DevicePipeline.from_cfg([PC.LOAD[0], dict(type=t)],
                                       device='cpu')
    with pytest.raises(NotImplementedError,
                       match='^pipeline step FilterAnnotations$'):
        PL.DevicePipeline.from_cfg(
            [PC.LOAD[0], dict(type='PhotoMetricDistortion'),
             dict(type='FilterAnnotations', min_gt_bbox_wh=(4, 4))],
            device='cpu')


def test_photo_needs_to_float32():
    with pytest.raises(ValueError, match='to_float32=True'):
        PL.DevicePipeline(photo={}, device='cpu')
    with pytest.raises(ValueError, match='hue_delta'):
        PL.DevicePipeline(photo=dict(hue_delta=400), to_float32=True,
                          device='cpu')
    p = PL.DevicePipeline(photo={}, to_float32=True, device='cpu')
    assert p.photo == dict(brightness_delta=32, contrast_range=(0.5, 1.5),
                           saturation_range=(0.5, 1.5), hue_delta=18)
    # the 8-bit mode keeps the uint8 cast of the fill
    e = dict(mean=(123.675, 116.28, 103.53), to_rgb=True)
    assert PL.DevicePipeline(expand=e, device='cpu').expand_fill == \
        (103, 116, 123)
    f = PL.DevicePipeline(expand=e, to_float32=True, device='cpu')
    assert f.expand_fill == tuple(
        float(np.float32(v)) for v in (103.53, 116.28, 123.675))


# ---------------------------------------------------------------------------
# the descriptor
# ---------------------------------------------------------------------------
def test_photo_descriptor_layout_and_fill():
    """The ctypes mirror of ld_image_photo_t (LP64: one pointer, 17 int32,
    7 floats, 10 int32) and what a plan writes into it; the two older
    descriptors keep their layout."""
    from ld_amd import lib as L
    assert C.sizeof(L.ImagePhotoT) == 8 + 17 * 4 + 7 * 4 + 10 * 4 == 144
    assert L.ImagePhotoT.fill.offset == 76 and L.ImagePhotoT.delta.offset == 88
    assert L.ImagePhotoT.do_brightness.offset == 104
    assert L.ImagePhotoT.perm.offset == 128
    assert C.sizeof(L.ImageAugT) == 80 and C.sizeof(L.ImageT) == 32
    for f, _ in L.ImageAugT._fields_[:-1]:   # the shared geometry prefix
        assert getattr(L.ImagePhotoT, f).offset == getattr(L.ImageAugT,
                                                           f).offset
    name = 'ssd_s%d' % GOLD['ssd_seeds'][0]
    pipe = PL.DevicePipeline.from_cfg(PC.LOAD + PC.SSD, device='cpu')
    seed = int(GOLD['ssd_seeds'][0])
    plan = pipe.plan_image((8, 8), np.random.RandomState(seed), PC.BOXES,
                           PC.LABELS, PC.IGNORE)
    d = L.ImagePhotoT()
    pipe.fill_photo_descriptor(d, plan, (8, 8))
    assert (d.canvas_h, d.canvas_w, d.img_top, d.img_left) == plan['canvas']
    assert (d.win_y, d.win_x, d.win_h, d.win_w) == plan['window']
    assert (d.new_h, d.new_w, d.out_h, d.out_w) == (12, 12, 12, 12)
    assert tuple(d.fill) == plan['fill']
    ph = PC.photo_of(GOLD, name)
    for field, key, flag in (('delta', 'delta', 'do_brightness'),
                             ('alpha', 'alpha', 'do_contrast'),
                             ('saturation', 'saturation', 'do_saturation'),
                             ('hue', 'hue', 'do_hue')):
        assert getattr(d, flag) == int(ph[key] is not None)
        if ph[key] is not None:   # rounded to float32, once
            assert getattr(d, field) == float(np.float32(ph[key]))
    assert d.contrast_mode == ph['mode'] and d.do_hsv == 1
    assert tuple(d.perm) == (ph['perm'] or (0, 1, 2))
    # float mode without the distortion: the identity chain, no round trip
    e = L.ImagePhotoT()
    PL.DevicePipeline.fill_photo_descriptor(
        e, dict(img_shape=(50, 70, 3), flip=False, photo=None), (40, 60))
    assert (e.do_brightness, e.do_contrast, e.do_saturation, e.do_hue,
            e.do_hsv) == (0, 0, 0, 0, 0)
    assert tuple(e.perm) == (0, 1, 2) and tuple(e.fill) == (0.0, 0.0, 0.0)
    assert (e.win_h, e.win_w, e.new_h, e.new_w) == (40, 60, 50, 70)
    with pytest.raises(ValueError, match='permutation'):
        PL.DevicePipeline.fill_photo_descriptor(
            e, dict(img_shape=(5, 7, 3), flip=False,
                    photo=dict(ph, perm=(0, 0, 2))), (4, 6))


# ---------------------------------------------------------------------------
# oracle sanity
# ---------------------------------------------------------------------------
OUT_OF_GAMUT = np.array(
    [[-20, 5, 300], [-31.5, -2, -0.25], [260, 270, 255.5], [-5, -3, 0],
     [382.5, 0, -16], [0, -1, 0], [300, 300, -10], [-10, 5, 5]], np.float32)


def test_oracle_round_trip_against_float64():
    """hsv2bgr(bgr2hsv(x)) in float32 against the same formulas evaluated in
    float64, on the 17^3 lattice over [0, 255]^3 plus pixels below 0 and
    above 255.  Measured worst absolute difference: 7.52e-05 (at B, G, R =
    223.125, 31.875, 255; 5.46e-05 on the out-of-gamut pixels).  The bar is
    twice that.  It only guards the oracle against a slip in the restatement;
    it says nothing about cv2."""
    g = np.linspace(0, 255, 17).astype(np.float32)
    lat = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    x = np.concatenate([lat, OUT_OF_GAMUT])
    hsv = PO.bgr2hsv(x)
    assert hsv.dtype == np.float32
    assert (hsv[:len(lat), 0] >= 0).all() and (hsv[:len(lat), 0] <= 360).all()
    assert (hsv[:len(lat), 1] >= 0).all() and (hsv[:len(lat), 1] <= 1).all()
    assert (hsv[len(lat):, 1] > 1).any()          # S > 1 flows through
    got = PO.hsv2bgr(hsv)
    err = np.abs(got.astype(np.float64) - PO.roundtrip_f64(x)).max()
    print('worst |fp32 - fp64| of the round trip:', err)
    assert err <= 2 * 7.52e-05
    # greys come back exactly (the S == 0 shortcut)
    grey = np.repeat(g[:, None], 3, 1)
    assert np.array_equal(PO.hsv2bgr(PO.bgr2hsv(grey)), grey)
    # the primaries land on the documented hues
    prim = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.float32)
    np.testing.assert_array_equal(PO.bgr2hsv(prim)[:, 0], [240, 120, 0])


def test_oracle_float_resize_differs_from_the_8bit_one():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
    import pipeline_oracle as P8
    img = PC.palette_image(13, 17, seed=3)
    f = PO.resize_linear_f32(img.astype(np.float32), 20, 11)
    u = P8.resize_linear_u8(img, 20, 11).astype(np.float32)
    assert f.shape == u.shape == (20, 11, 3)
    assert np.abs(f - u).max() <= 1.0 and (f != u).any()
    # 1 : 1 copies the pixels
    same = PO.resize_linear_f32(img.astype(np.float32), 13, 17)
    assert np.array_equal(same, img.astype(np.float32))
