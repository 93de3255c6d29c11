"""CPU checks of the train-time augmentations' host half (ld_amd.pipeline:
Expand, MinIoURandomCrop, Resize(keep_ratio=False), RandomCrop, Pad(size)):
every plan against what the reference's own classes returned for the same
seed (tests/golden/augment.npz, tools/gen_golden_augment.py), the config
reader, and the loader's replacement of a rejected image."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _augment_cases as AC  # noqa: E402
import _dataset_fixture as FX  # noqa: E402

from ld_amd import dataloader as DL  # noqa: E402
from ld_amd import datasets as D  # noqa: E402
from ld_amd import pipeline as PL  # noqa: E402

GOLD = np.load(os.path.join(HERE, 'golden', 'augment.npz'))
LOAD = [dict(type='LoadImageFromFile'),
        dict(type='LoadAnnotations', with_bbox=True)]
BUNDLE = [dict(type='DefaultFormatBundle'),
          dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]


# ---------------------------------------------------------------------------
# plans against the reference's own transforms
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', AC.CASES, ids=[c[0] for c in AC.CASES])
def test_plan_equals_reference(case):
    name, seed, shape, boxes, labels, ignore, steps = case
    g = {k[len(name) + 1:]: GOLD[k] for k in GOLD.files
         if k.startswith(name + '_')}
    pipe = PL.DevicePipeline.from_cfg(LOAD + steps + BUNDLE, device='cpu')
    assert pipe.augmented
    np.random.seed(seed)  # the module generator, as the reference draws
    plan = pipe.plan([shape], gt_bboxes=[boxes], gt_labels=[labels],
                     gt_bboxes_ignore=[ignore])[0]
    # the number of draws: the next one is the reference's next one
    assert np.random.random_sample() == float(g['next'])
    assert plan['rejected'] == bool(g['rejected'])
    if plan['rejected']:
        return
    for k in ('canvas', 'window', 'resized', 'crop', 'img_shape'):
        np.testing.assert_array_equal(np.asarray(plan[k]), g[k], err_msg=k)
    assert plan['flip'] == bool(g['flip'])
    if any(s['type'] == 'MinIoURandomCrop' for s in steps):
        assert plan['mode'] == float(g['mode'])
    np.testing.assert_array_equal(plan['scale_factor'], g['scale_factor'])
    assert plan['scale_factor'].dtype == g['scale_factor'].dtype
    for k in ('gt_bboxes', 'gt_labels', 'gt_bboxes_ignore'):
        np.testing.assert_array_equal(plan[k], g[k], err_msg=k)
        assert plan[k].dtype == g[k].dtype and plan[k].shape == g[k].shape
    # which input rows survived
    np.testing.assert_array_equal(labels[plan['keep']], g['gt_labels'])
    assert len(plan['keep_ignore']) == len(g['gt_labels_ignore'])
    # the same plan from a generator object as from the module
    again = pipe.plan([shape], np.random.RandomState(seed), [boxes], [labels],
                      [ignore])[0]
    assert repr(again) == repr(plan)


def test_golden_covers_the_edges():
    """What the issue asks the seeds to include, read from the stored
    reference outputs."""
    rej = {c[0] for c in AC.CASES if bool(GOLD[c[0] + '_rejected'])}
    assert {'jitter_rejected', 'jitter_no_boxes_rejected'} <= rej
    assert len(GOLD['jitter_negative_empty_gt_bboxes']) == 0
    assert tuple(GOLD['jitter_small_image_img_shape'][:2]) < (64, 64)
    modes = {float(GOLD[c[0] + '_mode']) for c in AC.CASES}
    assert modes >= {1.0, 0.1, 0.3, 0.5, 0.7, 0.9, 0.0}
    assert tuple(GOLD['zoom_s10_canvas']) == (100, 130, 0, 0)  # prob skipped
    assert tuple(GOLD['zoom_s9_canvas'][:2]) != (100, 130)
    assert len(GOLD['zoom_s9_gt_bboxes_ignore']) == 1
    # the centre on the patch border is out
    c = [c for c in AC.CASES if c[0] == 'miniou_center_on_border'][0]
    x1 = GOLD['miniou_center_on_border_window'][1]
    assert (c[3][1, 0] + c[3][1, 2]) / 2 == x1
    assert len(GOLD['miniou_center_on_border_gt_bboxes']) == 1


def test_pad_shape_and_metas_of_a_plan():
    """img_metas of a fixed pad are the reference's: checked on the host half
    (``__call__`` needs a device) through the pad-size rule."""
    for case in AC.CASES:
        name, steps = case[0], case[6]
        pads = [s for s in steps if s['type'] == 'Pad']
        if not pads or bool(GOLD[name + '_rejected']):
            continue
        pipe = PL.DevicePipeline.from_cfg(steps, device='cpu')
        h, w = GOLD[name + '_img_shape'][:2]
        if pipe.pad_size is not None:
            want = tuple(pipe.pad_size) + (3,)
        else:
            d = pipe.size_divisor
            want = (-(-h // d) * d, -(-w // d) * d, 3)
        assert want == tuple(GOLD[name + '_pad_shape']), name


# ---------------------------------------------------------------------------
# from_cfg
# ---------------------------------------------------------------------------
def test_from_cfg_nas_fpn_style():
    steps = [
        dict(type='Resize', img_scale=(640, 640), ratio_range=(0.8, 1.2),
             keep_ratio=True),
        dict(type='RandomCrop', crop_size=(640, 640)),
        dict(type='RandomFlip', flip_ratio=0.5),
        AC.NORM,
        dict(type='Pad', size=(640, 640)),
    ]
    p = PL.DevicePipeline.from_cfg(LOAD + steps + BUNDLE, device='cpu')
    assert p.augmented and p.pad_size == (640, 640) and p.size_divisor is None
    assert p.crop['crop_size'] == (640, 640)
    assert p.crop['crop_type'] == 'absolute'
    assert not p.crop['allow_negative_crop'] and p.crop['bbox_clip_border']
    assert p.ratio_range == (0.8, 1.2) and p.keep_ratio
    assert not p.pad_val.any()
    # one shape per run: whatever the draw, the crop never exceeds the pad
    rs = np.random.RandomState(0)
    box = [np.array([[0, 0, 640, 480]], np.float32)]
    for _ in range(20):
        plan = p.plan([(480, 640)], rs, box, [np.array([1])])[0]
        assert plan['img_shape'][0] <= 640 and plan['img_shape'][1] <= 640


def test_from_cfg_expand_min_iou_style():
    steps = AC.zoom(expand={}, min_iou={})
    p = PL.DevicePipeline.from_cfg(LOAD + steps + BUNDLE, device='cpu')
    assert p.augmented and not p.keep_ratio
    assert p.expand['ratio_range'] == (1, 4) and p.expand['prob'] == 0.5
    # the mean is given in RGB order, the canvas is BGR, np.full truncates
    assert p.expand_fill == (103, 116, 123)
    assert p.min_iou_crop['min_crop_size'] == 0.3
    bgr = PL.DevicePipeline.from_cfg(
        AC.zoom(expand=dict(to_rgb=False)), device='cpu')
    assert bgr.expand_fill == (123, 116, 103)
    # keep_ratio=False: independent scales, mmcv.imresize
    plan = p.plan_image((50, 200), np.random.RandomState(2))
    wh, ww = plan['window'][2:]
    np.testing.assert_array_equal(
        plan['scale_factor'],
        np.array([64 / ww, 64 / wh, 64 / ww, 64 / wh], np.float32))
    assert plan['img_shape'] == (64, 64, 3)


def test_plain_pipeline_is_untouched():
    """Without the new steps the plan and the launch are the old ones."""
    p = PL.DevicePipeline.from_cfg(
        [dict(type='Resize', img_scale=(1333, 800), keep_ratio=True),
         dict(type='RandomFlip', flip_ratio=0.5), AC.NORM,
         dict(type='Pad', size_divisor=32)], device='cpu')
    assert not p.augmented
    plan = p.plan([(480, 640)], np.random.RandomState(0))[0]
    assert sorted(plan) == ['flip', 'img_shape', 'ori_shape', 'scale',
                            'scale_factor']


@pytest.mark.parametrize('order,first,second', [
    (['RandomCrop', 'Resize'], 'Resize', 'RandomCrop'),
    (['Resize', 'Expand'], 'Expand', 'Resize'),
    (['MinIoURandomCrop', 'Expand', 'Resize'], 'Expand', 'MinIoURandomCrop'),
    (['Resize', 'MinIoURandomCrop'], 'MinIoURandomCrop', 'Resize'),
    (['Resize', 'RandomFlip', 'RandomCrop'], 'RandomCrop', 'RandomFlip'),
    (['Resize', 'Pad', 'Normalize'], 'Normalize', 'Pad'),
    (['Resize', 'Pad', 'RandomCrop'], 'RandomCrop', 'Pad'),
])
def test_from_cfg_refuses_other_orders(order, first, second):
    args = dict(
        Expand=dict(), MinIoURandomCrop=dict(),
        Resize=dict(img_scale=(64, 64)), RandomCrop=dict(crop_size=(32, 32)),
        RandomFlip=dict(flip_ratio=0.5),
        Normalize={k: v for k, v in AC.NORM.items() if k != 'type'},
        Pad=dict(size=(64, 64)))
    steps = [dict(type=t, **args[t]) for t in order]
    with pytest.raises(NotImplementedError) as e:
        PL.DevicePipeline.from_cfg(steps, device='cpu')
    # both steps are named, the late one first
    assert f'pipeline step {first} after {second}' in str(e.value)


def test_normalize_and_flip_in_either_order():
    for pair in ([PL_FLIP, AC.NORM], [AC.NORM, PL_FLIP]):
        p = PL.DevicePipeline.from_cfg(
            [dict(type='Resize', img_scale=(64, 64)),
             dict(type='RandomCrop', crop_size=(32, 32)), *pair,
             dict(type='Pad', size=(32, 32))], device='cpu')
        assert p.flip_ratio == 0.5 and p.to_rgb


PL_FLIP = AC.FLIP


def test_pad_size_too_small_and_both_pads():
    with pytest.raises(ValueError, match='size_divisor'):
        PL.DevicePipeline.from_cfg(
            [dict(type='Resize', img_scale=(64, 64)),
             dict(type='Pad', size=(64, 64), size_divisor=32)], device='cpu')
    with pytest.raises(ValueError, match='size_divisor'):
        PL.DevicePipeline(pad_size=(64, 64), size_divisor=32, device='cpu')
    # an image larger than the pad: mmcv asserts, both sizes are named
    p = PL.DevicePipeline(img_scale=(96, 64), pad_size=(40, 48),
                          size_divisor=None, flip_ratio=0.0, device='cpu')
    plans = p.plan([(64, 96)], np.random.RandomState(0))
    with pytest.raises(ValueError) as e:
        p.batch_shape(plans)
    assert '(40, 48)' in str(e.value) and '(64, 96)' in str(e.value)
    p.img_scale = (48, 32)
    plans = p.plan([(64, 96)], np.random.RandomState(0))
    assert plans[0]['img_shape'] == (32, 48, 3)
    assert p.batch_shape(plans) == (40, 48)


def test_descriptor_layout_and_fill():
    """The ctypes mirror of ld_image_aug_t (LP64: one pointer, 17 int32, 4
    bytes of fill) and what a plan writes into it."""
    import ctypes as C
    from ld_amd import lib as L
    assert C.sizeof(L.ImageAugT) == 8 + 17 * 4 + 4 == 80
    assert L.ImageAugT.canvas_h.offset == 16 and L.ImageAugT.fill.offset == 76
    case = [c for c in AC.CASES if c[0] == 'all_steps'][0]
    pipe = PL.DevicePipeline.from_cfg(case[6], device='cpu')
    plan = pipe.plan_image(case[2], np.random.RandomState(case[1]), case[3],
                           case[4], case[5])
    d = L.ImageAugT()
    pipe.fill_descriptor(d, plan, case[2])
    assert (d.canvas_h, d.canvas_w, d.img_top, d.img_left) == plan['canvas']
    assert (d.win_y, d.win_x, d.win_h, d.win_w) == plan['window']
    assert (d.new_h, d.new_w) == plan['resized'] == (64, 64)
    assert (d.crop_y, d.crop_x) == plan['crop']
    assert (d.out_h, d.out_w) == plan['img_shape'][:2] == (48, 40)
    assert tuple(d.fill)[:3] == (103, 116, 123)
    # the crop lies inside the resized image, the window inside the canvas
    assert d.crop_y + d.out_h <= d.new_h and d.crop_x + d.out_w <= d.new_w
    assert d.win_y + d.win_h <= d.canvas_h and d.win_x + d.win_w <= d.canvas_w
    # a plain plan gives the identity descriptor
    e = L.ImageAugT()
    PL.DevicePipeline.fill_descriptor(
        e, dict(img_shape=(50, 70, 3), flip=False), (40, 60))
    assert (e.canvas_h, e.canvas_w, e.img_top, e.img_left) == (40, 60, 0, 0)
    assert (e.win_y, e.win_x, e.win_h, e.win_w) == (0, 0, 40, 60)
    assert (e.new_h, e.new_w, e.crop_y, e.crop_x, e.out_h, e.out_w) == \
        (50, 70, 0, 0, 50, 70)


def test_photometric_distortion_still_refused():
    with pytest.raises(NotImplementedError,
                       match='^pipeline step PhotoMetricDistortion$'):
        PL.DevicePipeline.from_cfg(
            [dict(type='PhotoMetricDistortion'),
             *AC.zoom(expand={}, min_iou={})], device='cpu')
    for t in ('CutOut', 'RandomCenterCropPad', 'AutoAugment', 'Albu',
              'Corrupt'):
        with pytest.raises(NotImplementedError, match=f'^pipeline step {t}$'):
            PL.DevicePipeline.from_cfg([dict(type=t)], device='cpu')


# ---------------------------------------------------------------------------
# the loader's replacement rule
# ---------------------------------------------------------------------------
# the crop is small against the resized images (about 2.5 x the 130 x 100
# sources), so that some crops of the thin and corner boxes of the tree miss
# every gt box: seed 11 rejects in epochs 0, 1 and 2
JITTER = LOAD + [
    dict(type='Resize', img_scale=(320, 320), ratio_range=(0.8, 1.2),
         keep_ratio=True),
    dict(type='RandomCrop', crop_size=(24, 24)),
    AC.FLIP, AC.NORM,
    dict(type='Pad', size=(24, 24)),
] + BUNDLE


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    root = FX.write_fixture(tmp_path_factory.mktemp('fixture'))
    kw = dict(FX.dataset_kwargs(root)['voc_train'][1])
    kw['pipeline'] = JITTER
    return D.VOCDataset(**kw)


def test_loader_replaces_a_rejected_image_from_its_group(dataset):
    ld = DL.build_dataloader(dataset, 2, 1, seed=11, num_threads=2)
    rejected = []
    plan_image = ld.pipeline.plan_image

    def spy(*a, **k):
        p = plan_image(*a, **k)
        rejected.append(p['rejected'])
        return p

    ld.pipeline.plan_image = spy
    flag = np.asarray(dataset.flag)
    replaced = n_rejected = 0
    for epoch in range(4):
        order = ld.epoch_order(epoch)
        for index in range(len(ld)):
            del rejected[:]
            h = ld.host_batch(epoch, index, order)
            want = ld.batch_indices(order, index)
            assert len(h['indices']) == len(want) == len(h['plans'])
            n_rej = sum(rejected)
            n_rejected += n_rej
            assert len(rejected) == len(want) + n_rej
            for k, (got, w) in enumerate(zip(h['indices'], want)):
                # a replacement comes from the rejected image's own group
                assert flag[got] == flag[w]
                replaced += got != w
                p = h['plans'][k]
                assert not p['rejected']
                assert tuple(h['images'][k].shape) == p['ori_shape']
                assert h['filenames'][k] == dataset.img_names(got)
                ann = dataset.get_ann_info(got)
                np.testing.assert_array_equal(h['gt_bboxes'][k], ann['bboxes'])
                # what survives is a non-empty selection of that image's rows
                assert len(p['keep']) >= 1
                np.testing.assert_array_equal(p['gt_labels'],
                                              ann['labels'][p['keep']])
                assert p['img_shape'] == (24, 24, 3)
            if n_rej == 0:
                assert h['indices'] == list(want)
    ld.close()
    # the seeded tree exercises the rule (a replacement may draw the rejected
    # index itself again, so fewer indices change than plans are rejected)
    assert n_rejected >= replaced >= 3


def test_loader_batch_is_a_function_of_seed_epoch_index(dataset):
    a = DL.build_dataloader(dataset, 2, 1, seed=11, num_threads=1)
    b = DL.build_dataloader(dataset, 2, 4, seed=11, num_threads=8)
    for epoch, index in ((0, 0), (1, 2), (3, 1), (1, 2)):
        x, y = a.host_batch(epoch, index), b.host_batch(epoch, index)
        assert x['indices'] == y['indices']
        assert x['filenames'] == y['filenames']
        assert repr(x['plans']) == repr(y['plans'])
        for p, q in zip(x['images'], y['images']):
            np.testing.assert_array_equal(p, q)
    # in sequence, through the look-ahead queue, as on its own
    seq = list(b.host_batches(1))
    assert repr(seq[2]['plans']) == repr(a.host_batch(1, 2)['plans'])
    assert seq[2]['indices'] == a.host_batch(1, 2)['indices']
    other = DL.build_dataloader(dataset, 2, 1, seed=12, num_threads=1)
    assert any(repr(other.host_batch(0, i)['plans']) !=
               repr(a.host_batch(0, i)['plans']) for i in range(len(a)))
    for ld in (a, b, other):
        ld.close()


def test_virtual_rank_loader_replaces_too(dataset):
    vr = DL.build_dataloader(dataset, 1, 1, seed=11, virtual_ranks=2,
                             num_threads=2)
    flag = np.asarray(dataset.flag)
    for index in range(len(vr)):
        hosts = vr.host_batch(0, index)
        again = vr.host_batch(0, index)
        for r, (h, g) in enumerate(zip(hosts, again)):
            want = vr.ranks[r].batch_indices(vr.ranks[r].epoch_order(0), index)
            assert [flag[i] for i in h['indices']] == [flag[i] for i in want]
            assert h['indices'] == g['indices']
            assert repr(h['plans']) == repr(g['plans'])
            assert not any(p['rejected'] for p in h['plans'])
    vr.close()
