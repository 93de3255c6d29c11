"""CPU checks of the loader's host half (ld_amd.dataloader): order, decode and
plans are a pure function of (seed, epoch, index) whatever the thread count;
decode gives 3-channel BGR with EXIF orientation applied."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dataset_fixture as FX  # noqa: E402

from ld_amd import dataloader as DL  # noqa: E402
from ld_amd import datasets as D  # noqa: E402

IMG_SCALE = (160, 128)
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375],
            to_rgb=True)
TRAIN_PIPELINE = [
    dict(type='LoadImageFromFile'),
    dict(type='LoadAnnotations', with_bbox=True),
    dict(type='Resize', img_scale=[(160, 96), (160, 128)],
         multiscale_mode='range', keep_ratio=True),
    dict(type='RandomFlip', flip_ratio=0.5),
    dict(type='Normalize', **NORM),
    dict(type='Pad', size_divisor=32),
    dict(type='DefaultFormatBundle'),
    dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels']),
]


def make_test_pipeline(flip=False):
    return [
        dict(type='LoadImageFromFile'),
        dict(type='MultiScaleFlipAug', img_scale=IMG_SCALE, flip=flip,
             transforms=[
                 dict(type='Resize', keep_ratio=True),
                 dict(type='RandomFlip'),
                 dict(type='Normalize', **NORM),
                 dict(type='Pad', size_divisor=32),
                 dict(type='ImageToTensor', keys=['img']),
                 dict(type='Collect', keys=['img'])])]


@pytest.fixture(scope='module')
def root(tmp_path_factory):
    return FX.write_fixture(tmp_path_factory.mktemp('fixture'))


def voc(root, train=True, flip=False):
    kw = dict(FX.dataset_kwargs(root)['voc_train' if train else 'voc_test'][1])
    kw['pipeline'] = TRAIN_PIPELINE if train else make_test_pipeline(flip)
    return D.VOCDataset(**kw)


def _epoch(loader, epoch):
    return list(loader.host_batches(epoch))


def _same_hosts(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x['indices'] == y['indices']
        assert x['filenames'] == y['filenames']
        assert len(x['images']) == len(y['images'])
        for p, q in zip(x['images'], y['images']):
            np.testing.assert_array_equal(p, q)
        assert repr(x['plans']) == repr(y['plans'])
        for k in ('gt_bboxes', 'gt_labels', 'gt_bboxes_ignore'):
            for p, q in zip(x.get(k, []), y.get(k, [])):
                np.testing.assert_array_equal(p, q)


def test_thread_pool_size_rule(root):
    assert [DL.threads_for_workers(w) for w in (0, 1, 2, 4, 8, 9, 64)] == \
        [1, 2, 4, 8, 16, 16, 16]
    ds = voc(root)
    assert DL.DeviceDataLoader(ds, 1, 3).num_threads == 6
    # num_threads= names the size itself, capped like the rule
    assert [DL.build_dataloader(ds, 1, 8, num_threads=t).num_threads
            for t in (1, 3, 16, 64)] == [1, 3, 16, 16]
    with pytest.raises(ValueError):
        DL.DeviceDataLoader(ds, 1, 1, num_threads=0)


def test_batch_seed_is_stable():
    """sha256 of the three numbers: the same in every process."""
    import hashlib
    assert DL.batch_seed(0, 0, 0) == 493420924 == int.from_bytes(
        hashlib.sha256(b'0,0,0').digest()[:4], 'little')
    assert len({DL.batch_seed(s, e, b) for s in range(3) for e in range(3)
                for b in range(3)}) == 27


@pytest.mark.parametrize('spg', (1, 2))
def test_same_seed_any_thread_count(root, spg):
    ds = voc(root)
    hosts = []
    for threads in (1, 4):
        ld = DL.DeviceDataLoader(ds, spg, 1, seed=7, num_threads=threads)
        hosts.append(_epoch(ld, 0))
        assert ld._pool._max_workers == threads
        ld.close()
    _same_hosts(hosts[0], hosts[1])
    h = hosts[0]
    # every image is used; groups are padded to a multiple of samples_per_gpu
    assert {i for b in h for i in b['indices']} == set(range(5))
    assert len(h) == (5 if spg == 1 else 3)
    for b in h:
        assert len(b['indices']) == spg
        assert len({int(ds.flag[i]) for i in b['indices']}) == 1  # one group
        for im, i, (name, ori) in zip(b['images'], b['indices'],
                                      b['filenames']):
            info = ds.data_infos[i]
            assert im.shape == (info['height'], info['width'], 3)
            assert im.dtype == np.uint8 and im.flags['C_CONTIGUOUS']
            assert ori == info['filename']
            assert name == os.path.join(ds.img_prefix, ori)
        for p, im in zip(b['plans'], b['images']):
            assert p['ori_shape'] == im.shape
            assert p['scale'][0] == 160 and 96 <= p['scale'][1] <= 128


def test_epochs_differ_and_repeat(root):
    ds = voc(root)
    ld = DL.DeviceDataLoader(ds, 2, 2, seed=7)
    assert ld.num_threads == 4 and len(ld) == 3
    e0, e1, e0b = _epoch(ld, 0), _epoch(ld, 1), _epoch(ld, 0)
    _same_hosts(e0, e0b)
    assert repr([(b['indices'], b['plans']) for b in e0]) != \
        repr([(b['indices'], b['plans']) for b in e1])
    # a batch alone equals the same batch inside its epoch
    one = ld.host_batch(1, 2)
    _same_hosts([one], [e1[2]])
    # another seed: other draws
    other = _epoch(DL.DeviceDataLoader(ds, 2, 2, seed=8), 0)
    assert repr([(b['indices'], b['plans']) for b in e0]) != \
        repr([(b['indices'], b['plans']) for b in other])
    # the global generator is left where it was
    np.random.seed(3)
    a = np.random.rand()
    np.random.seed(3)
    ld.epoch_order(5)
    assert np.random.rand() == a
    # set_epoch / call
    ld.set_epoch(1)
    assert ld.epoch_order() == ld.epoch_order(1) != ld.epoch_order(0)


def test_sequential_test_order_and_views(root):
    ds = voc(root, train=False)
    ld = DL.DeviceDataLoader(ds, 2, 1, shuffle=False)
    assert ld.epoch_order() == list(range(8)) and len(ld) == 4
    assert not ld.multi_view and ld.batch_size == 2
    hosts = _epoch(ld, 0)
    assert [b['indices'] for b in hosts] == [[0, 1], [2, 3], [4, 5], [6, 7]]
    assert all(len(p) == 1 and not p[0]['flip'] for b in hosts
               for p in b['plans'])
    assert 'gt_bboxes' not in hosts[0]
    tta = DL.DeviceDataLoader(voc(root, train=False, flip=True), 2, 1,
                              shuffle=False)
    assert tta.multi_view and tta.batch_size == 1 and len(tta) == 8
    h = tta.host_batch(0, 3)
    assert h['indices'] == [3] and [p['flip'] for p in h['plans'][0]] == \
        [False, True]
    dist = DL.DeviceDataLoader(ds, 1, 1, dist=True, shuffle=False,
                               num_replicas=3, rank=1)
    assert dist.epoch_order() == [1, 4, 7] and len(dist) == 3
    assert DL.DeviceDataLoader(ds, 1, 1, dist=True, shuffle=False,
                               num_replicas=3, rank=2).epoch_order() == \
        [2, 5, 0]


def test_distributed_group_order(root):
    ds = voc(root)
    parts = []
    for rank in range(2):
        ld = DL.build_dataloader(ds, 1, 1, dist=True, seed=3, num_replicas=2,
                                 rank=rank)
        parts.append(ld.epoch_order(4))
        assert ld.epoch_order(4) != ld.epoch_order(5)
    assert len(parts[0]) == len(parts[1]) == 3
    assert set(parts[0] + parts[1]) == set(range(5))
    with pytest.raises(NotImplementedError, match='num_gpus'):
        DL.build_dataloader(ds, 1, 1, num_gpus=2)


def test_look_ahead_is_bounded(root, monkeypatch):
    """While the caller holds batch k, exactly the LOOK_AHEAD batches after it
    have been handed to the decode pool, never more."""
    ds = voc(root)
    ld = DL.DeviceDataLoader(ds, 1, 1, seed=1)
    started = []
    real = ld._submit

    def spy(order, epoch, index):
        started.append(index)
        return real(order, epoch, index)

    monkeypatch.setattr(ld, '_submit', spy)
    it = ld.host_batches(0)
    order = ld.epoch_order(0)
    assert DL.LOOK_AHEAD == 2 and len(order) == 5
    for k in range(len(order)):
        got = next(it)
        assert got['indices'] == [order[k]]
        assert started == list(range(min(k + 1 + DL.LOOK_AHEAD, len(order))))
    assert next(it, None) is None


def test_decode_grey_and_exif(tmp_path):
    from PIL import Image
    grey = np.arange(24 * 40, dtype=np.uint8).reshape(24, 40)
    Image.fromarray(grey, 'L').save(str(tmp_path / 'g.jpg'), quality=95)
    g = DL.imread(str(tmp_path / 'g.jpg'))
    assert g.shape == (24, 40, 3) and g.dtype == np.uint8
    assert (g[..., 0] == g[..., 1]).all() and (g[..., 1] == g[..., 2]).all()
    # orientation 6: the stored 20 x 50 (h x w) picture is shown 50 x 20
    pix = np.zeros((20, 50, 3), np.uint8)
    pix[:, :25] = (255, 0, 0)  # left half red
    exif = Image.Exif()
    exif[0x0112] = 6
    Image.fromarray(pix, 'RGB').save(str(tmp_path / 'r.jpg'), quality=95,
                                     exif=exif)
    r = DL.imread(str(tmp_path / 'r.jpg'))
    assert r.shape == (50, 20, 3)
    # rotated 90 degrees clockwise: the red (BGR: channel 2) half is on top
    assert r[:20, :, 2].mean() > 200 and r[30:, :, 2].mean() < 50
    assert r[:20, :, 0].mean() < 50
    plain = DL.imread(str(tmp_path / 'g.jpg'))
    np.testing.assert_array_equal(plain, g)
    png = np.random.RandomState(0).randint(0, 256, (9, 7, 4)).astype(np.uint8)
    Image.fromarray(png, 'RGBA').save(str(tmp_path / 'a.png'))
    a = DL.imread(str(tmp_path / 'a.png'))
    np.testing.assert_array_equal(a, png[:, :, 2::-1])  # BGR, alpha dropped


def test_wrapped_datasets_load(root):
    ds = voc(root)
    rep = D.RepeatDataset(ds, 2)
    cat = D.ConcatDataset([ds, rep])
    ld = DL.DeviceDataLoader(cat, 1, 1, shuffle=False)
    ld.test_mode = False
    h = ld.host_batch(0, 12)  # 5 + (12 - 5) % 5 = image 2 of the dataset
    assert h['filenames'][0][1] == ds.data_infos[2]['filename']
    np.testing.assert_array_equal(h['gt_bboxes'][0],
                                  ds.get_ann_info(2)['bboxes'])
