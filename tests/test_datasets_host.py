"""CPU checks of ld_amd.datasets against what the REFERENCE's dataset classes
returned on the same seeded fixture tree (tests/golden/datasets.npz, written
by tools/gen_golden_datasets.py): values, dtypes and empty shapes exact.
CocoDataset has no reference run (pycocotools is absent): it is pinned on
answers derived by hand from coco.py, rule by rule."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dataset_fixture as FX  # noqa: E402

from ld_amd import datasets as D  # noqa: E402
from ld_amd.config import Config  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden', 'datasets.npz')
REFERENCE = os.environ.get('LD_REFERENCE_ROOT', '/root/reference')
needs_reference = pytest.mark.skipif(
    not os.path.isdir(os.path.join(REFERENCE, 'configs', 'ld')),
    reason='needs the reference checkout for its config files')
RUNS = ('voc_train', 'voc_test', 'voc_nofilter', 'voc_minsize', 'xml_classes',
        'custom_train', 'custom_test')


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


@pytest.fixture(scope='module')
def root(tmp_path_factory):
    return FX.write_fixture(tmp_path_factory.mktemp('fixture'))


@pytest.fixture(scope='module')
def built(root):
    import warnings
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for run, (typ, kw) in FX.dataset_kwargs(root).items():
            out[run] = D.build_dataset(dict(kw, type=typ))
    return out


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype, (what, a.dtype, b.dtype)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    np.testing.assert_array_equal(a, b, err_msg=what)


@pytest.mark.parametrize('run', RUNS)
def test_dataset_equals_reference(gold, built, run):
    ds = built[run]
    train = not ds.test_mode
    assert len(ds) == int(gold[f'{run}_len'])
    infos = ds.data_infos
    assert [i.get('id', i['filename']) for i in infos] == \
        gold[f'{run}_ids'].tolist()
    assert [i['filename'] for i in infos] == gold[f'{run}_filename'].tolist()
    assert [i['width'] for i in infos] == gold[f'{run}_width'].tolist()
    assert [i['height'] for i in infos] == gold[f'{run}_height'].tolist()
    if train:
        _same(ds.flag, gold[f'{run}_flag'], 'flag')
    else:
        assert not hasattr(ds, 'flag')
    for i in range(len(ds)):
        ann = ds.get_ann_info(i)
        for k in ('bboxes', 'labels', 'bboxes_ignore', 'labels_ignore'):
            _same(ann[k], gold[f'{run}_{i}_{k}'], f'{run}[{i}].{k}')
        assert ds.get_cat_ids(i) == gold[f'{run}_{i}_cat_ids'].tolist()


def test_fixture_covers_the_edge_cases(built):
    """The goldens above mean something only if the tree has the cases."""
    tr, te = built['voc_train'], built['voc_test']
    assert [i['id'] for i in te.data_infos] == [i[0] for i in FX.IMAGES]
    # too small, only-unknown and empty images are filtered in train mode
    assert [i['id'] for i in tr.data_infos] == \
        ['000001', '000002', '000005', '000006', '000007']
    assert set(tr.flag.tolist()) == {0, 1}  # portrait and landscape
    assert tr.flag.tolist() == [1, 0, 0, 1, 0]  # 100 x 100 is not > 1
    a = tr.get_ann_info(0)  # difficult -> ignore, float coords truncated, - 1
    assert a['bboxes'].tolist() == [[11, 19, 89, 76], [4, 39, 47, 87]]
    assert a['bboxes_ignore'].tolist() == [[59, 9, 99, 94]]
    assert a['labels'].tolist() == [6, 11] and a['labels_ignore'].tolist() == [14]
    e = te.get_ann_info(7)  # empty arrays keep their shapes and dtypes
    assert e['bboxes'].shape == (0, 4) and e['bboxes'].dtype == np.float32
    assert e['labels'].shape == (0, ) and e['labels'].dtype == np.int64
    assert e['bboxes_ignore'].shape == (0, 4)
    # the file without <size> got its size from the image
    assert (te.data_infos[4]['width'], te.data_infos[4]['height']) == (100, 100)
    # min_size: the 6 x 40 and 7 x 8 boxes of 000006 move to the ignored field
    m = built['voc_minsize'].get_ann_info(3)
    assert len(m['bboxes']) == 1 and len(m['bboxes_ignore']) == 2
    assert built['voc_train'].year == 2007


def test_min_size_in_test_mode_is_an_error(root):
    kw = dict(FX.dataset_kwargs(root)['voc_test'][1], min_size=10)
    ds = D.VOCDataset(**kw)
    with pytest.raises(AssertionError):
        ds.get_ann_info(0)


def test_year_from_img_prefix(root, tmp_path):
    kw = dict(FX.dataset_kwargs(root)['voc_train'][1])
    os.symlink(os.path.join(root, 'VOC2007'), str(tmp_path / 'VOC2012'))
    ds = D.VOCDataset(**dict(kw, data_root=str(tmp_path),
                             ann_file='VOC2012/ImageSets/Main/trainval.txt',
                             img_prefix='VOC2012/'))
    assert ds.year == 2012 and ds._map_dataset_name() == D.VOCDataset.CLASSES
    assert D.VOCDataset(**kw)._map_dataset_name() == 'voc07'
    os.symlink(os.path.join(root, 'VOC2007'), str(tmp_path / 'other'))
    with pytest.raises(ValueError, match='year'):
        D.VOCDataset(**dict(kw, data_root=str(tmp_path),
                            ann_file='other/ImageSets/Main/trainval.txt',
                            img_prefix='other/'))


def test_wrappers_equal_reference(gold, built):
    rep = D.RepeatDataset(built['voc_train'], 3)
    assert len(rep) == int(gold['repeat_len']) == 15
    _same(rep.flag, gold['repeat_flag'], 'repeat flag')
    assert [json.dumps(rep.get_cat_ids(i)) for i in range(len(rep))] == \
        gold['repeat_cat_ids'].tolist()
    assert rep[7]['img_info'] is built['voc_train'][2]['img_info']
    cat = D.ConcatDataset([built['voc_train'], built['voc_minsize'],
                           built['xml_classes']])
    assert len(cat) == int(gold['concat_len'])
    _same(cat.flag, gold['concat_flag'], 'concat flag')
    assert list(cat.cumulative_sizes) == \
        gold['concat_cumulative_sizes'].tolist()
    assert [json.dumps(cat.get_cat_ids(i)) for i in range(len(cat))] == \
        gold['concat_cat_ids'].tolist()
    assert [json.dumps(cat.get_cat_ids(-i))
            for i in range(1, len(cat) + 1)] == \
        gold['concat_cat_ids_neg'].tolist()
    with pytest.raises(ValueError):
        cat.get_cat_ids(-len(cat) - 1)
    # index map
    assert cat.locate(0) == (0, 0) and cat.locate(5) == (1, 0)
    assert cat.locate(len(cat) - 1) == (2, 3)
    assert cat[5]['img_info'] is built['voc_minsize'][0]['img_info']
    assert cat.CLASSES == built['voc_train'].CLASSES
    with pytest.raises(NotImplementedError):
        D.ConcatDataset([built['voc_train'], built['custom_train']],
                        separate_eval=False)


def test_group_sampler_order_equals_reference(gold, built):
    """Our dataset's flag through the existing GroupSampler gives the order
    the reference's sampler gave on the reference's dataset."""
    from ld_amd.pipeline import GroupSampler
    for spg in (1, 2, 3):
        np.random.seed(5)
        got = list(GroupSampler(built['voc_train'], spg))
        assert got == gold[f'sampler_{spg}'].tolist()


def test_ann_file_list_concatenates(root, built):
    """builder.py:26-50, the VOC07+12 form."""
    kw = dict(FX.dataset_kwargs(root)['voc_train'][1], type='VOCDataset')
    kw['ann_file'] = [kw['ann_file'], 'VOC2007/ImageSets/Main/test.txt']
    kw['img_prefix'] = ['VOC2007/', 'VOC2007/']
    ds = D.build_dataset(kw)
    assert isinstance(ds, D.ConcatDataset) and len(ds.datasets) == 2
    assert len(ds) == 10 and ds.flag.tolist() == [1, 0, 0, 1, 0] * 2
    rep = D.build_dataset(dict(type='RepeatDataset', times=2, dataset=kw))
    assert isinstance(rep, D.RepeatDataset) and len(rep) == 20
    both = D.build_dataset([dict(kw, ann_file=kw['ann_file'][0],
                                 img_prefix='VOC2007/')] * 2)
    assert isinstance(both, D.ConcatDataset) and len(both) == 10
    cc = D.build_dataset(dict(type='ConcatDataset', separate_eval=True,
                              datasets=[dict(kw, ann_file=kw['ann_file'][0],
                                             img_prefix='VOC2007/')]))
    assert len(cc) == 5


def test_classes_override_three_forms(root):
    kw = dict(FX.dataset_kwargs(root)['voc_train'][1])
    assert D.VOCDataset(**kw).CLASSES == FX.VOC_CLASSES
    t = D.VOCDataset(**dict(kw, classes=('dog', 'person', 'car')))
    assert t.CLASSES == ('dog', 'person', 'car')
    l = D.VOCDataset(**dict(kw, classes=['dog', 'person', 'car']))
    f = D.VOCDataset(**dict(kw, classes=os.path.join(root, 'classes.txt')))
    assert f.CLASSES == ['dog', 'person', 'car'] == l.CLASSES
    for ds in (t, l, f):
        assert ds.cat2label == {'dog': 0, 'person': 1, 'car': 2}
        assert [i['id'] for i in ds.data_infos] == \
            ['000001', '000002', '000006', '000007']
        assert ds.get_ann_info(0)['labels'].tolist() == [2, 0]
    with pytest.raises(ValueError):
        D.VOCDataset(**dict(kw, classes=3))
    with pytest.raises(AssertionError):
        D.XMLDataset(**kw)  # no CLASSES of its own


def test_data_root_joining(root):
    """custom.py:74-85: relative paths are joined, absolute ones and None
    are kept."""
    kw = dict(FX.dataset_kwargs(root)['voc_test'][1])
    ds = D.VOCDataset(**kw)
    assert ds.ann_file == os.path.join(
        root, 'VOC2007/ImageSets/Main/trainval.txt')
    assert ds.img_prefix == os.path.join(root, 'VOC2007/')
    assert ds.img_path(0) == os.path.join(root, 'VOC2007/',
                                          'JPEGImages/000001.jpg')
    assert os.path.exists(ds.img_path(0))
    ab = D.VOCDataset(**dict(kw, ann_file=ds.ann_file,
                             img_prefix=ds.img_prefix, data_root='/nowhere'))
    assert ab.ann_file == ds.ann_file and ab.img_prefix == ds.img_prefix
    no = D.VOCDataset(**dict(kw, ann_file=ds.ann_file,
                             img_prefix=ds.img_prefix, data_root=None))
    assert no.ann_file == ds.ann_file
    mid = dict(FX.dataset_kwargs(root)['custom_test'][1])
    c = D.CustomDataset(**dict(mid, img_prefix=None))
    assert c.img_prefix is None
    assert c.img_path(0) == 'VOC2007/JPEGImages/000001.jpg'
    c = D.CustomDataset(**mid)
    assert c.img_path(0) == os.path.join(root, '',
                                         'VOC2007/JPEGImages/000001.jpg')


def test_custom_json_equals_pkl(root, built):
    kw = dict(FX.dataset_kwargs(root)['custom_test'][1], ann_file='middle.json')
    js, pk = D.CustomDataset(**kw), built['custom_test']
    assert len(js) == len(pk) == 8
    for i in range(8):
        a, b = js.get_ann_info(i), pk.get_ann_info(i)
        for k in ('bboxes', 'labels', 'bboxes_ignore', 'labels_ignore'):
            _same(a[k], b[k], k)
    with pytest.raises(TypeError):
        D.CustomDataset(**dict(kw, ann_file='classes.txt'))


# ---------------------------------------------------------------------------
# CocoDataset: hand-derived answers (unpinned against pycocotools)
# ---------------------------------------------------------------------------
COCO4 = ('person', 'bicycle', 'car', 'dog')


def _coco(root, **kw):
    base = dict(ann_file='coco.json', img_prefix='', data_root=root,
                pipeline=[], classes=COCO4)
    base.update(kw)
    return D.CocoDataset(**base)


def test_coco_index_and_filter(root):
    te = _coco(root, test_mode=True)
    # coco.py:58-60: cat_ids in CLASSES order, img_ids in the json's order
    assert te.cat_ids == [1, 2, 3, 18]
    assert te.cat2label == {1: 0, 2: 1, 3: 2, 18: 3}
    assert te.img_ids == [100 + 7 * k for k in range(8)]
    assert [i['filename'] for i in te.data_infos] == \
        [f'VOC2007/JPEGImages/{i[0]}.jpg' for i in FX.IMAGES]
    assert D.CocoDataset.CLASSES[:3] == ('person', 'bicycle', 'car')
    assert len(D.CocoDataset.CLASSES) == 80
    # a different CLASSES order reorders cat_ids and labels
    sw = _coco(root, test_mode=True, classes=('dog', 'person'))
    assert sw.cat_ids == [18, 1] and sw.cat2label == {18: 0, 1: 1}
    # coco.py:98-120.  Image 2 (000003) has only a 'unicorn' annotation, 4
    # (000005) and 7 (000008) have none: dropped with filter_empty_gt; image 3
    # (000004, 40 x 24) is under min_size: dropped always.  img_ids follows.
    tr = _coco(root)
    assert tr.img_ids == [100, 107, 135, 142]
    assert [i['id'] for i in tr.data_infos] == tr.img_ids
    assert tr.flag.tolist() == [1, 0, 1, 0] and tr.flag.dtype == np.uint8
    nf = _coco(root, filter_empty_gt=False)
    assert nf.img_ids == [100, 107, 114, 128, 135, 142, 149]
    assert [i['id'] for i in nf.data_infos] == nf.img_ids
    # get_cat_ids: the raw category ids of the image's annotations (coco.py:96)
    assert tr.get_cat_ids(0) == [3, 1, 18, 1, 1]
    assert tr.get_cat_ids(1) == [18, 999, 2]


def test_coco_parse_ann_info(root):
    tr = _coco(root)
    a = tr.get_ann_info(0)  # image 000001, 130 x 100
    # car kept; crowd person -> ignore (coco.py:151); zero-area dog skipped
    # (:146); the box partly outside is kept UNclipped (:142-150); the one
    # wholly outside has zero intersection (:144)
    np.testing.assert_array_equal(
        a['bboxes'], np.array([[12, 20, 90, 77], [100, 60, 160, 130]],
                              np.float32))
    assert a['labels'].tolist() == [2, 0] and a['labels'].dtype == np.int64
    np.testing.assert_array_equal(
        a['bboxes_ignore'], np.array([[60.5, 10.25, 100.5, 95.25]],
                                     np.float32))
    assert a['bboxes'].dtype == a['bboxes_ignore'].dtype == np.float32
    assert a['seg_map'] == 'VOC2007/JPEGImages/000001.png'
    b = tr.get_ann_info(1)  # dog kept; unicorn outside cat_ids (:148); w < 1
    assert b['bboxes'].tolist() == [[10, 30, 70, 110]]
    assert b['labels'].tolist() == [3] and b['bboxes_ignore'].shape == (0, 4)
    c = tr.get_ann_info(2)  # 000006: the ``ignore`` annotation skipped (:139)
    assert c['bboxes'].tolist() == [[50, 20, 120, 90], [30, 30, 36, 70]]
    assert c['labels'].tolist() == [1, 1]
    d = tr.get_ann_info(3)  # 000007: person; crowd bicycle -> ignore
    assert d['labels'].tolist() == [0]
    assert d['bboxes_ignore'].tolist() == [[10, 50, 60, 99]]
    te = _coco(root, test_mode=True)
    e = te.get_ann_info(4)  # no annotations: empty shapes and dtypes
    assert e['bboxes'].shape == (0, 4) and e['bboxes'].dtype == np.float32
    assert e['labels'].shape == (0, ) and e['labels'].dtype == np.int64
    assert e['bboxes_ignore'].shape == (0, 4)
    # an image with only out-of-CLASSES annotations parses to nothing
    assert te.get_ann_info(2)['bboxes'].shape == (0, 4)


def test_coco_results2json_round_trip(root, tmp_path):
    te = _coco(root, test_mode=True)
    res = FX.seeded_results(len(te), 4)
    assert te.xyxy2xywh(np.array([1.5, 2.0, 4.0, 8.5])) == [1.5, 2.0, 2.5, 6.5]
    files, tmp = te.format_results(res, jsonfile_prefix=str(tmp_path / 'out'))
    assert tmp is None
    assert files == dict(bbox=str(tmp_path / 'out.bbox.json'),
                         proposal=str(tmp_path / 'out.bbox.json'))
    dets = json.load(open(files['bbox']))
    assert len(dets) == sum(len(c) for r in res for c in r)
    first = next((i, c) for i, r in enumerate(res) for c, a in enumerate(r)
                 if len(a))
    b = res[first[0]][first[1]][0]
    assert dets[0] == dict(
        image_id=te.img_ids[first[0]], category_id=te.cat_ids[first[1]],
        bbox=[float(b[0]), float(b[1]), float(b[2]) - float(b[0]),
              float(b[3]) - float(b[1])], score=float(b[4]))
    assert set(dets[0]) == {'image_id', 'bbox', 'score', 'category_id'}
    assert type(dets[0]['score']) is float
    files2, tmp2 = te.format_results(res)
    assert os.path.exists(files2['bbox'])
    tmp2.cleanup()
    props = [np.concatenate(r) for r in res]
    pf = te.results2json(props, str(tmp_path / 'p'))
    assert pf == dict(proposal=str(tmp_path / 'p.proposal.json'))
    assert all(d['category_id'] == 1 for d in json.load(open(pf['proposal'])))
    with pytest.raises(AssertionError):
        te.format_results(res[:-1])
    with pytest.raises(NotImplementedError):
        te.results2json([(r, None) for r in res], str(tmp_path / 'q'))
    # the inverse, for the metric round trip of the GPU test
    back = te.json2results(files['bbox'])
    for r, q in zip(res, back):
        for a, c in zip(r, q):
            assert c.dtype == np.float32 and c.shape == a.shape
            np.testing.assert_allclose(c, a, rtol=0, atol=1e-5)


# ---------------------------------------------------------------------------
# build_dataset on real configs; refusals
# ---------------------------------------------------------------------------
def _reroot(block, root):
    block = dict(block)
    if 'dataset' in block:
        block['dataset'] = _reroot(block['dataset'], root)
        return block
    block['data_root'] = root
    return block


@needs_reference
def test_build_dataset_from_voc_config(root):
    cfg = Config.fromfile(os.path.join(
        REFERENCE, 'configs', 'ld', 'ld_r18_gflv1_r101_fpn_voc_1x.py'))

    def voc07(block):  # the config lists VOC2007 + VOC2012; the tree has 2007
        block = dict(block)
        if 'dataset' in block:
            block['dataset'] = voc07(block['dataset'])
            return block
        for k in ('ann_file', 'img_prefix'):
            v = block[k]
            v = [s for s in v if 'VOC2007' in s] if isinstance(v, list) else v
            block[k] = [os.path.join(root, s[s.index('VOC2007'):])
                        for s in v] if isinstance(v, list) else \
                os.path.join(root, v[v.index('VOC2007'):])
        return block

    tr = D.build_dataset(voc07(cfg.data.train))
    inner = tr
    while not isinstance(inner, D.VOCDataset):
        inner = inner.dataset if hasattr(inner, 'dataset') else \
            inner.datasets[0]
    assert inner.year == 2007 and len(inner) == 5
    assert len(tr) % 5 == 0 and len(tr.flag) == len(tr)
    assert inner.pipeline == list(cfg.data.train.get(
        'dataset', cfg.data.train)['pipeline'])
    # tools/test.py sets test_mode itself (cfg.data.test.test_mode = True)
    te = D.build_dataset(voc07(cfg.data.test), dict(test_mode=True))
    assert isinstance(te, D.VOCDataset) and te.test_mode and len(te) == 8
    assert te.pipeline[1]['type'] == 'MultiScaleFlipAug'


@needs_reference
def test_build_dataset_from_coco_config(root):
    cfg = Config.fromfile(os.path.join(
        REFERENCE, 'configs', 'ld', 'ld_r50_gflv1_r101_fpn_coco_1x.py'))
    for name, n in (('train', 4), ('val', 8), ('test', 8)):
        block = dict(cfg.data[name])
        assert block['type'] == 'CocoDataset'
        block['ann_file'] = os.path.join(root, 'coco.json')
        block['img_prefix'] = root + '/'
        # the tools pass test_mode for val / test (tools/test.py:130,
        # apis/train.py:128)
        ds = D.build_dataset(block, dict(test_mode=name != 'train'))
        assert isinstance(ds, D.CocoDataset) and len(ds) == n
        assert ds.test_mode == (name != 'train')
        assert ds.cat_ids == [1, 2, 3, 18]  # the 80 names the json has
        assert os.path.exists(ds.img_path(0))


@pytest.mark.parametrize('cfg,key', [
    (dict(type='ClassBalancedDataset', oversample_thr=0.1,
          dataset=dict(type='VOCDataset')), 'ClassBalancedDataset'),
    (dict(type='VOCDataset', proposal_file='p.pkl'), 'proposal_file'),
    (dict(type='VOCDataset', seg_prefix='seg/'), 'seg_prefix'),
    (dict(type='VOCDataset', pipeline=[
        dict(type='LoadAnnotations', with_bbox=True, with_mask=True)]),
     'with_mask'),
    (dict(type='VOCDataset', pipeline=[
        dict(type='LoadAnnotations', with_bbox=True, with_seg=True)]),
     'with_seg'),
    (dict(type='CityscapesDataset'), 'CityscapesDataset'),
    (dict(type='LVISV1Dataset'), 'LVISV1Dataset'),
])
def test_refusals_name_their_key(root, cfg, key):
    base = dict(FX.dataset_kwargs(root)['voc_train'][1])
    if cfg['type'] == 'VOCDataset':
        cfg = dict(base, **cfg)
    with pytest.raises(NotImplementedError, match=key):
        D.build_dataset(cfg)


def test_evaluate_argument_rules(root, built):
    """What can be checked without the device evaluators."""
    with pytest.raises(KeyError, match='bbox'):
        built['voc_test'].evaluate([], metric='bbox')
    with pytest.raises(KeyError, match='mAP'):
        _coco(root, test_mode=True).evaluate([[]] * 8, metric='mAP')
    with pytest.raises(NotImplementedError, match='segm'):
        _coco(root, test_mode=True).evaluate([[]] * 8, metric='segm')
    with pytest.raises(AssertionError):
        built['voc_test'].evaluate([], metric=['mAP', 'recall'])
