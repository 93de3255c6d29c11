"""GPU checks (-m gpu) of the layer that runs a config end to end: the loader's
device half, ``single_gpu_test``, ``dataset.evaluate`` and the streamed
evaluators, ``inference_detector``, ``EpochRunner`` fed by a loader with a
validation pass, and tools/test.py / tools/train.py as child processes.

Everything runs on the 8 fixture images (24 x 40 to 100 x 130 pixels,
tests/_dataset_fixture.py) at img_scale (160, 128) with the seeded R18 <- R18 LD
detector and score_thr 0.001.  Bars: bit for bit (assert_array_equal /
torch.equal) against the same work done by hand; ``evaluate`` against the
REFERENCE's numbers in tests/golden/datasets.npz."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dataset_fixture as FX  # noqa: E402
import test_dataloader_host as TH  # noqa: E402  (pipelines, voc())

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden', 'datasets.npz')
DEV = torch.device('cuda:0')
# the seeded detector has 80 class outputs: VOC's 20 names, then fillers
NAMES80 = FX.VOC_CLASSES + tuple(f'filler{k}' for k in range(20, 80))


@pytest.fixture(scope='module')
def root(tmp_path_factory):
    return FX.write_fixture(tmp_path_factory.mktemp('fixture'))


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


@pytest.fixture(scope='module')
def det():
    from ld_amd import model_zoo
    d = model_zoo.build_seeded_ld_detector(18, 18, DEV).eval()
    d.bbox_head.test_cfg['score_thr'] = 0.001  # seeded weights score low
    d.CLASSES = NAMES80
    return d


def _voc80(root, flip=False):
    from ld_amd import datasets as D
    kw = dict(FX.dataset_kwargs(root)['voc_test'][1], classes=NAMES80,
              pipeline=TH.make_test_pipeline(flip))
    return D.VOCDataset(**kw)


def _loader(ds, spg, threads=2, **kw):
    from ld_amd.dataloader import DeviceDataLoader
    return DeviceDataLoader(ds, spg, 1, device=DEV, num_threads=threads, **kw)


def _same_meta(a, b):
    assert set(a) == set(b), (sorted(a), sorted(b))
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype
            np.testing.assert_array_equal(a[k], b[k])
        elif isinstance(a[k], dict):
            _same_meta(a[k], b[k])
        else:
            assert a[k] == b[k], k


def _same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y)
        for p, q in zip(x, y):
            assert p.dtype == q.dtype == np.float32 and p.shape == q.shape
            np.testing.assert_array_equal(p, q)


# ---------------------------------------------------------------- loader ----
@pytest.mark.parametrize('threads', (1, 4))
@pytest.mark.parametrize('spg', (1, 2))
def test_loader_batches_equal_by_hand_pipeline(root, spg, threads):
    from ld_amd.pipeline import DevicePipeline
    ds = TH.voc(root)
    # seed 7 flips 3 of 5 (spg 1) and 4 of 6 (spg 2) images of epoch 1
    ld = _loader(ds, spg, threads, seed=7)
    pipe = DevicePipeline.from_cfg(TH.TRAIN_PIPELINE, device=DEV)
    hosts = list(ld.host_batches(1))
    batches = list(ld(1))
    assert len(batches) == len(hosts) == (5 if spg == 1 else 3)
    flips = 0
    for host, got in zip(hosts, batches):
        want = pipe(host['images'], host['gt_bboxes'], host['gt_labels'],
                    plans=host['plans'],
                    gt_bboxes_ignore=host['gt_bboxes_ignore'])
        assert set(got) == {'img', 'img_metas', 'gt_bboxes', 'gt_labels',
                            'gt_bboxes_ignore'}
        assert got['img'].shape[0] == spg and got['img'].dtype == torch.float32
        assert torch.equal(got['img'], want['img'])
        for k in ('gt_bboxes', 'gt_labels', 'gt_bboxes_ignore'):
            assert len(got[k]) == spg
            for p, q in zip(got[k], want[k]):
                assert p.dtype == q.dtype and p.device.type == 'cuda'
                assert torch.equal(p, q)
        for m, w, (name, ori), i in zip(got['img_metas'], want['img_metas'],
                                        host['filenames'], host['indices']):
            assert m['filename'] == name and m['ori_filename'] == ori
            assert os.path.exists(name)
            _same_meta({k: v for k, v in m.items()
                        if k not in ('filename', 'ori_filename')}, w)
            flips += int(m['flip'])
        # every image brings its ignored boxes (000001 and 000005 have one)
        assert [len(a) for a in got['gt_bboxes_ignore']] == \
            [len(ds.get_ann_info(j)['bboxes_ignore'])
             for j in host['indices']]
    assert flips == (3 if spg == 1 else 4)
    ld.close()


def test_pipeline_ignored_boxes_follow_gt_boxes(root):
    """gt_bboxes_ignore= goes through the transform of gt_bboxes; without it
    the batch has no such key (today's behaviour)."""
    from ld_amd.pipeline import DevicePipeline
    pipe = DevicePipeline.from_cfg(TH.TRAIN_PIPELINE, device=DEV)
    img = np.zeros((100, 130, 3), np.uint8)
    box = np.array([[10, 20, 60, 90]], np.float32)
    plans = pipe.plan([(100, 130)], np.random.RandomState(0))
    plans[0]['flip'] = True
    out = pipe([img], [box], [np.array([1])], plans=plans,
               gt_bboxes_ignore=[box])
    assert torch.equal(out['gt_bboxes'][0], out['gt_bboxes_ignore'][0])
    plain = pipe([img], [box], [np.array([1])], plans=plans)
    assert 'gt_bboxes_ignore' not in plain
    assert torch.equal(plain['gt_bboxes'][0], out['gt_bboxes'][0])
    assert torch.equal(plain['img'], out['img'])


# ------------------------------------------------------- single_gpu_test ----
def _by_hand(det, ld):
    """forward_test per batch on the loader's own host batches."""
    from ld_amd.pipeline import DevicePipeline
    pipe = DevicePipeline.from_test_cfg(ld.dataset.pipeline, device=DEV)
    out = []
    for host in ld.host_batches(0):
        if ld.multi_view:
            imgs, metas = pipe.aug_views(host['images'][0])
        else:
            res = pipe(host['images'], plans=[p[0] for p in host['plans']])
            imgs, metas = [res['img']], [res['img_metas']]
        with torch.no_grad():
            out.extend(det.forward_test(imgs, metas, rescale=True))
    return out


@pytest.fixture(scope='module')
def results_spg1(root, det):
    from ld_amd.apis import single_gpu_test
    ld = _loader(_voc80(root), 1, shuffle=False)
    res = single_gpu_test(det, ld)
    return ld, res


def test_single_gpu_test_single_view(root, det, results_spg1):
    ld, res = results_spg1
    assert len(res) == 8 and all(len(r) == 80 for r in res)
    assert sum(len(c) for r in res for c in r) > 8  # there is something
    _same_results(res, _by_hand(det, ld))
    assert not det.training


def test_single_gpu_test_batched(root, det, results_spg1):
    """samples_per_gpu = 2 against the by-hand BATCHED call: a padded batch
    legitimately differs from per-image calls, as in the reference."""
    from ld_amd.apis import single_gpu_test
    ld = _loader(_voc80(root), 2, 4, shuffle=False)
    res = single_gpu_test(det, ld)
    assert len(res) == 8
    _same_results(res, _by_hand(det, ld))
    ld.close()


def test_single_gpu_test_flip_tta(root, det):
    from ld_amd.apis import single_gpu_test
    ld = _loader(_voc80(root, flip=True), 2, shuffle=False)
    assert ld.multi_view and len(ld) == 8
    res = single_gpu_test(det, ld)
    assert len(res) == 8
    _same_results(res, _by_hand(det, ld))
    ld.close()


# ------------------------------------------------------------ evaluation ----
def _gold_eval(gold, name):
    return dict(zip(gold[f'eval_{name}_keys'].tolist(),
                    gold[f'eval_{name}_vals'].tolist()))


def test_evaluate_equals_reference_golden(root, gold):
    """dataset.evaluate on the seeded results == the reference's evaluate."""
    from ld_amd import datasets as D
    built = {run: D.build_dataset(dict(kw, type=typ))
             for run, (typ, kw) in FX.dataset_kwargs(root).items()
             if run in ('voc_test', 'custom_test')}
    voc, cus = built['voc_test'], built['custom_test']
    res = FX.results_near_gt(voc)
    assert voc.evaluate(res, 'mAP', logger='silent') == \
        _gold_eval(gold, 'voc_map')
    assert voc.evaluate(res, ['mAP'], iou_thr=0.75, logger='silent') == \
        _gold_eval(gold, 'voc_map75')
    # ap_range: the reference's printed AP50 ... AP95 from ONE accumulation
    # equal ten separate evaluations at its accumulated thresholds
    from ld_amd import eval_map
    anns = [voc.get_ann_info(i) for i in range(len(voc))]
    rng = voc.evaluate(res, 'mAP', logger='silent', ap_range=True)
    thr, maps = 0.5, []
    for k in range(10):
        maps.append(eval_map(res, anns, iou_thr=thr, dataset='voc07',
                             logger='silent')[0])
        assert rng[f'AP{50 + 5 * k}'] == maps[-1]
        thr = thr + 0.05
    assert rng['mAP'] == maps[0] == _gold_eval(gold, 'voc_map')['mAP']
    assert rng['AP'] == sum(maps) / 10 and maps[0] > maps[-1]
    assert list(rng) == ['mAP'] + [f'AP{50 + 5 * k}' for k in range(10)] + \
        ['AP']
    res = FX.results_near_gt(cus)
    assert dict(cus.evaluate(res, 'mAP', iou_thr=[0.5, 0.7],
                             logger='silent')) == _gold_eval(gold,
                                                             'custom_map')
    for ds, name in ((voc, 'voc_test_recall'), (cus, 'custom_test_recall')):
        props = [np.concatenate(r) for r in FX.results_near_gt(ds)]
        got = ds.evaluate(props, 'recall', proposal_nums=(1, 3, 10),
                          iou_thr=[0.5, 0.7], logger='silent')
        assert {k: float(v) for k, v in got.items()} == _gold_eval(gold, name)
    cat = D.ConcatDataset([voc, cus])
    got = cat.evaluate(FX.results_near_gt(voc) + FX.results_near_gt(cus),
                       metric='mAP', logger='silent')
    assert {k: float(v) for k, v in got.items()} == \
        _gold_eval(gold, 'concat_map')


def test_evaluate_equals_direct_and_streamed(root, det, results_spg1):
    from ld_amd import eval_map
    from ld_amd.apis import single_gpu_test
    ld, res = results_spg1
    ds = ld.dataset
    anns = [ds.get_ann_info(i) for i in range(len(ds))]
    got = ds.evaluate(res, 'mAP', logger='silent')
    want, _ = eval_map(res, anns, iou_thr=0.5, dataset='voc07',
                       logger='silent')
    assert got == {'mAP': want}
    # streamed: the device detections of every batch straight into the
    # accumulator; same bits as the host round trip
    ev = ds.make_evaluator('mAP')
    again = single_gpu_test(det, ld, evaluator=ev)
    _same_results(again, res)
    assert ev.compute(logger='silent')[0][0] == want
    rec = ds.make_evaluator('recall', iou_thr=[0.5, 0.7],
                            proposal_nums=(1, 10, 100))
    single_gpu_test(det, ld, evaluator=rec)
    props = [np.concatenate(r) for r in res]
    want = ds.evaluate(props, 'recall', proposal_nums=(1, 10, 100),
                       iou_thr=[0.5, 0.7], logger='silent')
    got = rec.evaluate(logger='silent')
    assert list(got) == list(want)
    for k in want:
        np.testing.assert_array_equal(np.float64(got[k]), np.float64(want[k]))


def test_coco_evaluate_direct_streamed_and_json_round_trip(root, det,
                                                           tmp_path):
    from ld_amd import coco_evaluate, datasets as D
    from ld_amd.apis import single_gpu_test
    ds = D.CocoDataset(ann_file='coco.json', img_prefix='', data_root=root,
                       pipeline=TH.make_test_pipeline(), test_mode=True)
    assert ds.cat_ids == [1, 2, 3, 18]
    ld = _loader(ds, 2, shuffle=False)
    ev = ds.make_evaluator('bbox')
    res = single_gpu_test(det, ld, evaluator=ev)
    ld.close()
    # the detector has 80 class arrays, the json 4 categories: labels 0-3
    res4 = [r[:4] for r in res]
    got = ds.evaluate(res4, 'bbox', logger='silent',
                      jsonfile_prefix=str(tmp_path / 'dets'))
    want = coco_evaluate(res4, ds.ground_truth(), logger='silent')
    assert got == want and 'bbox_mAP' in got and 'bbox_mAP_copypaste' in got
    assert ev.evaluate(logger='silent') == want  # streamed
    back = ds.json2results(str(tmp_path / 'dets.bbox.json'))
    assert ds.evaluate(back, 'bbox', logger='silent') == want
    fast = ds.evaluate([np.concatenate(r) for r in res4], 'proposal_fast',
                       logger='silent')
    assert list(fast) == ['AR@100', 'AR@300', 'AR@1000']


# ---------------------------------------------------------- inference api ----
def test_inference_detector_path_equals_array(root, det, results_spg1):
    from ld_amd import Config
    from ld_amd.apis import inference_detector
    from ld_amd.dataloader import imread
    ld, res = results_spg1
    det.cfg = Config(dict(data=dict(test=dict(pipeline=TH.make_test_pipeline()))))
    try:
        paths = [ld.dataset.img_path(i) for i in (0, 3, 6)]
        by_path = inference_detector(det, paths)
        by_array = inference_detector(det, [imread(p) for p in paths])
        _same_results(by_path, by_array)
        one = inference_detector(det, paths[1])
        _same_results([one], [by_path[1]])
        # and it is the test loop's answer for that image
        _same_results(by_path, [res[i] for i in (0, 3, 6)])
    finally:
        del det.cfg
        del det._inference_pipeline


# ------------------------------------------------------------ EpochRunner ----
def _train_cfg(**extra):
    cfg = dict(
        optimizer=dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001),
        optimizer_config=dict(grad_clip=dict(max_norm=35.0, norm_type=2)),
        lr_config=dict(policy='step', warmup='linear', warmup_iters=3,
                       warmup_ratio=0.001, step=[1]),
        runner=dict(type='EpochBasedRunner', max_epochs=2),
        log_config=dict(interval=1), checkpoint_config=dict(interval=1),
        evaluation=dict(interval=1, metric='mAP'))
    cfg.update(extra)
    return cfg


def _trainer(cfg):
    from ld_amd import model_zoo
    from ld_amd.train import SGDTrainer
    d = model_zoo.build_seeded_ld_detector(18, 18, DEV)
    d.bbox_head.test_cfg['score_thr'] = 0.001
    d.CLASSES = NAMES80
    return SGDTrainer.from_config(d, cfg)


def test_epoch_runner_with_loader_and_val(root, tmp_path):
    from ld_amd.apis import single_gpu_test
    from ld_amd.runner import EpochRunner
    cfg = _train_cfg()
    train_set, val_set = TH.voc(root), TH.voc(root, train=False)
    ld = _loader(train_set, 2, seed=5)
    vld = _loader(val_set, 2, shuffle=False)
    assert len(ld) == 3
    tr = _trainer(cfg)
    run = EpochRunner(tr, cfg, tmp_path / 'a',
                      val=(vld, val_set, cfg['evaluation']))
    recs = run.run(ld)
    torch.cuda.synchronize()
    # the same batches by hand, no validation
    ld2 = _loader(train_set, 2, 4, seed=5)
    batches = [list(ld2(e)) for e in range(2)]
    tr2 = _trainer(cfg)
    recs2 = EpochRunner(tr2, cfg, tmp_path / 'b').run(lambda e: batches[e])
    torch.cuda.synchronize()
    assert [(r['epoch'], r['iter']) for r in recs] == \
        [(1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 3)]
    assert recs == recs2
    assert torch.equal(tr.arena.flat_param, tr2.arena.flat_param)
    lines = [json.loads(x) for x in
             open(tmp_path / 'a' / 'train.log.json').read().splitlines()]
    val = [r for r in lines if r['mode'] == 'val']
    assert [r for r in lines if r['mode'] == 'train'] == recs
    assert [r['epoch'] for r in val] == [1, 2] == \
        [r['epoch'] for r in run.val_records]
    # one val line per epoch, after that epoch's train lines
    assert [r['mode'] for r in lines] == ['train'] * 3 + ['val'] + \
        ['train'] * 3 + ['val']
    assert tr.model.training  # the validation pass hands the mode back
    final = val_set.evaluate(single_gpu_test(tr.model, vld), metric='mAP',
                             logger='silent')
    assert val[1]['mAP'] == float(final['mAP']) and val[1]['iter'] == len(vld)
    ck = torch.load(tmp_path / 'a' / 'epoch_2.pth', map_location='cpu')
    assert tuple(ck['meta']['CLASSES']) == NAMES80
    assert ck['meta']['epoch'] == 2 and ck['meta']['iter'] == 6
    lines_b = open(tmp_path / 'b' / 'train.log.json').read().splitlines()
    assert len(lines_b) == 6  # without val nothing changes
    for x in (ld, ld2, vld):
        x.close()


# ------------------------------------------------------------------ tools ----
CONFIG = '''\
from ld_amd import model_zoo

model = model_zoo.ld_detector(18, 18)
model['test_cfg']['score_thr'] = 0.001
model['bbox_head']['num_classes'] = 20
model['teacher_config']['model']['bbox_head']['num_classes'] = 20
norm = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375],
            to_rgb=True)
train_pipeline = [
    dict(type='LoadImageFromFile'),
    dict(type='LoadAnnotations', with_bbox=True),
    dict(type='Resize', img_scale=[(160, 96), (160, 128)],
         multiscale_mode='range', keep_ratio=True),
    dict(type='RandomFlip', flip_ratio=0.5),
    dict(type='Normalize', **norm),
    dict(type='Pad', size_divisor=32),
    dict(type='DefaultFormatBundle'),
    dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]
test_pipeline = [
    dict(type='LoadImageFromFile'),
    dict(type='MultiScaleFlipAug', img_scale=(160, 128), flip=False,
         transforms=[dict(type='Resize', keep_ratio=True),
                     dict(type='RandomFlip'),
                     dict(type='Normalize', **norm),
                     dict(type='Pad', size_divisor=32),
                     dict(type='ImageToTensor', keys=['img']),
                     dict(type='Collect', keys=['img'])])]
voc = dict(type='VOCDataset', data_root={root!r},
           ann_file='VOC2007/ImageSets/Main/trainval.txt',
           img_prefix='VOC2007/')
data = dict(samples_per_gpu=2, workers_per_gpu=1,
            train=dict(pipeline=train_pipeline, **voc),
            val=dict(pipeline=test_pipeline, **voc),
            test=dict(pipeline=test_pipeline, samples_per_gpu=2, **voc))
evaluation = dict(interval=1, metric='mAP')
optimizer = dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001)
optimizer_config = dict(grad_clip=dict(max_norm=35.0, norm_type=2))
lr_config = dict(policy='step', warmup='linear', warmup_iters=3,
                 warmup_ratio=0.001, step=[1])
runner = dict(type='EpochBasedRunner', max_epochs=2)
log_config = dict(interval=1)
checkpoint_config = dict(interval=1)
'''


def _child(args, cwd):
    """One fresh child process under its own time limit."""
    cmd = ['timeout', '-k', '10', '120', sys.executable] + args
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run(cmd, cwd=str(cwd), env=env, capture_output=True,
                       text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:],
                               r.stderr[-4000:])
    return r


def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        f'_tool_{name}', os.path.join(REPO, 'tools', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tools_train_then_test_as_child_processes(root, tmp_path):
    """tools/train.py and tools/test.py once each as a child; the first
    non-zero exit stops the test.  The train child's last checkpoint equals
    the same run made in this process bit for bit, the test child's pkl equals
    single_gpu_test here."""
    cfg_path = tmp_path / 'ld_r18_fixture.py'
    cfg_path.write_text(CONFIG.format(root=str(root)))
    train_args = [str(cfg_path), '--seed', '3', '--deterministic']
    _child([os.path.join(REPO, 'tools', 'train.py')] + train_args +
           ['--work-dir', str(tmp_path / 'child')], tmp_path)
    _tool('train').main(train_args + ['--work-dir', str(tmp_path / 'here')])
    a = torch.load(tmp_path / 'child' / 'epoch_2.pth', map_location='cpu')
    b = torch.load(tmp_path / 'here' / 'epoch_2.pth', map_location='cpu')
    assert list(a['state_dict']) == list(b['state_dict'])
    for k in a['state_dict']:
        assert torch.equal(a['state_dict'][k], b['state_dict'][k]), k
    assert tuple(a['meta']['CLASSES']) == FX.VOC_CLASSES
    assert a['meta']['iter'] == b['meta']['iter'] == 6
    la = open(tmp_path / 'child' / 'train.log.json').read()
    assert la == open(tmp_path / 'here' / 'train.log.json').read()
    assert la.count('"mode": "val"') == 2 and la.count('"mode": "train"') == 6
    assert os.path.isfile(tmp_path / 'child' / 'ld_r18_fixture.py')
    # tools/test.py on that checkpoint
    ckpt = str(tmp_path / 'child' / 'epoch_2.pth')
    out = str(tmp_path / 'res.pkl')
    r = _child([os.path.join(REPO, 'tools', 'test.py'), str(cfg_path), ckpt,
                '--out', out, '--eval', 'mAP', '--show-dir',
                str(tmp_path / 'shown')], tmp_path)
    from ld_amd import Config
    from ld_amd.apis import single_gpu_test
    from ld_amd.cli import load_for_test, pop_test_samples_per_gpu
    from ld_amd.datasets import build_dataset
    cfg = Config.fromfile(str(cfg_path))
    spg = pop_test_samples_per_gpu(cfg)
    ds = build_dataset(cfg.data['test'])
    assert spg == 2 and len(ds) == 8
    model = load_for_test(cfg, ckpt, DEV, ds.CLASSES)
    assert tuple(model.CLASSES) == FX.VOC_CLASSES
    ld = _loader(ds, spg, shuffle=False)
    here = single_gpu_test(model, ld)
    ld.close()
    _same_results(pickle.load(open(out, 'rb')), here)
    assert "'mAP'" in r.stdout
    shown = sorted(os.listdir(tmp_path / 'shown' / 'JPEGImages'))
    assert shown == [f'{i[0]}.png' for i in FX.IMAGES]
