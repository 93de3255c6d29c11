"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/datasets.npz by EXECUTING THE
REFERENCE's dataset classes on the CPU (the reference package is imported,
unmodified, through oracle/ref_shim.py).  Run from the repo root in the build
container, never on the GPU machine:

    python tools/gen_golden_datasets.py

Reference entry points exercised (file:line under the reference tree):
  mmdet/datasets/custom.py:15-325         CustomDataset
  mmdet/datasets/xml_style.py:12-169      XMLDataset
  mmdet/datasets/voc.py:6-101             VOCDataset (evaluate included)
  mmdet/datasets/dataset_wrappers.py      ConcatDataset, RepeatDataset
  mmdet/datasets/samplers/group_sampler.py:10-48  GroupSampler
  mmdet/core/evaluation/{mean_ap,recall}.py through ``evaluate``

The inputs are the seeded fixture tree of tests/_dataset_fixture.py, written to
a temporary directory; only what the reference returns is stored.  Stubs that
live here, not in ref_shim: ``mmcv.load`` / ``mmcv.list_from_file`` (restated
from mmcv's public behaviour), ``np.int`` (removed from numpy 2, custom.py:140
uses it), NumPy 1's object array for the ragged list of recall.py:102, a
serial worker pool and silent summary tables (terminaltables is absent).
The reference's CocoDataset needs pycocotools and is not run.

Stored per run ``R`` (``_dataset_fixture.dataset_kwargs``):``R_len``, ``R_ids`` (the kept image ids or
filenames), ``R_width`` / ``R_height``, ``R_flag`` (train mode), per index i
``R_{i}_{bboxes,labels,bboxes_ignore,labels_ignore}`` and ``R_{i}_cat_ids``;
``eval_*_keys`` / ``eval_*_vals`` for the evaluate calls; ``sampler_*``.
"""
import json
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'oracle'))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)

import gen_golden as G  # noqa: E402,F401  (installs ref_shim)

import _dataset_fixture as FX  # noqa: E402


class _SerialPool:
    def __init__(self, nproc=1):
        pass

    def starmap(self, fn, args):
        return [fn(*a) for a in args]

    def close(self):
        pass


class _RaggedNumpy:
    """numpy as recall.py sees it, with NumPy 1's ``np.array`` of a ragged
    list: an object array (recall.py:102 relies on it; NumPy 2 raises)."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def array(obj, *args, **kw):
        try:
            return np.array(obj, *args, **kw)
        except ValueError:
            out = np.empty(len(obj), dtype=object)
            for i, o in enumerate(obj):
                out[i] = o
            return out


def _mmcv_load(path):
    if path.endswith('.json'):
        with open(path) as f:
            return json.load(f)
    with open(path, 'rb') as f:
        return pickle.load(f)


def _mmcv_list_from_file(path):
    with open(path, 'r', encoding='utf-8') as f:
        return [line.rstrip('\n\r') for line in f]


def record(d, run, ds, train):
    d[f'{run}_len'] = np.array(len(ds), np.int64)
    infos = ds.data_infos
    d[f'{run}_ids'] = np.array([i.get('id', i['filename']) for i in infos])
    d[f'{run}_filename'] = np.array([i['filename'] for i in infos])
    d[f'{run}_width'] = np.array([i['width'] for i in infos], np.int64)
    d[f'{run}_height'] = np.array([i['height'] for i in infos], np.int64)
    if train:
        d[f'{run}_flag'] = np.asarray(ds.flag)
    for i in range(len(ds)):
        ann = ds.get_ann_info(i)
        for k in ('bboxes', 'labels', 'bboxes_ignore', 'labels_ignore'):
            d[f'{run}_{i}_{k}'] = np.asarray(ann[k])
        d[f'{run}_{i}_cat_ids'] = np.asarray(ds.get_cat_ids(i), np.int64)


def record_eval(d, name, res):
    d[f'eval_{name}_keys'] = np.array(list(res.keys()))
    d[f'eval_{name}_vals'] = np.array([float(v) for v in res.values()],
                                      np.float64)
    print(f'[datasets] eval {name}:', dict(res), flush=True)


def main():
    np.int = int  # custom.py:140
    import mmcv
    mmcv.load = _mmcv_load
    mmcv.list_from_file = _mmcv_list_from_file
    from mmdet.core.evaluation import mean_ap as MA
    from mmdet.core.evaluation import recall as RC
    MA.Pool = _SerialPool
    MA.print_map_summary = lambda *a, **k: None
    RC.print_recall_summary = lambda *a, **k: None
    RC.np = _RaggedNumpy()
    from mmdet import datasets as RD
    from mmdet.datasets.samplers import GroupSampler

    d = {}
    with tempfile.TemporaryDirectory() as root:
        FX.write_fixture(root)
        built = {}
        for run, (typ, kw) in FX.dataset_kwargs(root).items():
            ds = getattr(RD, typ)(**kw)
            built[run] = ds
            record(d, run, ds, not kw.get('test_mode', False))
            print(f'[datasets] {run}: {len(ds)} images', flush=True)
        assert built['voc_train'].year == 2007
        # wrappers
        rep = RD.RepeatDataset(built['voc_train'], 3)
        d['repeat_len'] = np.array(len(rep), np.int64)
        d['repeat_flag'] = np.asarray(rep.flag)
        d['repeat_cat_ids'] = np.array(
            [json.dumps(rep.get_cat_ids(i)) for i in range(len(rep))])
        cat = RD.ConcatDataset([built['voc_train'], built['voc_minsize'],
                                built['xml_classes']])
        d['concat_len'] = np.array(len(cat), np.int64)
        d['concat_flag'] = np.asarray(cat.flag)
        d['concat_cumulative_sizes'] = np.asarray(cat.cumulative_sizes,
                                                  np.int64)
        d['concat_cat_ids'] = np.array(
            [json.dumps(cat.get_cat_ids(i)) for i in range(len(cat))])
        d['concat_cat_ids_neg'] = np.array(
            [json.dumps(cat.get_cat_ids(-i)) for i in range(1, len(cat) + 1)])
        # sampler order on the train flag, numpy's global RNG seeded
        for spg in (1, 2, 3):
            np.random.seed(5)
            d[f'sampler_{spg}'] = np.asarray(
                list(GroupSampler(built['voc_train'], spg)), np.int64)
        # evaluate on seeded results
        for run in ('voc_test', 'custom_test'):
            ds = built[run]
            res = FX.results_near_gt(ds)
            if run == 'voc_test':
                record_eval(d, 'voc_map', ds.evaluate(res, 'mAP'))
                record_eval(d, 'voc_map75', ds.evaluate(res, ['mAP'],
                                                        iou_thr=0.75))
            else:
                record_eval(d, 'custom_map', ds.evaluate(
                    res, 'mAP', iou_thr=[0.5, 0.7]))
            props = [np.concatenate(r) for r in res]
            record_eval(d, f'{run}_recall', ds.evaluate(
                props, 'recall', proposal_nums=(1, 3, 10),
                iou_thr=[0.5, 0.7]))
        record_eval(d, 'concat_map', RD.ConcatDataset(
            [built['voc_test'], built['custom_test']]).evaluate(
                FX.results_near_gt(built['voc_test']) +
                FX.results_near_gt(built['custom_test']), metric='mAP'))
    out = os.path.join(REPO, 'tests', 'golden', 'datasets.npz')
    np.savez_compressed(out, **d)
    print('[datasets] wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
