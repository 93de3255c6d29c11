"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/analyze_results.npz by
EXECUTING THE REFERENCE's per-image mAP on CPU (the reference package is
imported, unmodified, through oracle/ref_shim.py).  Run from the repo root in
the build container, never on the GPU machine:

    python tools/gen_golden_analyze_results.py

Reference entry points exercised (file:line under the reference tree):
  tools/analysis_tools/analyze_results.py:13-45   bbox_map_eval
  tools/analysis_tools/analyze_results.py:107-129 topk clamp, sort, good / bad
  mmdet/core/evaluation/mean_ap.py:267-402        eval_map (through it, and
                                                  directly for ap / mean_ap)

Route taken: the reference's own ``bbox_map_eval`` is loaded from its file.
What the top of that file imports and this interpreter lacks (mmcv, the
matplotlib behind mmdet.core.visualization) is fabricated by ref_shim; if that
import fails the script falls back to calling ``eval_map`` ten times per image
exactly as lines 38-45 do, and prints which route it took (stored as
``route``).  ``print_map_summary`` is stubbed and the worker pool runs
in-process, as in tools/gen_golden_evalmap.py.

Inputs are regenerated from ld_amd.synthetic.image_map_cases() (seeds); only
reference outputs are stored, per case:
  map      (I,) float64       bbox_map_eval of every image
  mean_ap  (I, T) float64     eval_map's mean_ap at each threshold
  ap       (I, T, C) float32  eval_map's per-class ap
  has_gt   (I, C) uint8       num_gts > 0
  good3 / bad3 / goodall / badall   index lists for topk = 3 and topk = I
  valid    (I, T, C) uint8    0 where equal scores make the reference's answer
                              depend on the order np.argsort leaves open
plus ``numpy_version``.

Tie cap: no (image, class) of any case but 'exact' may hold two equal scores
(asserted).  In 'exact' a class with equal scores is evaluated in both orders
and its cells are valid only where the reference agrees with itself; the
excluded share is printed and may not exceed 10 %.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'oracle'))
sys.path.insert(0, REPO)

import gen_golden as G  # noqa: E402,F401  (installs ref_shim)
import ref_shim  # noqa: E402

from ld_amd import synthetic  # noqa: E402


class _SerialPool:
    def __init__(self, nproc=1):
        pass

    def starmap(self, fn, args):
        return [fn(*a) for a in args]

    def close(self):
        pass


def _load_bbox_map_eval(MA):
    path = os.path.join(ref_shim.REFERENCE_ROOT, 'tools', 'analysis_tools',
                        'analyze_results.py')
    try:
        spec = importlib.util.spec_from_file_location('_ref_analyze', path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.eval_map = MA.eval_map  # the patched module's function, same code
        return mod.bbox_map_eval, 'reference bbox_map_eval'
    except Exception as e:  # noqa: BLE001
        print(f'[analyze_results] cannot import the reference tool ({e!r}); '
              'calling eval_map as its lines 38-45 do', flush=True)

        def bbox_map_eval(det_result, annotation):
            bbox = [det_result[0]] if isinstance(det_result, tuple) else \
                [det_result]
            iou_thrs = np.linspace(
                .5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
            mean_aps = []
            for thr in iou_thrs:
                mean_ap, _ = MA.eval_map(bbox, [annotation], iou_thr=thr,
                                         logger='silent')
                mean_aps.append(mean_ap)
            return sum(mean_aps) / len(mean_aps)
        return bbox_map_eval, 'eval_map x 10 per image'


def _rank(maps, topk):
    """analyze_results.py:107-129 on the reference's scores."""
    if (topk * 2) > len(maps):
        topk = len(maps) // 2
    _mAPs = dict(enumerate(maps))
    _mAPs = list(sorted(_mAPs.items(), key=lambda kv: kv[1]))
    return ([i for i, _ in _mAPs[-topk:]], [i for i, _ in _mAPs[:topk]])


def main():
    from mmdet.core.evaluation import mean_ap as MA
    MA.Pool = _SerialPool
    MA.print_map_summary = lambda *a, **k: None
    bbox_map_eval, route = _load_bbox_map_eval(MA)
    print(f'[analyze_results] route: {route}; numpy {np.__version__}',
          flush=True)
    thrs = np.linspace(
        .5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
    d = {'numpy_version': np.array(np.__version__), 'route': np.array(route)}

    def per_class(res, ann):
        ap = np.zeros((len(thrs), len(res)), np.float32)
        mean = np.zeros(len(thrs), np.float64)
        for t, thr in enumerate(thrs):
            mean[t], r = MA.eval_map([res], [ann], iou_thr=thr,
                                     logger='silent')
            ap[t] = [x['ap'] for x in r]
            ng = np.array([x['num_gts'] for x in r])
        return ap, mean, (ng > 0).astype(np.uint8)

    for case in synthetic.image_map_cases():
        name = case[0]
        results, anns, C = synthetic.image_map_inputs(case)
        I = len(results)
        maps = np.zeros(I, np.float64)
        mean_ap = np.zeros((I, len(thrs)), np.float64)
        ap = np.zeros((I, len(thrs), C), np.float32)
        has_gt = np.zeros((I, C), np.uint8)
        valid = np.ones((I, len(thrs), C), np.uint8)
        for i, (res, ann) in enumerate(zip(results, anns)):
            maps[i] = bbox_map_eval(res, ann)
            ap[i], mean_ap[i], has_gt[i] = per_class(res, ann)
            assert maps[i] == sum(mean_ap[i].tolist()) / len(thrs)
            tied = [c for c in range(C)
                    if len(np.unique(res[c][:, 4])) != len(res[c])]
            assert not tied or name == 'exact', (name, i, tied)
            if tied:  # both orders of the class arrays that hold ties
                flipped = [r[::-1].copy() if c in tied else r
                           for c, r in enumerate(res)]
                ap2, _, _ = per_class(flipped, ann)
                valid[i] = (ap2.view(np.uint32) == ap[i].view(np.uint32))
        excluded = 1.0 - valid.mean()
        assert excluded == 0 or name == 'exact'
        assert excluded <= 0.10, (name, excluded)
        d[f'{name}_map'], d[f'{name}_mean_ap'] = maps, mean_ap
        d[f'{name}_ap'], d[f'{name}_has_gt'] = ap, has_gt
        d[f'{name}_valid'] = valid
        for tag, k in (('3', 3), ('all', I)):
            good, bad = _rank(maps.tolist(), k)
            d[f'{name}_good{tag}'] = np.array(good, np.int64)
            d[f'{name}_bad{tag}'] = np.array(bad, np.int64)
        print(f'[analyze_results] {name}: {I} images, mean mAP '
              f'{maps.mean():.4f}, distinct {len(np.unique(maps))}, max '
              f'classes with GT {int(has_gt.sum(1).max())}, excluded cells '
              f'{100 * excluded:.2f} %', flush=True)
    out = os.path.join(REPO, 'tests', 'golden', 'analyze_results.npz')
    np.savez_compressed(out, **d)
    print(f'[analyze_results] wrote {out} ({os.path.getsize(out)} bytes)')


if __name__ == '__main__':
    main()
