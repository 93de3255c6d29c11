"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/eval_map.npz by EXECUTING THE
REFERENCE's mAP evaluation on CPU (the reference package is imported,
unmodified, through oracle/ref_shim.py).  Run from the repo root in the build
container, never on the GPU machine:

    python tools/gen_golden_evalmap.py

Reference entry points exercised (file:line under the reference tree):
  mmdet/core/evaluation/mean_ap.py:153-237  tpfp_default (per image, per class)
  mmdet/core/evaluation/mean_ap.py:240-264  get_cls_results
  mmdet/core/evaluation/mean_ap.py:267-402  eval_map (nproc=1)
  mmdet/core/evaluation/mean_ap.py:12-55    average_precision (through eval_map)

Inputs are regenerated from ld_amd.synthetic.EVAL_CASES (seeds); only the
reference outputs are stored.  ``print_map_summary`` is stubbed (terminaltables
is absent) and the worker pool runs in-process (same calls, in order).

Stored per run ``{case}_{dataset or 'area'}_{int(iou_thr * 100)}``:
  tp, fp      (S, total) uint8: tpfp_default of every (class, image) slice,
              class-major, image order inside a class (np.hstack order)
  num_gts     (C, S) int64;  num_dets (C,) int64
  recall      (S, total) float64, precision (S, total) float32: class-major
  ap          (C, S) float32;  mean_ap (S,) float64
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'oracle'))
sys.path.insert(0, REPO)

import gen_golden as G  # noqa: E402,F401  (installs ref_shim)

from ld_amd import synthetic  # noqa: E402


class _SerialPool:
    def __init__(self, nproc=1):
        pass

    def starmap(self, fn, args):
        return [fn(*a) for a in args]

    def close(self):
        pass


def run_tag(case_name, dataset, iou_thr):
    return f'{case_name}_{dataset or "area"}_{int(round(iou_thr * 100))}'


def main():
    from mmdet.core.evaluation import mean_ap as MA
    MA.Pool = _SerialPool
    MA.print_map_summary = lambda *a, **k: None
    d = {}
    for case in synthetic.EVAL_CASES:
        name, C, scale_ranges = case[0], case[3], case[4]
        det_results, annotations = synthetic.eval_map_inputs(case)
        S = 1 if scale_ranges is None else len(scale_ranges)
        area_ranges = (None if scale_ranges is None else
                       [(rg[0]**2, rg[1]**2) for rg in scale_ranges])
        for dataset, iou_thr in synthetic.EVAL_RUNS[name]:
            tag = run_tag(name, dataset, iou_thr)
            tps, fps = [], []
            for c in range(C):
                dets, gts, igs = MA.get_cls_results(det_results, annotations, c)
                for dt, gt, ig in zip(dets, gts, igs):
                    tp, fp = MA.tpfp_default(dt, gt, ig, iou_thr, area_ranges)
                    tps.append(tp)
                    fps.append(fp)
            d[f'{tag}_tp'] = np.hstack(tps).astype(np.uint8)
            d[f'{tag}_fp'] = np.hstack(fps).astype(np.uint8)
            mean_ap, res = MA.eval_map(det_results, annotations,
                                       scale_ranges=scale_ranges,
                                       iou_thr=iou_thr, dataset=dataset,
                                       nproc=1)
            d[f'{tag}_num_gts'] = np.array(
                [np.atleast_1d(r['num_gts']) for r in res], np.int64)
            d[f'{tag}_num_dets'] = np.array([r['num_dets'] for r in res],
                                            np.int64)
            d[f'{tag}_recall'] = np.hstack(
                [np.atleast_2d(r['recall']).reshape(S, -1) for r in res])
            d[f'{tag}_precision'] = np.hstack(
                [np.atleast_2d(r['precision']).reshape(S, -1) for r in res])
            d[f'{tag}_ap'] = np.array([np.atleast_1d(r['ap']) for r in res],
                                      np.float32)
            d[f'{tag}_mean_ap'] = np.atleast_1d(np.array(mean_ap, np.float64))
            assert d[f'{tag}_recall'].dtype == np.float64
            assert d[f'{tag}_precision'].dtype == np.float32
            print(f'[eval_map] {tag}: dets {d[f"{tag}_num_dets"].sum()}, '
                  f'gts {d[f"{tag}_num_gts"].sum(0).tolist()}, mAP '
                  f'{d[f"{tag}_mean_ap"].tolist()}', flush=True)
    np.savez_compressed(os.path.join(REPO, 'tests', 'golden', 'eval_map.npz'),
                        **d)


if __name__ == '__main__':
    main()
