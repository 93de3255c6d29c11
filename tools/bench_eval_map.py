"""Time MapAccumulator (ld_eval_tpfp per batch + ld_eval_ap once) at VOC07-test
size on one GPU, next to the numpy restatement of the same evaluation on the
host (tests/_evalmap_oracle.py, one process).

    python tools/bench_eval_map.py [--batch 8] [--repeats 5] [--out x.json]

Input: ld_amd.synthetic.eval_map_scale_inputs() -- 4952 images x 100 detections
(20 classes) already on the device, as a test loop holds them after
get_bboxes; GTs on the device too.  Timed with torch.cuda.synchronize() around
each phase; the median of ``--repeats`` runs after one warm-up run.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out')
    a = ap.parse_args()
    from ld_amd import evaluation as E
    from ld_amd import synthetic
    dev = torch.device('cuda:0')
    s = synthetic.eval_map_scale_inputs()
    B, C = s['dets'].shape[0], 20
    off = s['gt_off']
    dets = list(torch.from_numpy(s['dets']).to(dev))
    labels = list(torch.from_numpy(s['labels']).to(dev))
    gts_all = torch.from_numpy(s['gts']).to(dev)
    gl_all = torch.from_numpy(s['gt_labels']).to(dev)
    gts = [gts_all[off[k]:off[k + 1]] for k in range(B)]
    gl = [gl_all[off[k]:off[k + 1]] for k in range(B)]

    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc = E.MapAccumulator(C, (0.5, ), device=dev)
        for i in range(0, B, a.batch):
            acc.add(dets[i:i + a.batch], labels[i:i + a.batch],
                    gts[i:i + a.batch], gl[i:i + a.batch])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        mean_ap, _ = acc.compute(logger='silent')[0]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, mean_ap

    run()
    runs = [run() for _ in range(a.repeats)]
    add_ms = statistics.median(r[0] for r in runs)
    compute_ms = statistics.median(r[1] for r in runs)
    out = dict(
        what='MapAccumulator add + compute, VOC07-test size',
        num_imgs=B, num_classes=C, dets_per_img=100,
        num_dets=int(B * 100), add_batch=a.batch, repeats=a.repeats,
        device=torch.cuda.get_device_name(0),
        add_ms=round(add_ms, 3), compute_ms=round(compute_ms, 3),
        total_ms=round(add_ms + compute_ms, 3), mean_ap=runs[0][2])
    if not a.no_host:
        import _evalmap_oracle as O
        det_results, anns = [], []
        for k in range(B):
            d, lab = s['dets'][k], s['labels'][k]
            det_results.append([d[lab == c] for c in range(C)])
            anns.append(dict(bboxes=s['gts'][off[k]:off[k + 1]],
                             labels=s['gt_labels'][off[k]:off[k + 1]]))
        t0 = time.perf_counter()
        m_host, _, _, _ = O.eval_map(det_results, anns, None, 0.5)
        out['host_restatement_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        out['host_restatement'] = 'tests/_evalmap_oracle.py, one process'
        out['host_cores_used'] = 1  # single-threaded Python / numpy loops
        out['host_mean_ap'] = m_host
        out['abs_diff_mean_ap'] = abs(m_host - runs[0][2])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
