"""Time ImageMapAnalyzer (ld_eval_image_map per batch + ld_rank_images once) at
val2017 size on one GPU, next to the numpy restatement of bbox_map_eval on the
host (tests/_imagemap_oracle.py, one core) on a subset of the same images.

    python tools/bench_analyze_results.py [--batch 512] [--repeats 5] \\
        [--host-imgs 100] [--out profiles/analyze_results_latency.json]

Input: 5000 images x 100 detections, 80 classes, 1-14 GTs per image, seeded
(ld_amd.synthetic.eval_map_scale_inputs), already on the device as a test loop
holds them after get_bboxes.  Timed with torch.cuda.synchronize() around each
phase; the median of --repeats runs after one warm-up run.  The host time of
the whole set is EXTRAPOLATED from the subset (labelled so in the output).
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
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host-imgs', type=int, default=100)
    ap.add_argument('--topk', type=int, default=20)
    ap.add_argument('--out')
    a = ap.parse_args()
    from ld_amd import analyze_results as A
    from ld_amd import synthetic
    dev = torch.device('cuda:0')
    C = 80
    s = synthetic.eval_map_scale_inputs(num_imgs=5000, num_classes=C,
                                        dets_per_img=100, seed=41)
    B, off = s['dets'].shape[0], s['gt_off']
    dets = list(torch.from_numpy(s['dets']).to(dev))
    labels = list(torch.from_numpy(s['labels']).to(dev))
    gts_all = torch.from_numpy(s['gts']).to(dev)
    gl_all = torch.from_numpy(s['gt_labels']).to(dev)
    gts = [gts_all[off[k]:off[k + 1]] for k in range(B)]
    gl = [gl_all[off[k]:off[k + 1]] for k in range(B)]

    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc = A.ImageMapAnalyzer(C, device=dev)
        for i in range(0, B, a.batch):
            acc.add(dets[i:i + a.batch], labels[i:i + a.batch],
                    gts[i:i + a.batch], gl[i:i + a.batch])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        good, bad = acc.topk(a.topk)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, acc

    run()
    runs = [run() for _ in range(a.repeats)]
    add_ms = statistics.median(r[0] for r in runs)
    topk_ms = statistics.median(r[1] for r in runs)
    maps = runs[0][2].compute()[0].cpu().numpy()
    out = dict(
        what='ImageMapAnalyzer add + topk, val2017 size',
        num_imgs=B, num_classes=C, dets_per_img=100, num_thrs=10,
        add_batch=a.batch, repeats=a.repeats, topk=a.topk,
        device=torch.cuda.get_device_name(0),
        add_ms=round(add_ms, 3), topk_ms=round(topk_ms, 3),
        total_ms=round(add_ms + topk_ms, 3),
        mean_image_map=float(maps.mean()))
    if a.host_imgs > 0:
        import _imagemap_oracle as IO
        n = min(a.host_imgs, B)
        t0 = time.perf_counter()
        host = []
        for k in range(n):
            d, lab = s['dets'][k], s['labels'][k]
            host.append(IO.bbox_map_eval(
                [d[lab == c] for c in range(C)],
                dict(bboxes=s['gts'][off[k]:off[k + 1]],
                     labels=s['gt_labels'][off[k]:off[k + 1]])))
        ms = (time.perf_counter() - t0) * 1e3
        out['host_restatement'] = 'tests/_imagemap_oracle.py, one core'
        out['host_subset_imgs'] = n
        out['host_subset_ms'] = round(ms, 1)
        out['host_full_ms_extrapolated'] = round(ms * B / n, 1)
        out['host_full_is'] = 'extrapolated from the subset, not measured'
        out['subset_bitwise_equal'] = bool(
            np.array_equal(np.array(host), maps[:n]))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
