"""Time RecallAccumulator (ld_eval_recalls_match per batch + ld_eval_recalls_count
once) at val2017 size on one GPU, next to a numpy restatement of the
reference's eval_recalls / _recalls on the host (one core) on a subset of the
same images.

    python tools/bench_recall.py [--batch 512] [--repeats 5] \\
        [--host-imgs 100] [--out profiles/recall_latency.json]

Input: 5000 images x 1000 scored proposals, 1-13 (about 7) GTs per image,
budgets (100, 300, 1000), 10 IoU thresholds, seeded
(ld_amd.synthetic.recall_scale_inputs), already on the device as a test loop
holds them after get_bboxes.  Three clocks, each the median of --repeats runs
after one warm-up run:
  match_kernel_ms  HIP events (torch.cuda.Event) recorded directly before and
                   after each ld_eval_recalls_match launch, summed over the
                   launches: the kernel's device time
  add_span_ms      HIP events around ALL ``add`` calls: includes the host
                   packing (torch.cat, offset uploads) that paces the loop
  *_wall_ms        perf_counter with a synchronize on both sides
The host time of the whole set is EXTRAPOLATED from the subset (labelled so in
the output).
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


def host_gt_ious(gts, props, nums):
    """recall.py:16-33, 88-101 restated in numpy for one image: descending
    score order (scores are distinct), the cap, fp32 IoU, greedy matching
    -> (P, G) float32."""
    p = props[np.argsort(props[:, 4])[::-1]][:nums[-1], :4]
    area_g = (gts[:, 2] - gts[:, 0]) * (gts[:, 3] - gts[:, 1])
    area_p = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    w = np.maximum(np.minimum(gts[:, None, 2], p[None, :, 2]) -
                   np.maximum(gts[:, None, 0], p[None, :, 0]), 0)
    h = np.maximum(np.minimum(gts[:, None, 3], p[None, :, 3]) -
                   np.maximum(gts[:, None, 1], p[None, :, 1]), 0)
    ov = w * h
    all_ious = ov / np.maximum(area_g[:, None] + area_p[None, :] - ov,
                               np.float32(1e-6))
    out = np.zeros((len(nums), len(gts)), np.float32)
    for k, num in enumerate(nums):
        ious = all_ious[:, :num].copy()
        if ious.size == 0:
            continue
        for j in range(ious.shape[0]):
            arg = ious.argmax(axis=1)
            mx = ious[np.arange(ious.shape[0]), arg]
            g = mx.argmax()
            out[k, j] = mx[g]
            ious[g, :] = -1
            ious[:, arg[g]] = -1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--imgs', type=int, default=5000)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host-imgs', type=int, default=100)
    ap.add_argument('--out')
    a = ap.parse_args()
    from ld_amd import synthetic
    from ld_amd.recall import RecallAccumulator
    dev = torch.device('cuda:0')
    nums, thrs = (100, 300, 1000), np.linspace(.5, 0.95, 10)
    s = synthetic.recall_scale_inputs(num_imgs=a.imgs, props_per_img=1000)
    B, off = s['proposals'].shape[0], s['gt_off']
    props = list(torch.from_numpy(s['proposals']).to(dev))
    gts_all = torch.from_numpy(s['gts']).to(dev)
    gts = [gts_all[off[k]:off[k + 1]] for k in range(B)]

    from ld_amd import lib as L
    lib = L.get_lib()
    match, spans = lib.ld_eval_recalls_match, []

    def timed_match(*args):  # events directly around the launch
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        rc = match(*args)
        e[1].record()
        spans.append(e)
        return rc

    lib.ld_eval_recalls_match = timed_match

    def run(no_lds=False):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        del spans[:]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc = RecallAccumulator(nums, thrs, device=dev)
        acc._no_lds = no_lds
        ev[0].record()
        for i in range(0, B, a.batch):
            acc.add(props[i:i + a.batch], gts[i:i + a.batch])
        ev[1].record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ev[2].record()
        rec = acc.compute()
        ev[3].record()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3]),
                (t1 - t0) * 1e3, (t2 - t1) * 1e3, acc, rec,
                sum(e[0].elapsed_time(e[1]) for e in spans), len(spans))

    run()
    runs = [run() for _ in range(a.repeats)]
    ws_runs = [run(no_lds=True) for _ in range(max(1, a.repeats // 2))]
    med = lambda k, rs=runs: round(statistics.median(r[k] for r in rs), 3)  # noqa: E731,E501
    acc, rec = runs[0][4], runs[0][5]
    out = dict(
        what='RecallAccumulator add + compute, val2017 size',
        num_imgs=B, props_per_img=1000, num_gts=int(off[-1]),
        proposal_nums=list(nums), num_thrs=len(thrs), add_batch=a.batch,
        repeats=a.repeats, device=torch.cuda.get_device_name(0),
        timing='HIP events directly around each match launch, summed '
               '(match_kernel_ms); HIP events around all add calls, host '
               'packing included (add_span_ms); events around compute '
               '(compute_device_ms); perf_counter around synchronize '
               '(wall_ms); median after one warm-up run',
        match_launches=runs[0][7], match_kernel_ms=med(6),
        match_kernel_ms_workspace_route=med(6, ws_runs),
        add_span_ms=med(0), compute_device_ms=med(1), add_wall_ms=med(2),
        compute_wall_ms=med(3),
        routes_bitwise_equal=bool(torch.equal(acc.gt_ious(),
                                              ws_runs[0][4].gt_ious())),
        recalls_at_1000=[round(float(x), 4) for x in rec[-1]],
        status='measured once')
    if a.host_imgs > 0:
        n = min(a.host_imgs, B)
        t0 = time.perf_counter()
        host = [host_gt_ious(s['gts'][off[k]:off[k + 1]], s['proposals'][k],
                             nums) for k in range(n)]
        ms = (time.perf_counter() - t0) * 1e3
        out['host_restatement'] = 'tools/bench_recall.py host_gt_ious ' \
            '(numpy, vectorised IoU, the reference\'s greedy loop), one core'
        out['host_subset_imgs'] = n
        out['host_subset_ms'] = round(ms, 1)
        out['host_full_ms_extrapolated'] = round(ms * B / n, 1)
        out['host_full_is'] = 'extrapolated from the subset, not measured'
        out['subset_bitwise_equal'] = bool(np.array_equal(
            np.concatenate(host, 1),
            acc.gt_ious()[:, :off[n]].cpu().numpy()))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
