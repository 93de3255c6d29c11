#!/usr/bin/env python
"""Latency of the grouped-convolution kernels (csrc/gconv.hip): forward, data
gradient and weight gradient of the four conv2 shapes of ResNeXt-101 32x4d at
800x1344 (batch 2) and of the two grouped GEMMs behind the c4 / c5 grouped DCN.

HIP-event medians.  What each figure is held against: the stride-1 data
gradient moves the bytes and does the flops of the forward of the same shape,
so both and their ratio are recorded; the weight gradient makes one pass over x
and dy, recorded as achieved bytes/s against the HBM peak.

    python tools/bench_gconv_backward.py --out profiles/gconv_backward_latency.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # B/s, MI355X HBM3E
# (name, Cin, Cout, H, W, k, stride): conv2 of layer1-4 (the first block of
# layer2-4 strides), then the K = 1 GEMMs over the Cin*9 DCN columns
LAYERS = [('layer1.conv2', 128, 128, 200, 336, 3, 1),
          ('layer2.conv2', 256, 256, 100, 168, 3, 1),
          ('layer3.conv2', 512, 512, 50, 84, 3, 1),
          ('layer4.conv2', 1024, 1024, 25, 42, 3, 1),
          ('layer3.dcn_gemm', 512 * 9, 512, 50, 84, 1, 1),
          ('layer4.dcn_gemm', 1024 * 9, 1024, 25, 42, 1, 1)]
GROUPS, BATCH = 32, 2


def _median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def bench_layers(iters, warmup):
    from ld_amd import layers as Y
    dev = torch.device('cuda:0')
    rows = []
    for name, cin, cout, h, w, k, s in LAYERS:
        N, G, p = BATCH, GROUPS, k // 2
        g = torch.Generator().manual_seed(cin + k)
        ho, wo = Y.out_size(h, k, s, p), Y.out_size(w, k, s, p)
        x3 = torch.randn(N, cin, h * w, generator=g).to(dev)
        wt = (torch.randn(cout, cin // G, k, k, generator=g) * 0.05).to(dev)
        dy = torch.randn(N, cout, ho * wo, generator=g).to(dev)
        lv = ((h, w), )
        nbytes = 4 * N * (cin * h * w + cout * ho * wo)
        flops = 2 * N * cout * (cin // G) * k * k * ho * wo
        row = dict(layer=name, shape=f'N{N} {cin}>{cout} g{G} {h}x{w} k{k} s{s}',
                   bytes=nbytes, flops=flops)
        parts = dict(
            forward=lambda: Y.gconv_forward(x3, wt, G, s, p, lv),
            dgrad=lambda: Y.gconv_dgrad(dy, wt, G, s, p, lv, x3.shape),
            wgrad=lambda: Y.gconv_wgrad(x3, dy, wt, G, s, p, lv))
        for part, fn in parts.items():
            ms = _median_ms(fn, iters, warmup)
            row[part] = dict(ms=round(ms, 4),
                             bytes_per_s=round(nbytes / (ms * 1e-3), 1),
                             hbm_fraction=round(nbytes / (ms * 1e-3) / HBM_PEAK, 4),
                             tflops=round(flops / (ms * 1e-3) / 1e12, 3))
        row['dgrad_over_forward'] = round(row['dgrad']['ms'] /
                                          row['forward']['ms'], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/gconv_backward_latency.json')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), precision='fp32',
               hbm_peak_bytes_per_s=HBM_PEAK,
               layers=bench_layers(a.iters, a.warmup))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
