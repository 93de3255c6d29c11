#!/usr/bin/env python
"""Latency of the modulated deformable-convolution (DCNv2) sampling kernels
(csrc/dcn.hip) next to the DCNv1 launches of the same shape, in one process.

Per layer (the three conv2 shapes of R101 c3-c5 at 2 x 800x1344, batch 2):
HIP-event median of
    im2col            ld_mdeform_im2col            vs ld_deform_im2col
    offset_mask_grad  ld_mdeform_offset_mask_grad  vs ld_deform_offset_grad
    data_grad_index   ld_mdeform_col2im_index      vs ld_deform_col2im_index
    data_grad         index + ld_deform_col2im_sum, both versions (the sum
                      kernel is the same code; only the stored weights differ)
The two versions of a part are timed in alternating rounds, so drift of the
machine falls on both.  Each row carries the bytes the part must move
(Cin*k*k*Pout*4 B per image for col / d_col, one more plane per tap for v2)
and the fraction of the HBM peak that gives.  The ratio v2 / v1 is reported,
not judged: no bar is set.

    python tools/bench_mdcn.py --out profiles/mdcn_latency.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # B/s, MI355X HBM3E
LAYERS = [(128, 100, 168), (256, 50, 84), (512, 25, 42)]


def _times_ms(fn, iters):
    ts = []
    for _ in range(iters):
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def _pair_ms(fn1, fn2, iters, warmup, rounds):
    """Medians of two callables timed in alternating rounds."""
    for _ in range(warmup):
        fn1()
        fn2()
    torch.cuda.synchronize()
    t1, t2 = [], []
    for _ in range(rounds):
        t1 += _times_ms(fn1, iters)
        t2 += _times_ms(fn2, iters)
    return statistics.median(t1), statistics.median(t2)


def bench_layers(iters, warmup, rounds):
    from ld_amd import layers as Y
    dev = torch.device('cuda:0')
    rows = []
    for cin, h, w in LAYERS:
        N, k, s, p = 2, 3, 1, 1
        g = torch.Generator().manual_seed(cin)
        x3 = torch.randn(N, cin, h * w, generator=g).to(dev)
        om3 = (torch.randn(N, 27, h * w, generator=g) * 1.5).to(dev)
        off3 = om3[:, :18].contiguous()  # v1 sees the same offsets
        dcol = torch.randn(N, cin * 9, h * w, generator=g).to(dev)
        geo = (h, w, k, s, p)
        ws1 = Y.deform_col2im_index(off3, cin, *geo)
        ws2 = Y.mdeform_col2im_index(om3, cin, *geo)
        plane = N * 9 * h * w * 4  # one fp32 plane per tap
        col_bytes = N * cin * 9 * h * w * 4
        x_bytes = N * cin * h * w * 4
        entries = N * 9 * h * w * 4
        parts = dict(
            im2col=(lambda: Y.deform_im2col(x3, off3, h, w, k, s, p, 1),
                    lambda: Y.mdeform_im2col(x3, om3, h, w, k, s, p, 1),
                    col_bytes + x_bytes + 2 * plane, plane),
            offset_mask_grad=(
                lambda: Y.deform_offset_grad(x3, off3, dcol, *geo),
                lambda: Y.mdeform_offset_mask_grad(x3, om3, dcol, *geo),
                col_bytes + x_bytes + 4 * plane, 2 * plane),
            data_grad_index=(
                lambda: Y.deform_col2im_index(off3, cin, *geo),
                lambda: Y.mdeform_col2im_index(om3, cin, *geo),
                entries * 20 + 2 * plane, plane),
            data_grad=(
                lambda: Y.deform_col2im_sum(
                    dcol, Y.deform_col2im_index(off3, cin, *geo), cin, *geo),
                lambda: Y.deform_col2im_sum(
                    dcol, Y.mdeform_col2im_index(om3, cin, *geo), cin, *geo),
                entries * 20 + 2 * plane + col_bytes + x_bytes, plane))
        assert ws1.numel() == ws2.numel()
        row = dict(shape=f'N{N} C{cin} {h}x{w} k3 s1', col_bytes=col_bytes,
                   workspace_bytes=int(ws2.numel()))
        for name, (f1, f2, bytes1, extra) in parts.items():
            ms1, ms2 = _pair_ms(f1, f2, iters, warmup, rounds)
            row[name] = dict(
                v1_ms=round(ms1, 4), v2_ms=round(ms2, 4),
                ratio_v2_over_v1=round(ms2 / ms1, 4),
                v1_bytes=bytes1, v2_bytes=bytes1 + extra,
                v1_hbm_fraction=round(bytes1 / (ms1 * 1e-3) / HBM_PEAK, 4),
                v2_hbm_fraction=round((bytes1 + extra) / (ms2 * 1e-3) /
                                      HBM_PEAK, 4))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/mdcn_latency.json')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mdcn: needs the MI355X (no CPU timing path)')
    res = dict(device=torch.cuda.get_device_name(0), precision='fp32',
               hbm_peak_bytes_per_s=HBM_PEAK, iters=a.iters, rounds=a.rounds,
               timing='HIP events around each call, median; v1 and v2 in '
                      'alternating rounds in one process',
               layers=bench_layers(a.iters, a.warmup, a.rounds))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
