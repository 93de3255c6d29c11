#!/usr/bin/env python
"""Latency of the trainable stem's two backward kernels and the price of the
trainable stem in a whole step, at the benchmark's 2 x 3 x 800 x 1344.

HIP-event medians.  What each figure is held against:
  * the small-Cin weight gradient (ld_conv_wgrad_smallc) against the generic
    ld_conv_wgrad on the same operands in the same process, and against its
    algorithmic bytes (dY + x, read once) at the HBM peak;
  * the max-pool backward against 9 bytes per input element (x and dx once,
    4 + 4, dy at a quarter of the positions, 1) next to the forward (5 bytes
    per input element) in the same session;
  * one GFL-R50 SGD step with frozen_stages=-1 against frozen_stages=0.

    python tools/bench_stem_backward.py --out profiles/stem_backward_latency.json
"""
import argparse
import copy
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # B/s, MI355X HBM3E
BATCH, H, W = 2, 800, 1344
# (name, Cin, k, stride, pad, Cout)
WGRADS = [('resnet stem 7x7', 3, 7, 2, 3, 64),
          ('res2net deep stem conv 0', 3, 3, 2, 1, 32)]


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


def bench_wgrad(iters, warmup):
    from ld_amd import layers as Y
    from ld_amd import lib as L
    lib, dev = L.get_lib(), torch.device('cuda:0')
    st = L.stream_ptr(dev)
    rows = []
    for name, cin, k, s, p, cout in WGRADS:
        g = torch.Generator().manual_seed(cin * k)
        d, out_lv = Y.conv_desc(BATCH, cin, cout, k, k, s, p, ((H, W), ))
        x = torch.randn(BATCH, cin, d.Pin, generator=g).to(dev)
        dy = torch.randn(BATCH, cout, d.Pout, generator=g).to(dev)
        dw = torch.empty(cout, cin, k, k, device=dev)
        dwg = torch.empty_like(dw)
        nbytes = 4 * (x.numel() + dy.numel())
        row = dict(layer=name, shape=f'N{BATCH} {cin}>{cout} {H}x{W} k{k} s{s}',
                   algorithmic_bytes=nbytes,
                   slabs=lib.ld_conv_wgrad_smallc_slabs(C.byref(d)))
        need = lib.ld_conv_wgrad_smallc_workspace_bytes(C.byref(d))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        job = L.WgradJobT()

        def flat():
            L.check(lib.ld_conv_wgrad_smallc(
                C.byref(d), L.ptr(x), L.ptr(dy), L.ptr(dw), 0, L.ptr(ws),
                need, st), 'ld_conv_wgrad_smallc')

        def slabs_only():
            L.check(lib.ld_conv_wgrad_smallc_partial(
                C.byref(d), L.ptr(x), L.ptr(dy), L.ptr(ws), need,
                C.byref(job), st), 'ld_conv_wgrad_smallc_partial')

        ms = _median_ms(flat, iters, warmup)
        row['smallc'] = dict(
            ms=round(ms, 4), slabs_only_ms=round(_median_ms(slabs_only, iters,
                                                            warmup), 4),
            bytes_per_s=round(nbytes / (ms * 1e-3), 1),
            hbm_fraction=round(nbytes / (ms * 1e-3) / HBM_PEAK, 4),
            ms_at_hbm_peak=round(nbytes / HBM_PEAK * 1e3, 4))
        gneed = lib.ld_conv_wgrad_workspace_bytes(C.byref(d))
        gws = torch.empty(max(gneed, 16), dtype=torch.uint8, device=dev)
        rc = lib.ld_conv_wgrad(C.byref(d), L.ptr(x), L.ptr(dy), L.ptr(dwg), 0,
                               L.ptr(gws), gneed, st)
        torch.cuda.synchronize()
        if rc == 0:
            gms = _median_ms(lambda: lib.ld_conv_wgrad(
                C.byref(d), L.ptr(x), L.ptr(dy), L.ptr(dwg), 0, L.ptr(gws),
                gneed, st), iters, warmup)
            flat()
            torch.cuda.synchronize()
            row['generic'] = dict(
                accepted=True, ms=round(gms, 4), workspace_bytes=gneed,
                max_abs_diff_over_max=float((dw - dwg).abs().max() /
                                            dwg.abs().max()))
            row['generic_over_smallc'] = round(gms / ms, 2)
        else:
            row['generic'] = dict(accepted=False, rc=rc)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def bench_pool(iters, warmup):
    from ld_amd import lib as L
    lib, dev = L.get_lib(), torch.device('cuda:0')
    st = L.stream_ptr(dev)
    rows, h, w = BATCH * 64, H // 2, W // 2  # the stem's output: 400 x 672
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    x = torch.relu(torch.randn(rows, h, w, device=dev))
    y = torch.empty(rows, ho, wo, device=dev)
    dy = torch.randn(rows, ho, wo, device=dev)
    dx = torch.empty_like(x)
    fwd = _median_ms(lambda: lib.ld_maxpool3x3s2(L.ptr(x), rows, h, w, L.ptr(y),
                                                 st), iters, warmup)
    bwd = _median_ms(lambda: lib.ld_maxpool_3x3s2_backward(
        L.ptr(x), L.ptr(dy), rows, h, w, L.ptr(dx), st), iters, warmup)
    n = x.numel()
    res = dict(shape=f'{rows} x {h} x {w}',
               forward=dict(ms=round(fwd, 4), bytes=5 * n,
                            gbytes_per_s=round(5 * n / (fwd * 1e-3) / 1e9, 1)),
               backward=dict(ms=round(bwd, 4), bytes=9 * n,
                             gbytes_per_s=round(9 * n / (bwd * 1e-3) / 1e9, 1)))
    print(json.dumps(res), flush=True)
    return res


def bench_step(iters, warmup):
    from ld_amd import model_zoo, synthetic
    from ld_amd.registry import build_detector
    from ld_amd.train import SGDTrainer
    dev = torch.device('cuda:0')
    b = synthetic.synthetic_batch(BATCH, (H, 1333), (H, W), [3, 2], 21)
    data = dict(img=b['img'].to(dev), img_metas=b['img_metas'],
                gt_bboxes=[t.to(dev) for t in b['gt_bboxes']],
                gt_labels=[t.to(dev) for t in b['gt_labels']])
    res = {}
    for frozen in (0, -1):
        cfg = copy.deepcopy(model_zoo.gfl_detector(50))
        cfg['backbone']['frozen_stages'] = frozen
        det = build_detector(cfg)
        det.load_state_dict(synthetic.seeded_state_dict(det.state_dict(),
                                                        seed=1))
        tr = SGDTrainer(det.to(dev).train(), lr=0.0025)
        res[f'frozen_stages={frozen}'] = dict(
            ms=round(_median_ms(lambda: tr.step(data), iters, warmup), 3))
        del tr, det
        torch.cuda.empty_cache()
    res['trainable_stem_ms'] = round(res['frozen_stages=-1']['ms'] -
                                     res['frozen_stages=0']['ms'], 3)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/stem_backward_latency.json')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_stem_backward.py measures on the GPU only')
    res = dict(device=torch.cuda.get_device_name(0), precision='fp32',
               input=f'{BATCH} x 3 x {H} x {W}', iters=a.iters,
               hbm_peak_bytes_per_s=HBM_PEAK,
               weight_gradient=bench_wgrad(a.iters, a.warmup),
               maxpool=bench_pool(a.iters, a.warmup),
               gfl_r50_step=bench_step(a.iters, a.warmup))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
