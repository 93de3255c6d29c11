#!/usr/bin/env python
"""Latency of the deformable-convolution sampling kernels (csrc/dcn.hip) and what
a trainable R101-DCN backbone adds to the GFL train step.

Per layer (the three conv2 shapes of c3-c5 at 2 x 800x1344, batch 2): HIP-event
median of the forward im2col, the offset-gradient kernel, and the two data-
gradient passes (index = entry keys + radix sort + segment starts; sum = chunk
sums + fix-up), each with the bytes it must move -- Cin*k*k*Pout*4 B per image
for col / d_col -- and the fraction of the HBM peak that gives.

Whole step: the full-size GFL-R101-DCN train step next to the plain GFL-R101
step at the same shape (fp32, eager SGDTrainer steps); the difference is
reported, not judged.

    python tools/bench_dcn_backward.py --out profiles/dcn_backward_latency.json
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
    for cin, h, w in LAYERS:
        N, k, s, p = 2, 3, 1, 1
        g = torch.Generator().manual_seed(cin)
        x3 = torch.randn(N, cin, h * w, generator=g).to(dev)
        off3 = (torch.randn(N, 18, h * w, generator=g) * 1.5).to(dev)
        dcol = torch.randn(N, cin * 9, h * w, generator=g).to(dev)
        geo = (h, w, k, s, p)
        ws = Y.deform_col2im_index(off3, cin, *geo)
        col_bytes = N * cin * 9 * h * w * 4
        x_bytes = N * cin * h * w * 4
        entries = N * 9 * h * w * 4
        parts = dict(
            im2col=(lambda: Y.deform_im2col(x3, off3, h, w, k, s, p, 1),
                    col_bytes + x_bytes),
            offset_grad=(lambda: Y.deform_offset_grad(x3, off3, dcol, *geo),
                         col_bytes + x_bytes),
            data_grad_index=(lambda: Y.deform_col2im_index(off3, cin, *geo),
                             entries * 20),
            data_grad_sum=(lambda: Y.deform_col2im_sum(dcol, ws, cin, *geo),
                           col_bytes + x_bytes))
        row = dict(shape=f'N{N} C{cin} {h}x{w} k3 s1', col_bytes=col_bytes,
                   workspace_bytes=int(ws.numel()))
        for name, (fn, nbytes) in parts.items():
            ms = _median_ms(fn, iters, warmup)
            row[name] = dict(ms=round(ms, 4), bytes=nbytes,
                             hbm_fraction=round(nbytes / (ms * 1e-3) / HBM_PEAK, 4))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def bench_step(steps, warmup):
    from ld_amd import build_detector, model_zoo, synthetic
    from ld_amd.train import SGDTrainer
    dev = torch.device('cuda:0')
    b = synthetic.synthetic_batch(2, (800, 1333), (800, 1344), [8, 5], 21)
    d = dict(img=b['img'].to(dev), img_metas=b['img_metas'],
             gt_bboxes=[x.to(dev) for x in b['gt_bboxes']],
             gt_labels=[x.to(dev) for x in b['gt_labels']])
    out = {}
    for name, cfg in (('gfl_r101', model_zoo.gfl_detector(101)),
                      ('gfl_r101_dcn', model_zoo.gfl_dcn_detector(101))):
        det = build_detector(cfg)
        sd = synthetic.seeded_state_dict(det.state_dict(), seed=1)
        for k, v in sd.items():
            if k.endswith('conv_offset.bias'):
                v.fill_(0.6)  # offsets that matter: the sort sees real scatter
        det.load_state_dict(sd)
        det.to(dev).train()
        tr = SGDTrainer(det, lr=0.0025)
        ms = _median_ms(lambda: tr.step(d), steps, warmup)
        out[name] = dict(step_ms=round(ms, 3))
        print(name, out[name], flush=True)
        del tr, det
        torch.cuda.empty_cache()
    out['difference_ms'] = round(out['gfl_r101_dcn']['step_ms'] -
                                 out['gfl_r101']['step_ms'], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/dcn_backward_latency.json')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-step', action='store_true')
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), precision='fp32',
               hbm_peak_bytes_per_s=HBM_PEAK,
               layers=bench_layers(a.iters, a.warmup))
    if not a.no_step:
        res['train_step_2x800x1344'] = bench_step(a.steps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
