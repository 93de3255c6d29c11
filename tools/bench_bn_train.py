#!/usr/bin/env python
"""Latency of training-mode BatchNorm2d (csrc/nn.hip ld_bn_train_forward /
ld_bn_train_backward) at the conv-output shapes of ResNet-50 stages 2-4 for
2 x 800 x 1344 and 16 x 800 x 1344, with the eval-mode node (ld_bn_act_forward /
ld_bn_act_backward) timed at the same shape in the same session.

HIP-event medians, held against the algorithmic bytes per element:
  forward          12 = statistics read x (4) + apply read x, write y (8);
                   + 4 with a residual
  backward reduce  12 = read dy, y, x
  backward apply   16 = read dy, y, x, write dx; + 4 with dres
  eval forward      8 (+ 4 with a residual); eval backward 16 (+ 4 with dres)
The second read of a tensor that fits the 256 MB last-level cache may not come
from HBM: the figures are what the run shows, `tensor_mb` says which case a
row is.  Nothing is claimed that this tool has not measured.

    python tools/bench_bn_train.py --out profiles/bn_train_latency.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # B/s, MI355X HBM3E
# (name, C, H, W): the conv1 / conv2 and the conv3 outputs of R50 layer2-4
SHAPES = [('layer2.mid', 128, 100, 168), ('layer2.out', 512, 100, 168),
          ('layer3.mid', 256, 50, 84), ('layer3.out', 1024, 50, 84),
          ('layer4.mid', 512, 25, 42), ('layer4.out', 2048, 25, 42)]
BATCHES = (2, 16)
EPS, MOMENTUM = 1e-5, 0.1


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


def _entry(ms, elems, bytes_per_elem):
    bps = elems * bytes_per_elem / (ms * 1e-3)
    return dict(ms=round(ms, 4), bytes_per_elem=bytes_per_elem,
                gb_per_s=round(bps / 1e9, 1),
                hbm_fraction=round(bps / HBM_PEAK, 4))


def bench(iters, warmup):
    from ld_amd import layers as Y
    dev = torch.device('cuda:0')
    rows = []
    for N in BATCHES:
        for name, c, h, w in SHAPES:
            P = h * w
            elems = N * c * P
            x = torch.randn(N, c, P, device=dev)
            res = torch.randn(N, c, P, device=dev)
            dy = torch.randn(N, c, P, device=dev)
            gamma = torch.rand(c, device=dev) + 0.5
            beta = torch.randn(c, device=dev)
            rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
            nbt = torch.zeros((), dtype=torch.long, device=dev)
            params = (gamma, beta)
            y, scale, mean, rstd = Y._bn_train_forward(
                x, gamma, beta, rm, rv, nbt, EPS, MOMENTUM, res, True, True)
            ye, scale_e, rstd_e = Y._bn_act_forward(x, gamma, beta, rm, rv, EPS,
                                                    res, True)
            parts = {
                'train_forward': (12, lambda: Y._bn_train_forward(
                    x, gamma, beta, rm, rv, nbt, EPS, MOMENTUM, None, True,
                    True)),
                'train_forward_res': (16, lambda: Y._bn_train_forward(
                    x, gamma, beta, rm, rv, nbt, EPS, MOMENTUM, res, True,
                    True)),
                'train_backward_reduce': (12, lambda: Y._bn_train_backward(
                    dy, x, y, scale, mean, rstd, True, params, False, True,
                    True, False)),
                'train_backward': (28, lambda: Y._bn_train_backward(
                    dy, x, y, scale, mean, rstd, True, params, True, True,
                    True, False)),
                'train_backward_dres': (32, lambda: Y._bn_train_backward(
                    dy, x, y, scale, mean, rstd, True, params, True, True,
                    True, True)),
                'eval_forward': (8, lambda: Y._bn_act_forward(
                    x, gamma, beta, rm, rv, EPS, None, True)),
                'eval_forward_res': (12, lambda: Y._bn_act_forward(
                    x, gamma, beta, rm, rv, EPS, res, True)),
                'eval_backward': (16, lambda: Y._bn_act_backward(
                    dy, x, ye, scale_e, rm, rstd_e, True, params, True, True,
                    True, False)),
                'eval_backward_dres': (20, lambda: Y._bn_act_backward(
                    dy, x, ye, scale_e, rm, rstd_e, True, params, True, True,
                    True, True)),
            }
            row = dict(layer=name, shape=f'N{N} C{c} {h}x{w}', elements=elems,
                       tensor_mb=round(elems * 4 / 2 ** 20, 1))
            for part, (bpe, fn) in parts.items():
                row[part] = _entry(_median_ms(fn, iters, warmup), elems, bpe)
            row['train_over_eval_forward'] = round(
                row['train_forward_res']['ms'] / row['eval_forward_res']['ms'],
                3)
            row['train_over_eval_backward'] = round(
                row['train_backward_dres']['ms'] /
                row['eval_backward_dres']['ms'], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del x, res, dy, y, ye
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/bn_train_latency.json')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    from ld_amd import layers as Y
    Y.DIRECT_GRADS[0] = False  # fresh gradient tensors: no arena here
    res = dict(device=torch.cuda.get_device_name(0), precision='fp32',
               hbm_peak_bytes_per_s=HBM_PEAK, timing='HIP events, median of '
               f'{a.iters} after {a.warmup} warm-up calls, one process',
               rows=bench(a.iters, a.warmup))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
