#!/usr/bin/env python
"""Latency of the input launch with augmentations (``ld_preprocess_batch_aug``,
csrc/pipeline.hip) next to ``ld_preprocess_batch`` at the same output size, in
one process.

Two cases, each a batch of two 480 x 640 uint8 images already on the device:
    plain_800x1344   Resize(1333, 800) -> Pad(32): out 2 x 3 x 800 x 1344.  The
                     new entry point gets the identity descriptors (no canvas,
                     full window, no crop), so both calls compute the same
                     bits -- checked before timing.
    crop_640x640     out 2 x 3 x 640 x 640.  New: Expand canvas, a window, the
                     resize, a 640 x 640 crop, a flip.  Old: a plain resize to
                     640 x 640, the launch a user had before at that size.
HIP events around each call, the two calls in alternating rounds so drift of
the machine falls on both; medians.  Bytes are what the launch must move: 3 B
read and 12 B written per output pixel (15 B; the four bilinear taps of
neighbouring pixels overlap, and a downscale reads more source than that, so
the figure is a floor on the traffic and the GB/s a floor on the rate).  No
bar is set on the ratio.

    python tools/bench_augment.py --out profiles/augment_latency.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # B/s, MI355X HBM3E
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


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
    for _ in range(warmup):
        fn1()
        fn2()
    torch.cuda.synchronize()
    t1, t2 = [], []
    for _ in range(rounds):
        t1 += _times_ms(fn1, iters)
        t2 += _times_ms(fn2, iters)
    return t1, t2


def _launchers(imgs, old_geo, new_plans, Hpad, Wpad, dev):
    """(old call, new call, old out, new out) on device-resident inputs: only
    the launches are timed, not the staging copies."""
    from ld_amd import lib as L
    from ld_amd.pipeline import DevicePipeline
    lib = L.get_lib()
    raw = [torch.from_numpy(im).to(dev) for im in imgs]
    N = len(imgs)
    d_old, d_new = (L.ImageT * N)(), (L.ImageAugT * N)()
    for i, im in enumerate(imgs):
        h, w = im.shape[:2]
        for d in (d_old[i], d_new[i]):
            d.data, d.src_h, d.src_w = raw[i].data_ptr(), h, w
        d_old[i].new_h, d_old[i].new_w, d_old[i].flip = old_geo[i]
        d_new[i].flip = int(new_plans[i]['flip'])
        DevicePipeline.fill_descriptor(d_new[i], new_plans[i], (h, w))
    dd = [torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8).to(dev)
          for d in (d_old, d_new)]
    outs = [torch.empty(N, 3, Hpad, Wpad, device=dev) for _ in range(2)]
    mean = (C.c_float * 3)(*MEAN)
    sinv = (C.c_float * 3)(*(1.0 / np.asarray(STD, np.float64)).astype(
        np.float32).tolist())
    pad = (C.c_float * 3)(0.0, 0.0, 0.0)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def old():
        L.check(lib.ld_preprocess_batch(dd[0].data_ptr(), N, Hpad, Wpad, mean,
                                        sinv, 1, outs[0].data_ptr(), stream),
                'ld_preprocess_batch')

    def new():
        L.check(lib.ld_preprocess_batch_aug(dd[1].data_ptr(), N, Hpad, Wpad,
                                            mean, sinv, pad, 1,
                                            outs[1].data_ptr(), stream),
                'ld_preprocess_batch_aug')
    return old, new, outs, (raw, dd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/augment_latency.json')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_augment needs the GPU: nothing is timed '
                         'without one')
    dev = torch.device('cuda:0')
    rs = np.random.RandomState(0)
    imgs = [rs.randint(0, 256, (480, 640, 3)).astype(np.uint8)
            for _ in range(2)]
    ident = dict(img_shape=(800, 1067, 3), flip=False)
    zoom = [dict(canvas=(960, 1280, 200, 300), fill=(103, 116, 123),
                 window=(100, 150, 700, 900), resized=(720, 926),
                 crop=(40, 143), img_shape=(640, 640, 3), flip=bool(i))
            for i in range(2)]
    cases = [
        ('plain_800x1344', [(800, 1067, 0)] * 2, [ident] * 2, 800, 1344, True),
        ('crop_640x640', [(640, 640, i) for i in range(2)], zoom, 640, 640,
         False),
    ]
    rows = []
    for name, old_geo, plans, Hp, Wp, same in cases:
        old, new, outs, keep = _launchers(imgs, old_geo, plans, Hp, Wp, dev)
        old()
        new()
        torch.cuda.synchronize()
        equal = bool(torch.equal(outs[0], outs[1]))
        if same and not equal:
            raise SystemExit(f'{name}: the identity descriptor does not give '
                             "ld_preprocess_batch's bits")
        t_old, t_new = _pair_ms(old, new, args.iters, args.warmup,
                                args.rounds)
        nbytes = 2 * Hp * Wp * 15
        row = dict(case=name, out_shape=[2, 3, Hp, Wp], bytes_floor=nbytes,
                   bit_identical=equal if same else None,
                   samples=len(t_old))
        for key, ts in (('ld_preprocess_batch', t_old),
                        ('ld_preprocess_batch_aug', t_new)):
            med = statistics.median(ts)
            q = statistics.quantiles(ts, n=10)
            row[key] = dict(median_us=round(med * 1e3, 2),
                            p10_us=round(q[0] * 1e3, 2),
                            p90_us=round(q[-1] * 1e3, 2),
                            gb_per_s=round(nbytes / (med * 1e-3) / 1e9, 1),
                            hbm_peak_fraction=round(
                                nbytes / (med * 1e-3) / HBM_PEAK, 4))
        row['ratio_new_over_old'] = round(
            row['ld_preprocess_batch_aug']['median_us'] /
            row['ld_preprocess_batch']['median_us'], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = dict(tool='tools/bench_augment.py',
               device=torch.cuda.get_device_name(0),
               timing='HIP events around each call, alternating rounds, '
                      'medians', iters=args.iters, rounds=args.rounds,
               warmup=args.warmup, bytes_per_output_pixel=15, cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
