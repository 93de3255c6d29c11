#!/usr/bin/env python
"""Latency of the float-image input launch (``ld_preprocess_batch_photo``,
csrc/pipeline.hip) next to ``ld_preprocess_batch_aug`` at the same geometry,
in one process.

Each case is a batch of two 480 x 640 uint8 images already on the device:
    identity_800x1344   out 2 x 3 x 800 x 1344, identity geometry.  New:
                        float mode without the distortion (no chain, no HSV
                        round trip, the float resize).
    full_800x1344       the same geometry; new: the full chain with the HSV
                        step (brightness, contrast, saturation, hue,
                        permutation) on each of the four taps.
    full_320x320        out 2 x 3 x 320 x 320, the SSD / YOLO size: Expand
                        canvas, a window, Resize(keep_ratio=False), a flip;
                        new: the full chain.
The old call gets the same geometry with the uint8 fill.  HIP events around
each call, the two calls in alternating rounds so drift of the machine falls
on both; medians of 500 samples.  Bytes are what a launch must move: 3 B read
and 12 B written per output pixel (15 B, a floor on the traffic, so the GB/s
is a floor on the rate).  No bar is set on the ratio.

    python tools/bench_photometric.py --out profiles/photometric_latency.json
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
FULL = dict(delta=-12.5, mode=1, alpha=1.25, saturation=0.75, hue=11.0,
            perm=(2, 0, 1))


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


def _launchers(imgs, plans, Hpad, Wpad, dev):
    """(old call, new call, outs) on device-resident inputs: only the
    launches are timed, not the staging copies."""
    from ld_amd import lib as L
    from ld_amd.pipeline import DevicePipeline
    lib = L.get_lib()
    raw = [torch.from_numpy(im).to(dev) for im in imgs]
    N = len(imgs)
    d_old, d_new = (L.ImageAugT * N)(), (L.ImagePhotoT * N)()
    for i, im in enumerate(imgs):
        h, w = im.shape[:2]
        for d in (d_old[i], d_new[i]):
            d.data, d.src_h, d.src_w = raw[i].data_ptr(), h, w
            d.flip = int(plans[i]['flip'])
        DevicePipeline.fill_descriptor(d_old[i], plans[i], (h, w))
        DevicePipeline.fill_photo_descriptor(d_new[i], plans[i], (h, w))
    dd = [torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8).to(dev)
          for d in (d_old, d_new)]
    outs = [torch.empty(N, 3, Hpad, Wpad, device=dev) for _ in range(2)]
    mean = (C.c_float * 3)(*MEAN)
    sinv = (C.c_float * 3)(*(1.0 / np.asarray(STD, np.float64)).astype(
        np.float32).tolist())
    pad = (C.c_float * 3)(0.0, 0.0, 0.0)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(name, k):
        fn = getattr(lib, name)

        def run():
            L.check(fn(dd[k].data_ptr(), N, Hpad, Wpad, mean, sinv, pad, 1,
                       outs[k].data_ptr(), stream), name)
        return run
    return (call('ld_preprocess_batch_aug', 0),
            call('ld_preprocess_batch_photo', 1), outs, (raw, dd))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/photometric_latency.json')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_photometric needs the GPU: nothing is timed '
                         'without one')
    dev = torch.device('cuda:0')
    rs = np.random.RandomState(0)
    imgs = [rs.randint(0, 256, (480, 640, 3)).astype(np.uint8)
            for _ in range(2)]
    ident = dict(img_shape=(800, 1067, 3), flip=False)
    zoom = [dict(canvas=(960, 1280, 200, 300), fill=(103, 116, 123),
                 window=(100, 150, 700, 900), resized=(320, 320),
                 img_shape=(320, 320, 3), flip=bool(i)) for i in range(2)]
    cases = [
        ('identity_800x1344', [dict(ident, photo=None)] * 2, 800, 1344),
        ('full_800x1344', [dict(ident, photo=FULL)] * 2, 800, 1344),
        ('full_320x320', [dict(z, photo=FULL) for z in zoom], 320, 320),
    ]
    rows = []
    for name, plans, Hp, Wp in cases:
        old, new, outs, keep = _launchers(imgs, plans, Hp, Wp, dev)
        old()
        new()
        torch.cuda.synchronize()
        if not all(bool(torch.isfinite(o).all()) for o in outs):
            raise SystemExit(f'{name}: a launch wrote a non-finite value')
        # identity chain: the float resize stays within one 8-bit level of
        # the 8-bit one
        close = None
        if name.startswith('identity'):
            close = float((outs[0] - outs[1]).abs().max()) <= 1.0 / min(STD)
            if not close:
                raise SystemExit(f'{name}: float and 8-bit resize differ by '
                                 'more than one level')
        t_old, t_new = _pair_ms(old, new, args.iters, args.warmup,
                                args.rounds)
        nbytes = 2 * Hp * Wp * 15
        row = dict(case=name, out_shape=[2, 3, Hp, Wp], bytes_floor=nbytes,
                   within_one_level_of_8bit=close, samples=len(t_old))
        for key, ts in (('ld_preprocess_batch_aug', t_old),
                        ('ld_preprocess_batch_photo', t_new)):
            med = statistics.median(ts)
            q = statistics.quantiles(ts, n=10)
            row[key] = dict(median_us=round(med * 1e3, 2),
                            p10_us=round(q[0] * 1e3, 2),
                            p90_us=round(q[-1] * 1e3, 2),
                            gb_per_s=round(nbytes / (med * 1e-3) / 1e9, 1),
                            hbm_peak_fraction=round(
                                nbytes / (med * 1e-3) / HBM_PEAK, 4))
        row['ratio_new_over_old'] = round(
            row['ld_preprocess_batch_photo']['median_us'] /
            row['ld_preprocess_batch_aug']['median_us'], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = dict(tool='tools/bench_photometric.py',
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
