#!/usr/bin/env python
"""Latency of the Res2Net backbone (ld_amd/resnet.py Res2Net, csrc/res2net.hip)
at the benchmark size, batch 2 x 800 x 1344, fp32.  Record only: no threshold.

  * the Res2Net-101-DCN teacher backbone forward under no_grad
    (configs/imv2/gflv2_r2n101_dcn_fpn_2x.py), and the R101-DCN teacher backbone
    forward from the same session as a yardstick;
  * forward + backward of the trainable configuration (frozen_stages=1,
    norm_eval=True), ones as the cotangents of the four stage outputs;
  * every glue kernel at the shapes the four stages launch it with: time, the
    bytes it has to move (computed from the shapes below) and their rate as a
    fraction of the HBM peak -- all of them are pure copies / pools, bound by
    bandwidth;
  * the glue's share of the teacher forward: the per-kernel medians times the
    number of launches per stage, over the forward time (an estimate from
    isolated launches, named as such in the output).

HIP-event medians after a warm-up; a glue kernel is launched 20 times between
an event pair (back to back on one stream) and the time divided by 20.

    python tools/bench_res2net.py --out profiles/res2net_latency.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # B/s, MI355X HBM3E
BATCH, H, W = 2, 800, 1344
# stage: (width, blocks at depth 101, map entering the stage, stride)
STAGES = [(26, 3, (200, 336), 1), (52, 4, (200, 336), 2),
          (104, 23, (100, 168), 2), (208, 3, (50, 84), 2)]


def _median_ms(fn, iters, warmup, reps=1):
    """Median over ``iters`` event pairs of the time of one call; ``reps``
    calls go between a pair (an event pair around ONE launch of a few
    microseconds measures the launch gap, not the kernel)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    return statistics.median(ts)


GLUE_REPS = 20


def _backbone(cfg, dev, train):
    from ld_amd import synthetic
    from ld_amd.registry import build_backbone
    net = build_backbone(cfg)
    net.load_state_dict(synthetic.seeded_state_dict(net.state_dict(), seed=5))
    net.to(dev)
    return net.train() if train else net.eval()


def bench_backbones(iters, warmup):
    from ld_amd import model_zoo
    dev = torch.device('cuda:0')
    x = torch.randn(BATCH, 3, H, W,
                    generator=torch.Generator().manual_seed(1)).to(dev)
    out = {}

    def fwd(net):
        with torch.no_grad():
            return net(x)

    r101 = model_zoo.gfl_dcn_detector(101)['backbone']
    for name, cfg in (('res2net101_dcn', model_zoo._r2n_backbone(101, True)),
                      ('resnet101_dcn_c3_c5', r101)):
        net = _backbone(cfg, dev, False)
        out[name + '_teacher_forward_ms'] = round(
            _median_ms(lambda: fwd(net), iters, warmup), 3)
        del net
        torch.cuda.empty_cache()
    net = _backbone(model_zoo._r2n_backbone(101, True), dev, True)
    # stage 1 is frozen: its output carries no gradient
    cots = [torch.ones_like(o) for o in fwd(net)[1:]]

    def step():
        for p in net.parameters():
            p.grad = None
        torch.autograd.backward(net(x)[1:], cots)

    out['res2net101_dcn_train_forward_backward_ms'] = round(
        _median_ms(step, max(3, iters // 2), warmup), 3)
    return out


def _row(name, shape, nbytes, ms, launches):
    return dict(kernel=name, shape=shape, bytes=nbytes, ms=round(ms, 4),
                bytes_per_s=round(nbytes / (ms * 1e-3), 1),
                hbm_fraction=round(nbytes / (ms * 1e-3) / HBM_PEAK, 4),
                launches_per_forward=launches)


def bench_glue(iters, warmup):
    from ld_amd import layers as Y
    dev = torch.device('cuda:0')
    rows = []
    for w, blocks, (h, w_), s in STAGES:
        ho, wo = Y.out_size(h, 3, s, 1), Y.out_size(w_, 3, s, 1)
        P, Po = h * w_, ho * wo
        cin = {26: 64, 52: 256, 104: 512, 208: 1024}[w]  # entering the stage
        u_in = torch.randn(BATCH, 4 * w, P, device=dev)   # first block
        u = torch.randn(BATCH, 4 * w, Po, device=dev)     # the others
        sp = torch.randn(BATCH, w, Po, device=dev)
        st0 = Y.Res2State(w, (h, w_), s, s != 1)
        st = Y.Res2State(w, (ho, wo), 1, False)
        f4 = 4 * BATCH * w  # bytes per position of one width-w slice
        shape = f'N{BATCH} w{w} '
        rows.append(_row('gather', shape + f'{h}x{w_}', 2 * f4 * P,
                         _median_ms(lambda: Y.res2_gather(u_in, None, 1, st0),
                                    iters, warmup, GLUE_REPS), 3))
        rows.append(_row('gather_add', shape + f'{ho}x{wo}', 3 * f4 * Po,
                         _median_ms(lambda: Y.res2_gather(u, sp, 1, st),
                                    iters, warmup, GLUE_REPS),
                         2 * (blocks - 1)))
        rows.append(_row('gather', shape + f'{ho}x{wo}', 2 * f4 * Po,
                         _median_ms(lambda: Y.res2_gather(u, None, 0, st),
                                    iters, warmup, GLUE_REPS), blocks - 1))
        rows.append(_row('concat_pool' if s != 1 else 'concat',
                         shape + f'{h}x{w_} s{s}', f4 * (7 * Po + P),
                         _median_ms(lambda: Y.res2_concat([sp, sp, sp], u_in,
                                                          st0, False),
                                    iters, warmup, GLUE_REPS), 1))
        rows.append(_row('concat', shape + f'{ho}x{wo}', 8 * f4 * Po,
                         _median_ms(lambda: Y.res2_concat([sp, sp, sp], u, st,
                                                          True),
                                    iters, warmup, GLUE_REPS), blocks - 1))
        if s != 1:
            x = torch.randn(BATCH, cin, P, device=dev)
            rows.append(_row('shortcut_pool', f'N{BATCH} C{cin} {h}x{w_}',
                             4 * BATCH * cin * (P + Po),
                             _median_ms(lambda: Y.avgpool_ceil(x, (h, w_), s),
                                        iters, warmup, GLUE_REPS), 1))
        for r in rows[-6:]:
            print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/res2net_latency.json')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_res2net.py measures on the GPU only')
    glue = bench_glue(a.iters, a.warmup)
    nets = bench_backbones(a.iters, a.warmup)
    glue_ms = sum(r['ms'] * r['launches_per_forward'] for r in glue)
    res = dict(device=torch.cuda.get_device_name(0), precision='fp32',
               input=f'{BATCH}x3x{H}x{W}', hbm_peak_bytes_per_s=HBM_PEAK,
               backbones=nets, glue=glue,
               glue_forward_ms_estimate=round(glue_ms, 3),
               glue_share_of_teacher_forward_estimate=round(
                   glue_ms / nets['res2net101_dcn_teacher_forward_ms'], 4),
               note='glue share: isolated per-kernel medians x launches per '
                    'forward over the measured teacher forward')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(nets))
    print('wrote', a.out)


if __name__ == '__main__':
    main()
