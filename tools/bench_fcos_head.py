"""Latency of the plain FCOS head's new launches against what existed before,
at 2 x 800 x 1344 with strides 8 .. 128 and 80 classes, timed with HIP events
(500 samples per side, the two sides ALTERNATING in one process, medians):

  * the FCOSHead loss-block call (LD_LOSS_DIST, 4 activated distances) against
    the FCOSGFLHead loss-block call (4 x 17 distribution logits) on the same
    targets;
  * ld_scale_act_levels forward / backward (exp) against ld_scale_levels
    forward / backward on the same (2, 4, P) box map.

Run on the MI355X:

    python tools/bench_fcos_head.py --out profiles/fcos_head_latency.json
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def alternate(fa, fb, samples=500, warm=20):
    """Median microseconds of fa and fb, one event pair per call, a / b / a /
    b ... so that clock and cache state drift hits both alike."""
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)]
          for _ in range(samples)]
    for e0, e1, e2 in ev:
        e0.record()
        fa()
        e1.record()
        fb()
        e2.record()
    torch.cuda.synchronize()
    ta = sorted(e0.elapsed_time(e1) for e0, e1, _ in ev)
    tb = sorted(e1.elapsed_time(e2) for _, e1, e2 in ev)

    def stats(t):
        return dict(median_us=round(t[len(t) // 2] * 1e3, 2),
                    p10_us=round(t[len(t) // 10] * 1e3, 2),
                    p90_us=round(t[len(t) * 9 // 10] * 1e3, 2))
    return stats(ta), stats(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=500)
    ap.add_argument('--out', required=True)
    args = ap.parse_args()
    from ld_amd import layers as Y, lib as L, lossblock as LB, synthetic as S
    dev = torch.device('cuda:0')
    pad, strides, C_ = (800, 1344), [8, 16, 32, 64, 128], 80
    batch = S.synthetic_batch(2, (800, 1333), pad, [7, 7], 1234)
    sizes = S.level_shapes(pad)
    hi = S.synthetic_head_inputs(2, sizes, seed=103)
    cls = [x.to(dev) for x in hi['cls']]
    reg68 = [x.to(dev) for x in hi['reg']]
    ctr = [x.to(dev) for x in S.synthetic_centerness(2, sizes, seed=103)]
    gen = torch.Generator().manual_seed(5)
    raw = [(torch.randn(2, 4, h, w, generator=gen) * 0.5).to(dev)
           for h, w in sizes]
    inf = 1e8
    targets = LB.fcos_targets(
        sizes, strides, [b.to(dev) for b in batch['gt_bboxes']],
        [l.to(dev) for l in batch['gt_labels']], C_,
        ((-1, 64), (64, 128), (128, 256), (256, 512), (512, inf)), True, 1.5,
        dev)
    base = L.LD_LOSS_ATSS | L.LD_LOSS_FCOS
    kw = dict(num_classes=C_, lw_ctr=1.0, lw_dfl=0.0, lw_ld=0.0, lw_ld_vlr=0.0,
              lw_kd=0.0, lw_im=0.0, T_ld=1.0, T_ld_vlr=1.0, T_kd=1.0,
              lw_bbox=1.0, feat_channels=C_)
    hp_gfl = LB.make_hp(flags=base, bbox_loss='giou', **kw)
    hp_dist = LB.make_hp(flags=base | L.LD_LOSS_DIST, bbox_loss='giou', **kw)
    dist = [(r.exp() * 4.0) for r in raw]
    feats = [c.detach() for c in cls]

    def block_gfl():
        LB.loss_block_forward(hp_gfl, targets, cls, reg68, cls, reg68, feats,
                              feats, ctr=ctr)

    def block_dist():
        LB.loss_block_forward(hp_dist, targets, cls, dist, cls, dist, feats,
                              feats, ctr=ctr)
    d_dist, d_gfl = alternate(block_dist, block_gfl, args.samples)
    # the activation launch against the Scale launch
    x3, levels = Y.pack_levels(raw)
    scales = torch.tensor([1.0, 0.75, 1.25, 0.5, 1.5], device=dev)
    dy = torch.randn(x3.shape, generator=gen).to(dev)

    def fwd_act():
        Y.scale_act_levels(x3, scales, levels, 'exp', strides)

    def fwd_scale():
        Y.scale_levels(x3, scales, levels)
    f_act, f_scale = alternate(fwd_act, fwd_scale, args.samples)
    xa = x3.clone().requires_grad_(True)
    sa = scales.clone().requires_grad_(True)
    ya = Y.scale_act_levels(xa, sa, levels, 'exp', strides)
    ys = Y.scale_levels(xa, sa, levels)

    def bwd_act():
        torch.autograd.grad(ya, (xa, sa), dy, retain_graph=True)

    def bwd_scale():
        torch.autograd.grad(ys, (xa, sa), dy, retain_graph=True)
    b_act, b_scale = alternate(bwd_act, bwd_scale, args.samples)

    def ratio(a, b):
        return round(a['median_us'] / b['median_us'], 3)
    out = dict(
        shape='2 x 800 x 1344, strides 8..128, 80 classes, center_sampling',
        samples=args.samples, method='HIP events, the two sides alternating',
        device=torch.cuda.get_device_name(0),
        loss_block=dict(fcos_head_dist=d_dist, fcos_gfl_head=d_gfl,
                        ratio=ratio(d_dist, d_gfl)),
        activation_forward=dict(scale_act_exp=f_act, scale=f_scale,
                                ratio=ratio(f_act, f_scale)),
        activation_backward=dict(scale_act_exp=b_act, scale=b_scale,
                                 ratio=ratio(b_act, b_scale)))
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
