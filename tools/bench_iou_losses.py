"""Latency of the positives kernel (loss_pos_kernel) and of the whole fused
loss block at the C2 size (2 x 800 x 1344, the `c2` loss-block case) for each
box loss, with the timing method of tools/bench_kernels.py (median of CUDA-event
intervals).  Run on the MI355X:

    python tools/bench_iou_losses.py --tag this --losses giou,ciou --out FILE

``--repo`` points at another checkout (with its library built) to time that
tree instead, e.g. the parent commit with ``--losses giou``; results of several
invocations are merged into FILE under ``tag``.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

MODES = {'giou': 0, 'iou': 1, 'iou_linear': 2, 'diou': 3, 'ciou': 4}


def timeit(fn, warm=5, iters=30):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True),
            torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in evs)
    return ts[len(ts) // 2] * 1e3  # median microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repo', default=os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    ap.add_argument('--tag', required=True)
    ap.add_argument('--losses', default='giou,ciou')
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', required=True)
    args = ap.parse_args()
    sys.path.insert(0, args.repo)
    from ld_amd import lib as L, lossblock as LB, synthetic
    dev = torch.device('cuda:0')
    pad, img_shape, num_gt = (800, 1344), (800, 1333), [7, 7]
    batch = synthetic.synthetic_batch(2, img_shape, pad, num_gt, 1234)
    sizes = synthetic.level_shapes(pad)
    hi = synthetic.synthetic_head_inputs(2, sizes, seed=103)
    d = {k: [x.to(dev) for x in v] for k, v in hi.items()}
    lib = L.get_lib()
    res = {}
    for name in args.losses.split(','):
        hp = LB.make_hp()
        hp.flags |= MODES[name] << 8  # the box-loss field of ld_loss_hp_t.flags
        t = LB.atss_targets(sizes, [8, 16, 32, 64, 128], batch['img_metas'],
                            [b.to(dev) for b in batch['gt_bboxes']],
                            [l.to(dev) for l in batch['gt_labels']], hp, dev)

        def block():
            return LB.loss_block_forward(hp, t, d['cls'], d['reg'], d['t_cls'],
                                         d['t_reg'], d['x'], d['t_x'])

        losses, grads, norm, aux = block()
        geom = t['geom']
        maps = {k: L.make_maps(v) for k, v in d.items()}
        gm = {k: L.make_maps(grads[k]) for k in ('cls', 'reg', 'x')}
        ws = LB.workspace(dev, lib.ld_loss_workspace_bytes(C.byref(geom)),
                          'loss')
        st = L.stream_ptr(dev)

        def pos():  # LD_LOSS_PART_POS = 1: loss_pos_kernel alone
            L.check(lib.ld_loss_main_parts(
                C.byref(geom), C.byref(hp), C.byref(maps['cls']),
                C.byref(maps['reg']), C.byref(maps['t_cls']),
                C.byref(maps['t_reg']), C.byref(maps['x']),
                C.byref(maps['t_x']), L.ptr(t['labels']),
                L.ptr(t['label_weights']), L.ptr(t['bbox_targets']),
                L.ptr(t['vlr']), L.ptr(t['im']), L.ptr(t['counts']),
                L.ptr(aux['weight_targets']), L.ptr(aux['score']), L.ptr(norm),
                None, C.byref(gm['cls']), C.byref(gm['reg']), C.byref(gm['x']),
                None, None, None, L.ptr(ws), ws.numel(), 1, st), 'pos')

        res[name] = dict(
            loss_bbox=[round(float(v), 6) for v in losses[1]],
            loss_pos_kernel_us=[round(timeit(pos), 2)
                                for _ in range(args.runs)],
            loss_block_us=[round(timeit(block), 2) for _ in range(args.runs)])
        print(args.tag, name, res[name], flush=True)
    out = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            out = json.load(f)
    out[args.tag] = res
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
