"""Time the optimizer launch of the train step in three forms on the arena of
bench.py's detector (ld_r50_gflv1_r101_fpn_coco_1x student), on one GPU:

    plain            ld_sgd_step (the default trainer's launch)
    classes          ld_sgd_step_classes, the classes of
                     configs/ld/ld_r50_fcos_r101_1x.py's paramwise_cfg
                     (bias_lr_mult=2.0, bias_decay_mult=0.0)
    classes_norm     ld_grad_norm + ld_sgd_step_classes (grad_clip)

    python tools/bench_optim.py [--repeats 50] [--rounds 5] [--out x.json]

Each form is warmed up, then timed with HIP events around ``repeats``
back-to-back launches; the forms alternate for ``rounds`` rounds and the
median per-launch time is reported.  The entry points are called directly (no
weight-image refresh), so the times are the kernels'.  HBM bytes per element
are the algorithm's: read p, g, buf and write p, buf (20 B), + 1/64 B of class
id, + 4 B for the norm's read of g; the achieved bandwidth is bytes over the
measured time.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out')
    a = ap.parse_args()
    from ld_amd import lib as L
    from ld_amd import model_zoo
    from ld_amd.optim import build_optimizer
    from ld_amd.registry import build_detector
    from ld_amd.train import GradArena
    assert torch.cuda.is_available(), 'bench_optim needs the MI355X'
    dev = torch.device('cuda:0')
    lib = L.get_lib()
    det = build_detector(model_zoo.ld_detector(50, 101))
    det.to(dev)
    arena = GradArena(list(det.parameters()))
    pc = build_optimizer(det, dict(
        type='SGD', lr=0.01, momentum=0.9, weight_decay=1e-4,
        paramwise_cfg=dict(bias_lr_mult=2.0, bias_decay_mult=0.0)))['param_classes']
    n = arena.numel
    p = arena.flat_param
    g = torch.randn(n, device=dev) * 1e-3
    buf = torch.zeros(n, device=dev)
    ids = pc.chunk_ids(arena)
    ncls = len(pc)
    vals = [0.9, 1.0, 35.0, 0.0]
    for (lm, dm) in pc.classes:
        vals += [1e-6 * lm, 1e-4 * dm]
    hyper = torch.tensor(vals, dtype=torch.float32, device=dev)
    out = torch.zeros(2, device=dev)
    ws = torch.empty(lib.ld_grad_norm_workspace_bytes(), dtype=torch.uint8,
                     device=dev)
    s = L.stream_ptr(dev)
    P, G, B = C.c_void_p(p.data_ptr()), C.c_void_p(g.data_ptr()), \
        C.c_void_p(buf.data_ptr())

    def plain():
        L.check(lib.ld_sgd_step(P, G, B, n, 1e-6, 0.9, 1e-4, 1.0, s), 'sgd')

    def classes():
        L.check(lib.ld_sgd_step_classes(P, G, B, n, C.c_void_p(ids.data_ptr()),
                                        ncls, C.c_void_p(hyper.data_ptr()),
                                        None, s), 'sgd classes')

    def classes_norm():
        L.check(lib.ld_grad_norm(G, n, C.c_void_p(hyper.data_ptr()),
                                 C.c_void_p(out.data_ptr()),
                                 C.c_void_p(ws.data_ptr()), ws.numel(), s),
                'grad norm')
        L.check(lib.ld_sgd_step_classes(P, G, B, n, C.c_void_p(ids.data_ptr()),
                                        ncls, C.c_void_p(hyper.data_ptr()),
                                        C.c_void_p(out.data_ptr()), s),
                'sgd classes clip')

    forms = dict(plain=(plain, 20.0), classes=(classes, 20.0 + 1 / 64),
                 classes_norm=(classes_norm, 24.0 + 1 / 64))
    for fn, _ in forms.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, (fn, _) in forms.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.repeats):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.repeats)
    res = dict(what='optimizer launch on the bench detector arena, median of '
                    f'{a.rounds} rounds x {a.repeats} launches',
               device=torch.cuda.get_device_name(0), arena_floats=n,
               class_mults=[list(c) for c in pc.classes],
               chunks_per_class=[int((ids == k).sum()) for k in range(ncls)])
    for k, (_, bpe) in forms.items():
        us = statistics.median(times[k])
        res[k] = dict(us=round(us, 2), bytes_per_elem=round(bpe, 4),
                      gb_per_s=round(n * bpe / (us * 1e-6) / 1e9, 1),
                      rounds_us=[round(t, 2) for t in times[k]])
    res['cmd'] = 'python tools/bench_optim.py' + \
        (f' --out {a.out}' if a.out else '')
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
