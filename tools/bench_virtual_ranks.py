"""Time one virtual-rank optimizer step against the plain steps it stands for,
on one GPU:

    virtual   SGDTrainer(virtual_ranks=W).step(the W micro-batches)
    plain     W consecutive SGDTrainer.step calls on the same micro-batches
              (virtual_ranks=1: the path without virtual ranks)

    python tools/bench_virtual_ranks.py [--ranks 8] [--steps 5] [--warmup 2] \\
        [--precisions fp32 bf16] [--out profiles/virtual_ranks_latency.json]

Setup: the seeded R50 <- R101 LD detector of bench.py, W micro-batches of
2 x 800 x 1344 with 7 boxes per image, both forms in the same process.  Every
timed step (or group of W plain steps) is bracketed by device synchronisations;
the median of ``--steps`` after ``--warmup`` is reported, with
``torch.cuda.max_memory_allocated()`` of each form -- the virtual step keeps W
forward graphs alive until their backwards.

Expectation (reported, not asserted): the virtual step costs about W plain
steps minus W - 1 optimizer launches, i.e. a ratio slightly under 1; a ratio
well above 1 means something serialised that should not have.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def _batches(W, dev):
    from ld_amd import synthetic
    out = []
    for r in range(W):
        b = synthetic.synthetic_batch(2, (800, 1333), (800, 1344), [7, 7],
                                      100 + r)
        out.append(dict(img=b['img'].to(dev), img_metas=b['img_metas'],
                        gt_bboxes=[x.to(dev) for x in b['gt_bboxes']],
                        gt_labels=[x.to(dev) for x in b['gt_labels']]))
    return out


def _measure(step, warmup, steps, dev):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    times = []
    for _ in range(steps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize(dev)
        times.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(statistics.median(times), 3),
                all_ms=[round(t, 3) for t in times],
                max_memory_allocated_mib=round(
                    torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1))


def _one_precision(precision, W, a, dev):
    from ld_amd import layers as Y
    from ld_amd import model_zoo
    from ld_amd.train import SGDTrainer
    Y.set_precision(precision)
    batches = _batches(W, dev)
    kw = dict(lr=1e-6, momentum=0.9, weight_decay=1e-4)
    res = {}
    # plain first: its peak is measured before the virtual trainer's tables
    # and extra teacher slots exist
    det = model_zoo.build_seeded_ld_detector(50, 101, dev)
    plain = SGDTrainer(det, **kw)

    def plain_steps():
        for r in range(W):
            plain.step(batches[r], next_data=batches[(r + 1) % W])

    res['plain'] = _measure(plain_steps, a.warmup, a.steps, dev)
    del plain, det
    torch.cuda.empty_cache()
    det = model_zoo.build_seeded_ld_detector(50, 101, dev)
    virtual = SGDTrainer(det, virtual_ranks=W, **kw)
    res['virtual'] = _measure(
        lambda: virtual.step(batches, next_data=batches), a.warmup, a.steps,
        dev)
    res['teacher_slots'] = det.TEACHER_SLOTS
    del virtual, det
    torch.cuda.empty_cache()
    res['ratio_virtual_over_plain'] = round(
        res['virtual']['ms'] / res['plain']['ms'], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ranks', type=int, default=8)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--precisions', nargs='+', default=['fp32', 'bf16'])
    ap.add_argument('--out')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_virtual_ranks needs the MI355X'
    from ld_amd import layers as Y
    dev = torch.device('cuda:0')
    W = a.ranks
    res = dict(
        what=f'one virtual-rank step (W = {W}) against {W} consecutive plain '
             f'steps on the same micro-batches of 2 x 800 x 1344, R50 <- R101; '
             f'synchronised median of {a.steps} after {a.warmup} warm-up',
        device=torch.cuda.get_device_name(0), ranks=W)
    try:
        for precision in a.precisions:
            res[precision] = _one_precision(precision, W, a, dev)
    finally:
        Y.set_precision('fp32')
    res['cmd'] = 'python tools/bench_virtual_ranks.py' + \
        (f' --out {a.out}' if a.out else '')
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
