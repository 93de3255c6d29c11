"""Time the AP landscape and the teacher-student discrepancy pass
(ld_amd.landscape, landscape.hip) on one GPU: a 5 x 5 grid and one discrepancy
pass on one 800 x 1344 image with the R50 <- R101 LD detector (seeded
weights), next to the per-point torch formulation on the same build.

    python tools/bench_landscape.py [--repeats 10] [--warmup 2] \\
        [--out profiles/landscape_latency.json]

Clocks: HIP events (torch.cuda.Event) around each piece, the median of
--repeats runs after --warmup runs.
  landscape_add_ms      FeatureLandscape.add of the 25 points: both backbones
                        and necks once, two mix launches (16 + 9 points), two
                        head forwards (batch 16 and 9), two get_bboxes, 25
                        evaluator adds
  two_backbones_ms      both extract_feat calls alone
  torch_point_tail_ms   ONE point the torch way with the features given:
                        a * x + b * y per level, the head, get_bboxes, the
                        evaluator add (simple_test's tail)
  torch_grid_ms_derived 25 * (two_backbones_ms + torch_point_tail_ms): the
                        reference re-runs the whole two-backbone test per
                        point; derived from the two medians, not timed
  mix_k16_ms / mix_k9_ms   one ld_levels_mix launch; GB/s over
                        (2 + K) * 4 B per element
  abs_err_*_ms          ld_levels_abs_err on features (C 256), cls (C 80),
                        bbox (C 68); GB/s over 2 * 4 B per element
  pearson_ms            ld_levels_pearson on the features; GB/s over the
                        2 * 4 B per element of ONE pass (the second pass
                        re-reads a segment the first just pulled in)
  discrepancy_kernels_ms   the four launch pairs of one pass together
  discrepancy_add_ms    TeacherStudentDiscrepancy.add: both models' forwards
                        included
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--grid', type=int, default=5)
    ap.add_argument('--out')
    a = ap.parse_args()
    from ld_amd import landscape as LS
    from ld_amd import model_zoo, synthetic
    from ld_amd.coco_eval import CocoEvaluator, CocoGroundTruth
    dev = torch.device('cuda:0')
    det = model_zoo.build_seeded_ld_detector(50, 101, dev)
    det.eval()
    teacher = det.teacher_model
    batch = synthetic.synthetic_batch(1, (800, 1333), (800, 1344), [7], 7)
    img, metas = batch['img'].to(dev), batch['img_metas']
    metas[0]['scale_factor'] = np.array([1.25] * 4, dtype=np.float32)
    head = det.bbox_head

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(max(a.repeats, 10)):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            e[0].record()
            fn()
            e[1].record()
            torch.cuda.synchronize()
            ms.append(e[0].elapsed_time(e[1]))
        return round(statistics.median(ms), 4)

    with torch.no_grad():
        xs, xt = det.extract_feat(img), teacher.extract_feat(img)
        outs_s, outs_t = head(xs), teacher.bbox_head(xt)
        plain = head.get_bboxes(*outs_s, metas, rescale=True)
    gt = CocoGroundTruth.from_annotations(
        [dict(bboxes=d[:5, :4].cpu().numpy(), labels=l[:5].cpu().numpy())
         for d, l in plain], num_classes=80)
    fac = lambda: CocoEvaluator(gt)  # noqa: E731
    vals = np.linspace(0.0, 1.0, a.grid).tolist()
    grid = LS.FeatureLandscape.grid(vals, vals)
    K = len(grid)

    def landscape_add():
        land = LS.FeatureLandscape(det, coefs=grid, evaluator_factory=fac)
        land.add(img, metas, gt=[0])
        return land

    def two_backbones():
        with torch.no_grad():
            det.extract_feat(img)
            teacher.extract_feat(img)

    def torch_point():
        ev = fac()
        with torch.no_grad():
            y = tuple(0.9 * p + 0.7 * q for p, q in zip(xs, xt))
            boxes = head.get_bboxes(*head(y), metas, rescale=True)
        ev.add([0], [d for d, _ in boxes], [l for _, l in boxes])

    own3, levels = LS._pack(tuple(xs), LS._levels_of(xs)), LS._levels_of(xs)
    other3 = LS._pack(tuple(xt), levels)
    fams = dict(feature=(own3, other3),
                cls=(LS._pack(tuple(outs_s[0]), levels),
                     LS._pack(tuple(outs_t[0]), levels)),
                bbox=(LS._pack(tuple(outs_s[1]), levels),
                      LS._pack(tuple(outs_t[1]), levels)))
    n = own3.numel()

    def kernels():
        for s3, t3 in fams.values():
            LS.levels_abs_err(t3, s3, levels)
        LS.levels_pearson(other3, own3, levels)

    def disc_add():
        acc = LS.TeacherStudentDiscrepancy(det)
        acc.add(img)

    out = dict(
        what=f'{a.grid} x {a.grid} AP landscape and one discrepancy pass, '
             '1 x 800 x 1344, R50 <- R101 LD detector, seeded weights',
        device=torch.cuda.get_device_name(0), grid_points=K,
        chunks=LS.FeatureLandscape.chunks(K, 1),
        packed_feature_MB=round(n * 4 / 1e6, 2), repeats=max(a.repeats, 10),
        warmup=a.warmup,
        timing='HIP events around each piece with a synchronize on both '
               'sides; median after the warm-up runs',
        landscape_add_ms=timed(landscape_add),
        two_backbones_ms=timed(two_backbones),
        torch_point_tail_ms=timed(torch_point))
    out['torch_grid_ms_derived'] = round(
        K * (out['two_backbones_ms'] + out['torch_point_tail_ms']), 2)
    out['torch_grid_is'] = 'derived from two medians, not timed'
    for k in sorted({min(16, K), max(1, K - 16)}, reverse=True):
        ms = timed(lambda: LS.mix_levels(own3, other3, grid[:k],
                                         levels=levels))
        out[f'mix_k{k}_ms'] = ms
        out[f'mix_k{k}_GBps'] = round((2 + k) * 4 * n / ms / 1e6, 1)
    out['mix_includes'] = 'the allocation of the (K, C, P) output'
    total = 0
    for fam, (s3, t3) in fams.items():
        ms = timed(lambda: LS.levels_abs_err(t3, s3, levels))
        nbytes = 2 * 4 * s3.numel()
        total += nbytes
        out[f'abs_err_{fam}_ms'] = ms
        out[f'abs_err_{fam}_GBps'] = round(nbytes / ms / 1e6, 1)
    ms = timed(lambda: LS.levels_pearson(other3, own3, levels))
    out['pearson_ms'] = ms
    out['pearson_GBps_one_pass'] = round(2 * 4 * n / ms / 1e6, 1)
    out['discrepancy_kernels_ms'] = timed(kernels)
    out['discrepancy_read_MB'] = round(total / 1e6, 1)
    out['discrepancy_add_ms'] = timed(disc_add)
    res = landscape_add().compute()
    out['ap_diagonal'] = [round(float(res[i, i]['stats'][0]), 4)
                          for i in range(a.grid)]
    out['status'] = 'measured once'
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
