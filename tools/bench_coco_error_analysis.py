"""Time CocoErrorAnalysis (ld_coco_match_errors per batch +
ld_coco_accumulate once) at COCO val2017 size on one GPU, measured once.

    python tools/bench_coco_error_analysis.py [--batch 8] [--out x.json]

Workload: tools/bench_coco_eval.py's (5000 images, 80 categories, 100
detections per image, ~7.3 GTs per image) plus a seeded map of the 80
categories onto 12 supercategories.  Timed as bench_coco_eval.py times
CocoEvaluator: once, no warm-up, torch.cuda.synchronize() around ``add`` and
``compute``; the GT upload separately.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--out')
    a = ap.parse_args()
    from bench_coco_eval import workload
    from ld_amd import coco_analysis as CA, coco_eval as CE
    dev = torch.device('cuda:0')
    w = workload()
    B, K = len(w['img_ids']), len(w['cat_ids'])
    sup = np.random.RandomState(12).randint(0, 12, size=K)
    gt = CE.CocoGroundTruth(w['img_ids'], w['cat_ids'],
                            [str(c) for c in w['cat_ids']], w['gimg'],
                            w['gcat'], w['boxes'], w['areas'], w['crowd'],
                            w['ids'], [f's{s}' for s in sup])
    dets = list(torch.from_numpy(w['dets']).to(dev))
    labels = list(torch.from_numpy(w['labels']).to(dev))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ea = CA.CocoErrorAnalysis(gt, dev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for i in range(0, B, a.batch):
        j = min(B, i + a.batch)
        ea.add(range(i, j), dets[i:j], labels[i:j])
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    out = ea.compute()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    allc = out['aps']['allclass']['allarea']
    res = dict(
        what='CocoErrorAnalysis add + compute, COCO val2017 size, measured '
        'once',
        num_imgs=B, num_cats=K, num_supercategories=int(len(set(sup))),
        dets_per_img=int(w['dets'].shape[1]),
        num_dets=int(w['dets'].shape[0] * w['dets'].shape[1]),
        num_gts=int(len(w['ids'])), add_batch=a.batch,
        device=torch.cuda.get_device_name(0),
        gt_upload_ms=round((t1 - t0) * 1e3, 3),
        add_ms=round((t2 - t1) * 1e3, 3), compute_ms=round((t3 - t2) * 1e3, 3),
        total_ms=round((t3 - t1) * 1e3, 3),
        allclass_allarea={k: float(v) for k, v in allc.items()})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
