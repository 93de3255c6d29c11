"""Time CocoEvaluator (ld_coco_match per batch + ld_coco_accumulate once) at
COCO val2017 size on one GPU, measured once.

    python tools/bench_coco_eval.py [--batch 8] [--out x.json]

Workload (seeded, ld_amd-independent numpy): 5000 images, 80 categories, 100
detections per image, ~7.3 GTs per image (Poisson), ~1% crowds, one category
(index 0, "person") holding ~30% of GTs and detections, as in val2017.  The
detections are already on the device, as a test loop holds them after
get_bboxes.  ``add`` and ``compute`` are timed with torch.cuda.synchronize()
around them, once (no warm-up, no repeats: what a user waits for after an
epoch); the GT upload is timed separately.  pycocotools cannot be timed here.
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


def workload(seed=2017, B=5000, K=80, dets_per_img=100):
    rng = np.random.RandomState(seed)
    img_ids = rng.choice(600000, B, replace=False)
    cat_ids = np.sort(rng.choice(np.arange(1, 91), K, replace=False))
    pick = lambda n: np.where(rng.uniform(size=n) < 0.3, 0,  # noqa: E731
                              rng.randint(1, K, size=n))
    ng = rng.poisson(7.3, size=B)
    G = int(ng.sum())
    gimg = np.repeat(np.arange(B), ng)
    gcat = pick(G)
    xy = rng.uniform(0, 560, size=(G, 2))
    wh = np.exp(rng.uniform(np.log(4), np.log(400), size=(G, 2)))
    boxes = np.concatenate([xy, wh], 1)
    areas = wh[:, 0] * wh[:, 1] * rng.uniform(0.4, 1.0, size=G)
    crowd = (rng.uniform(size=G) < 0.01).astype(np.int64)
    goff = np.concatenate([[0], np.cumsum(ng)])
    dets = np.zeros((B, dets_per_img, 5), np.float32)
    labels = np.zeros((B, dets_per_img), np.int64)
    for i in range(B):
        n_tp = min(int(ng[i]) * 4, 60)
        src = goff[i] + rng.randint(0, max(int(ng[i]), 1), size=n_tp)
        b = np.zeros((dets_per_img, 4))
        lab = pick(dets_per_img)
        if ng[i]:
            jit = rng.normal(0, 0.12, size=(n_tp, 4)) * np.concatenate(
                [wh[src], wh[src]], 1)
            b[:n_tp] = np.concatenate([xy[src], xy[src] + wh[src]], 1) + jit
            lab[:n_tp] = np.where(rng.uniform(size=n_tp) < 0.85, gcat[src],
                                  lab[:n_tp])
        else:
            n_tp = 0
        rxy = rng.uniform(0, 560, size=(dets_per_img - n_tp, 2))
        rwh = np.exp(rng.uniform(np.log(4), np.log(300),
                                 size=(dets_per_img - n_tp, 2)))
        b[n_tp:] = np.concatenate([rxy, rxy + rwh], 1)
        dets[i, :, :4] = b
        dets[i, :, 4] = rng.uniform(0.05, 1.0, size=dets_per_img)
        labels[i] = lab
    return dict(img_ids=img_ids, cat_ids=cat_ids, gimg=img_ids[gimg],
                gcat=cat_ids[gcat], boxes=boxes, areas=areas, crowd=crowd,
                ids=np.arange(1, G + 1), dets=dets, labels=labels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--out')
    a = ap.parse_args()
    from ld_amd import coco_eval as CE
    dev = torch.device('cuda:0')
    w = workload()
    B, K = len(w['img_ids']), len(w['cat_ids'])
    gt = CE.CocoGroundTruth(w['img_ids'], w['cat_ids'],
                            [str(c) for c in w['cat_ids']], w['gimg'],
                            w['gcat'], w['boxes'], w['areas'], w['crowd'],
                            w['ids'])
    dets = list(torch.from_numpy(w['dets']).to(dev))
    labels = list(torch.from_numpy(w['labels']).to(dev))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gt.to(dev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ev = CE.CocoEvaluator(gt, device=dev)
    for i in range(0, B, a.batch):
        j = min(B, i + a.batch)
        ev.add(range(i, j), dets[i:j], labels[i:j])
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    out = ev.compute()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    res = dict(
        what='CocoEvaluator add + compute, COCO val2017 size, measured once',
        num_imgs=B, num_cats=K, dets_per_img=int(w['dets'].shape[1]),
        num_dets=int(w['dets'].shape[0] * w['dets'].shape[1]),
        num_gts=int(len(w['ids'])), num_crowd=int(w['crowd'].sum()),
        largest_category_dets=int((w['labels'] == 0).sum()),
        add_batch=a.batch, device=torch.cuda.get_device_name(0),
        gt_upload_ms=round((t1 - t0) * 1e3, 3),
        add_ms=round((t2 - t1) * 1e3, 3), compute_ms=round((t3 - t2) * 1e3, 3),
        total_ms=round((t3 - t1) * 1e3, 3),
        stats=[float(x) for x in out['stats']])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
