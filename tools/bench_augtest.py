"""Latency of test-time-augmentation post-processing at 1333x800 with 2 and 4
views (one image): (a) the merge-NMS launch sequence alone (ld_aug_merge_nms
via lossblock.aug_merge_nms), (b) the head's whole aug_test post-processing
(per-view get_bboxes(with_nms=False) + the merge-NMS; the head forward is a
lookup of precomputed maps), (c) a torch restatement of merge_aug_bboxes +
multiclass_nms on the same device (map back, cat, threshold, sort, class-shift,
greedy suppression one kept box at a time: torch has no NMS op of its own).
Wall time of whole calls, median of 15 after 3 warm-ups.  Prints one line
per case; ``--out FILE`` also writes the results as JSON."""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from ld_amd import lossblock as LB, model_zoo, synthetic  # noqa: E402
from ld_amd.config import ConfigDict  # noqa: E402
from ld_amd.registry import build_head  # noqa: E402

dev = torch.device('cuda:0')
SCORE_THR, IOU_THR, MAX_PER_IMG = 0.05, 0.6, 100
# a 1333x800 picture at scale 1.0 and at 0.5 (img_scale (1333, 800) / (666, 400))
BIG = ((800, 1344), (800, 1333, 3), 1.0, False, None)
SMALL = ((416, 672), (400, 666, 3), 0.4996, False, None)
CASES = [
    ('v2_1333x800', 'gfl', [BIG, BIG[:3] + (True, 'horizontal')], 81, 1000,
     1.25, -1.0, 'nms', False),
    ('v4_1333x800', 'gfl', [BIG, BIG[:3] + (True, 'horizontal'), SMALL,
                            SMALL[:3] + (True, 'horizontal')], 82, 1000,
     1.25, -1.0, 'nms', False),
]


def timed(fn, reps=15):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2] * 1e3


def torch_merge_nms(views, C):
    """merge_aug_bboxes + multiclass_nms (type 'nms') in plain torch ops."""
    boxes, scores = [], []
    for v in views:
        b = v['boxes']
        if v['flip']:
            w = float(v['img_shape'][1])
            b = torch.stack([w - b[:, 2], b[:, 1], w - b[:, 0], b[:, 3]], 1)
        boxes.append(b / torch.as_tensor(v['scale_factor'], device=b.device))
        scores.append(v['scores'][:, :C])
    boxes, scores = torch.cat(boxes), torch.cat(scores)
    valid = scores > SCORE_THR
    idx = valid.nonzero()
    s, lab, bx = scores[valid], idx[:, 1], boxes[idx[:, 0]]
    order = s.argsort(descending=True)
    s, lab, bx = s[order], lab[order], bx[order]
    sb = bx + (lab.float() * (bx.max() + 1))[:, None]
    area = (sb[:, 2] - sb[:, 0]) * (sb[:, 3] - sb[:, 1])
    alive = torch.ones(s.shape[0], dtype=torch.bool, device=s.device)
    keep = []
    while len(keep) < MAX_PER_IMG:
        nz = alive.nonzero()
        if nz.shape[0] == 0:
            break
        i = int(nz[0, 0])
        keep.append(i)
        lt = torch.maximum(sb[i, :2], sb[:, :2])
        rb = torch.minimum(sb[i, 2:], sb[:, 2:])
        wh = (rb - lt).clamp(min=0)
        inter = wh[:, 0] * wh[:, 1]
        alive &= inter / (area[i] + area - inter) <= IOU_THR
        alive[i] = False
    k = torch.as_tensor(keep, device=s.device, dtype=torch.long)
    return torch.cat([bx[k], s[k, None]], 1), lab[k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='write the results as JSON to this file')
    args = ap.parse_args()
    out = dict(device=torch.cuda.get_device_name(0), time=time.time(),
               note='wall ms per call (one image), median of 15', cases=[])
    hc = dict(model_zoo.gfl_detector(50)['bbox_head'])
    for case in CASES:
        head = build_head(dict(hc, test_cfg=ConfigDict.wrap(dict(
            nms_pre=case[4], min_bbox_size=0, score_thr=SCORE_THR,
            nms=dict(type='nms', iou_threshold=IOU_THR),
            max_per_img=MAX_PER_IMG)))).to(dev).eval()
        outs = [synthetic.aug_view_outs(case, v, device=dev)
                for v in range(len(case[2]))]
        metas = synthetic.aug_view_metas(case)
        views = []
        for o, m in zip(outs, metas):
            b, s = head.get_bboxes(*o, m, with_nms=False)[0]
            views.append(dict(boxes=b, scores=s, **m[0]))
        head.forward = lambda v: outs[v]
        rows = sum(int(v['boxes'].shape[0]) for v in views)
        cand = int(sum(int((v['scores'][:, :80] > SCORE_THR).sum())
                       for v in views))
        merge_ms = timed(lambda: LB.aug_merge_nms(
            views, SCORE_THR, IOU_THR, MAX_PER_IMG, num_classes=80))
        post_ms = timed(lambda: head.aug_test(list(range(len(views))), metas))
        torch_ms = timed(lambda: torch_merge_nms(views, 80), reps=5)
        d, l_ = LB.aug_merge_nms(views, SCORE_THR, IOU_THR, MAX_PER_IMG,
                                 rescale=True, num_classes=80)
        td, tl = torch_merge_nms(views, 80)
        same = bool(d.shape == td.shape and torch.equal(l_, tl) and
                    (d - td).abs().max().item() <= 1e-3)
        out['cases'].append(dict(
            case=case[0], views=len(views), merged_rows=rows,
            candidates=cand, merge_nms_ms=merge_ms, aug_test_post_ms=post_ms,
            torch_restatement_ms=torch_ms, dets=int(d.shape[0]),
            torch_restatement_same_dets=same))
        print(out['cases'][-1], flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
