"""Rank the images of a test set by their own mAP and save the best and the
worst: the reference's tools/analysis_tools/analyze_results.py on the device
(ld_amd.analyze_results).

    python tools/analyze_results.py results.pkl annotations.pkl show_dir \\
        [--topk 20] [--show-score-thr 0] [--img-dir DIR]

results.pkl: the list a test run dumps -- per image a list of per-class (k, 5)
arrays, or a (bbox, segm) tuple.  annotations.pkl: per image a dict of
``bboxes`` / ``labels`` (optional ``bboxes_ignore`` / ``labels_ignore``, and
``filename`` when --img-dir is given).  Writes show_dir/ranking.json: every
image's index and mAP, and the good / bad lists.
"""
import argparse
import json
import os
import os.path as osp
import pickle
import sys

import numpy as np

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))


def parse_args():
    ap = argparse.ArgumentParser(
        description='Per-image mAP ranking of a results file')
    ap.add_argument('results', help='pickled detection results')
    ap.add_argument('annotations', help='pickled list of annotation dicts')
    ap.add_argument('show_dir', help='directory for ranking.json, good/, bad/')
    ap.add_argument('--topk', type=int, default=20,
                    help='number of best and of worst images to list')
    ap.add_argument('--show-score-thr', type=float, default=0,
                    help='lowest detection score to draw')
    ap.add_argument(
        '--img-dir',
        help='also write good/ and bad/ images with GT and detection boxes '
        'drawn.  Images are read from DIR as raw .npy uint8 HWC arrays named '
        'after the annotation\'s "filename" with the extension replaced by '
        '.npy: this repository has no JPEG decoder.  Output is PNG; class '
        'names and scores are not drawn.')
    return ap.parse_args()


def save_images(pairs, out_dir, results, anns, img_dir, score_thr):
    from ld_amd import analyze_results as A
    os.makedirs(out_dir, exist_ok=True)
    for index, mAP in pairs:
        fname, ext = osp.splitext(osp.basename(anns[index]['filename']))
        img = np.load(osp.join(img_dir, fname + '.npy'))
        res = results[index]
        res = res[0] if isinstance(res, tuple) else res
        dets = np.concatenate([np.asarray(r, np.float32).reshape(-1, 5)
                               for r in res])
        out = A.draw_gt_det_bboxes(img, anns[index]['bboxes'], dets,
                                   score_thr=score_thr)
        # analyze_results.py:76-78; the pixels are PNG whatever ext says
        A.write_png(osp.join(out_dir, f'{fname}_{round(mAP, 3)}{ext}'), out)


def main():
    a = parse_args()
    from ld_amd import analyze_results as A
    with open(a.results, 'rb') as f:
        results = pickle.load(f)
    with open(a.annotations, 'rb') as f:
        anns = pickle.load(f)
    assert a.topk > 0 and len(results) == len(anns) > 0
    first = results[0][0] if isinstance(results[0], tuple) else results[0]
    acc = A.ImageMapAnalyzer(len(first))
    for i in range(0, len(results), 512):
        acc.add_results(results[i:i + 512], anns[i:i + 512])
    good, bad = acc.topk(a.topk)
    maps = acc.compute()[0].cpu().tolist()
    os.makedirs(a.show_dir, exist_ok=True)
    with open(osp.join(a.show_dir, 'ranking.json'), 'w') as f:
        json.dump(dict(
            images=[dict(index=i, mAP=m) for i, m in enumerate(maps)],
            good=[dict(index=i, mAP=m) for i, m in good],
            bad=[dict(index=i, mAP=m) for i, m in bad]), f, indent=1)
    if a.img_dir:
        for name, pairs in (('good', good), ('bad', bad)):
            save_images(pairs, osp.join(a.show_dir, name), results, anns,
                        a.img_dir, a.show_score_thr)
    print(f'{len(maps)} images, mean per-image mAP '
          f'{sum(maps) / len(maps):.4f}; wrote '
          f'{osp.join(a.show_dir, "ranking.json")}')


if __name__ == '__main__':
    main()
