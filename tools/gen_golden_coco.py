"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/coco_eval.npz from the numpy
restatement of pycocotools' COCOeval and of the reference's
CocoDataset.evaluate glue (tests/_cocoeval_oracle.py).  Run from the repo root
in the build container:

    python tools/gen_golden_coco.py

pycocotools cannot be installed where this project is built, so COCOeval's
arithmetic (IoU, the greedy match, accumulate, summarize) is pinned ONLY by the
restatement and by the hand-derived known answers of
tests/test_coco_eval_host.py -- not by pycocotools itself.  This file freezes
the restatement's outputs so that the device path is held to them bit for bit.

Inputs are regenerated from ld_amd.synthetic.COCO_CASES (seeds); only outputs
are stored.  Per case ``{name}_``:
  match, ign    (N,) uint64: per detection of the det2json list, bit t * A + a
                of dtm != 0 / dtIgnore;  kept (N,) bool (rank < maxDets[-1])
  npig          (K, A) int64
  precision, scores (T, R, K, A, M), recall (T, K, A, M) float64
  stats         (12,) float64
  eval          the evaluate() OrderedDict as JSON;  classwise  its table rows
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)

import _cocoeval_oracle as O  # noqa: E402

from ld_amd import synthetic  # noqa: E402


def main():
    d = {}
    for case in synthetic.COCO_CASES:
        name = case[0]
        ds, res, classes, kw = synthetic.coco_eval_inputs(case)
        ev, coco_eval, rows = O.evaluate(ds, res, classes, classwise=True,
                                         **kw)
        n = sum(len(r) for per_img in res for r in per_img)
        match, ign, kept = O.match_bits(coco_eval, n)
        d[f'{name}_match'], d[f'{name}_ign'], d[f'{name}_kept'] = \
            match, ign, kept
        d[f'{name}_npig'] = O.npig(coco_eval)
        for k in ('precision', 'recall', 'scores'):
            d[f'{name}_{k}'] = coco_eval.eval[k]
        d[f'{name}_stats'] = coco_eval.stats
        d[f'{name}_eval'] = np.array(json.dumps(ev))
        d[f'{name}_classwise'] = np.array(json.dumps(rows))
        print(name, n, 'dets', dict(ev))
    out = os.path.join(REPO, 'tests', 'golden', 'coco_eval.npz')
    np.savez_compressed(out, **d)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
