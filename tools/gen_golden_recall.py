"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/recall.npz by EXECUTING THE
REFERENCE's proposal recall on CPU (the reference package is imported,
unmodified, through oracle/ref_shim.py).  Run from the repo root in the build
container, never on the GPU machine:

    python tools/gen_golden_recall.py

Reference entry points exercised (file:line under the reference tree):
  mmdet/core/evaluation/bbox_overlaps.py:4-48  bbox_overlaps
  mmdet/core/evaluation/recall.py:10-40        _recalls
  mmdet/core/evaluation/recall.py:64-106       eval_recalls ('equal*' runs)

``eval_recalls`` does ``np.array(all_ious)`` on a list of per-image arrays,
which raises ValueError under the installed numpy unless all of them have one
shape.  The ragged runs therefore call the reference's own ``bbox_overlaps``
and ``_recalls`` on an object array built by hand; the score order, the cap at
``proposal_nums[-1]`` and the no-GT case that lead up to them are ``ragged``
below.  The equal-shape runs go through ``eval_recalls`` whole
(``print_recall_summary`` stubbed: terminaltables is absent).

Inputs are regenerated from ld_amd.synthetic.RECALL_CASES (seeds); only the
reference outputs are stored, per run ``{tag}``:
  {tag}_recalls   (P, T) float64
  {tag}_gt_ious   (P, total_gt) float32: ``_ious`` of recall.py:15-33 BEFORE
                  its sort (captured at the ``np.sort`` call), image after
                  image, matching round after round
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'oracle'))
sys.path.insert(0, REPO)

import gen_golden as G  # noqa: E402,F401  (installs ref_shim)

from ld_amd import synthetic  # noqa: E402
from ld_amd.recall import set_recall_param  # noqa: E402


class _SortSpy:
    """Records the argument of the one ``np.sort`` call of ``_recalls``."""

    def __enter__(self):
        self.real, self.seen = np.sort, []

        def spy(a, *args, **kw):
            self.seen.append(np.array(a, copy=True))
            return self.real(a, *args, **kw)

        np.sort = spy
        return self

    def __exit__(self, *exc):
        np.sort = self.real


def ragged(R, BO, gts, proposals, proposal_nums, iou_thrs):
    """What ``eval_recalls`` hands to ``_recalls``, image by image and of any
    shape: proposals in descending score order (given order without scores),
    the first ``proposal_nums[-1]`` of them against the GTs, and an array
    without rows for an image without GTs."""
    nums, thrs = set_recall_param(proposal_nums, iou_thrs)
    per_image = np.empty(len(gts), dtype=object)
    for n, (gt, props) in enumerate(zip(gts, proposals)):
        if props.shape[1:] == (5, ):
            assert np.unique(props[:, 4]).size == len(props), 'equal scores'
            props = props[np.argsort(-props[:, 4], kind='stable')]
        if gt is None or len(gt) == 0:
            per_image[n] = np.zeros((0, len(props)), np.float32)
        else:
            per_image[n] = BO.bbox_overlaps(gt, props[:int(nums[-1]), :4])
    with np.errstate(invalid='ignore'):
        return R._recalls(per_image, nums, thrs)


def main():
    from mmdet.core.evaluation import bbox_overlaps as BO
    from mmdet.core.evaluation import recall as R
    R.print_recall_summary = lambda *a, **k: None
    d = {}
    for tag, gts, props, nums, thrs, whole, interior in \
            synthetic.recall_cases():
        with _SortSpy() as spy:
            if whole:
                rec = R.eval_recalls(gts, props, nums, thrs)
            else:
                rec = ragged(R, BO, gts, props, nums, thrs)
        assert len(spy.seen) == 1
        table = spy.seen[0]
        assert rec.dtype == np.float64 and table.dtype == np.float32
        if interior:
            assert synthetic.recall_is_interior(rec), (tag, rec)
        d[f'{tag}_recalls'] = rec
        d[f'{tag}_gt_ious'] = table
        print(f'[recall] {tag}: gts {table.shape[1]}, recalls\n{rec}',
              flush=True)
    np.savez_compressed(os.path.join(REPO, 'tests', 'golden', 'recall.npz'),
                        **d)


if __name__ == '__main__':
    main()
