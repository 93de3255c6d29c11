"""GPU (-m gpu): the HIP loss block under the VIRTUAL cross-rank normaliser
against the reference's own output under a REAL two-rank process group
(tests/golden/lossblock_2rank.npz, oracle/gen_golden.py gen_lossblock_2rank: two
gloo ranks run LDHead.loss on different cases, reduce_mean all-reduces the two
normaliser partials, ld_head.py:338-341, 362-365, and _parse_losses averages
every logged value over the ranks, base.py:211-214).

Here the two cases are the two virtual ranks of one process: each rank's
prepass leaves its partials in its row of the (W, 4) table, ld_vrank_reduce
forms the mean, each rank's main / finalise part reads it
(lossblock.VirtualRanks / DeferredNorm, the path SGDTrainer(virtual_ranks=2)
takes), and the per-rank logged values go through the same launch.

Bound: 1e-4, the project's loss-parity bound against the reference
(tests/test_gpu_lossblock.py LOSS_ATOL / LOSS_RTOL, README "parity")."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-4


def _inputs(golden, name, dev):
    """What tests/test_gpu_lossblock.py loads for a case, on the device."""
    from ld_amd import lossblock as LB
    from ld_amd import synthetic
    g = golden['lossblock']
    cfg = g[name + '_cfg']
    pad, img_shape = tuple(cfg[:2]), tuple(cfg[2:4])
    bseed, hseed = int(cfg[4]), int(cfg[5])
    num_gt = [int(x) for x in g[name + '_num_gt']]
    batch = synthetic.synthetic_batch(len(num_gt), img_shape, pad, num_gt,
                                      bseed)
    sizes = synthetic.level_shapes(pad)
    hi = synthetic.synthetic_head_inputs(len(num_gt), sizes, seed=hseed)
    hp = LB.make_hp()
    t = LB.atss_targets(
        sizes, [8, 16, 32, 64, 128], batch['img_metas'],
        [b.to(dev) for b in batch['gt_bboxes']],
        [l.to(dev) for l in batch['gt_labels']], hp, dev)
    d = {k: [x.to(dev) for x in v] for k, v in hi.items()}
    return hp, t, d


@pytest.mark.parametrize('tag', ['small_pair', 'c2_pair'])
def test_two_virtual_ranks_equal_the_reference_two_rank_group(golden, tag):
    from ld_amd import lossblock as LB
    dev = torch.device('cuda:0')
    g2 = np.load(os.path.join(HERE, 'golden', 'lossblock_2rank.npz'))
    cases = [str(c) for c in g2[tag + '_cases']]
    assert len(cases) == 2
    vr = LB.VirtualRanks(2, dev)
    tables, keep = [], []
    with vr:
        for r, name in enumerate(cases):
            hp, t, d = _inputs(golden, name, dev)
            vr.rank = r
            losses, _, norm, _ = LB.loss_block_forward(
                hp, t, d['cls'], d['reg'], d['t_cls'], d['t_reg'], d['x'],
                d['t_x'], reduce_norm=vr.slot())
            tables.append(losses)
            keep.append((hp, t, d, norm))
    vr.reduce_norm()
    for r in range(2):
        vr.complete(r)
    # _parse_losses of each rank: the 8 key sums and their total, then the
    # rank mean of all 9 through the same launch
    for r in range(2):
        vr.rank = r
        sums = tables[r].sum(1)
        torch.cat([sums, sums.sum().reshape(1)], out=vr.log_row(9))
    logged = vr.reduce_logs()
    torch.cuda.synchronize()
    part = vr.partials.cpu().numpy()
    mean = vr.norm.cpu().numpy()
    # the injected normalisers: (p0 + p1) / 2 in float32, bit for bit
    np.testing.assert_array_equal(
        mean[:2], ((part[0, :2] + part[1, :2]) / np.float32(2)))
    assert part[0, 0] != part[1, 0]  # the ranks really differ
    want_log = g2[f'{tag}_r0_log_vars']
    np.testing.assert_array_equal(want_log, g2[f'{tag}_r1_log_vars'])
    for r in range(2):
        got = tables[r].cpu().numpy().astype(np.float64)
        ref = g2[f'{tag}_r{r}_losses']
        print(tag, 'rank', r, 'max abs table difference',
              float(np.abs(got - ref).max()))
        np.testing.assert_allclose(got, ref, rtol=TOL, atol=TOL)
        np.testing.assert_allclose(float(got.sum()),
                                   float(g2[f'{tag}_r{r}_loss']),
                                   rtol=TOL, atol=TOL)
    got_log = logged.cpu().numpy().astype(np.float64)
    print(tag, 'log_vars', got_log, 'reference', want_log)
    np.testing.assert_allclose(got_log, want_log, rtol=TOL, atol=TOL)
