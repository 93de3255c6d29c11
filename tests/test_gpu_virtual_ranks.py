"""GPU (-m gpu): ``SGDTrainer(virtual_ranks=W)`` -- one optimizer step on the W
rank-local micro-batches of a W-process job, with that job's semantics
(DESIGN.md section 6).

The expected step is built by hand the way tests/test_gpu_ddp_halves.py builds
the reference's data-parallel semantics: the partials every rank's prepass
leaves in norm[0:2] are captured through a replaced ``_norm_reducer``, their
mean is injected into every rank's loss block through the same hook, every
rank's backward runs on its own WITHOUT a gradient arena, and gradients and
logged values are averaged in float64.  The virtual step must give the same.

Detector and shapes: the seeded R18 <- R18 detectors at 128 x 150 padded to
128 x 160, 4 images with [3, 2, 5, 1] boxes (the halves test's batch).

Bounds (none fitted to this code): gradients 2e-4 of each tensor's max and
logged values 2e-5 relative (tests/test_gpu_ddp_halves.py:110, :97 -- the same
fp32 re-ordering between two ways of accumulating); gradient norms 1e-3
relative (README parity row); everything the project promises bitwise
(determinism, ``virtual_ranks=1``, the normaliser) bit for bit."""
import json
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dataset_fixture as FX  # noqa: E402
import test_dataloader_host as TH  # noqa: E402  (TRAIN_PIPELINE, voc())

DEV = torch.device('cuda:0')
KLD = ('loss_ld', 'loss_ld_vlr')
GRAD_TOL = 2e-4   # tests/test_gpu_ddp_halves.py:110
LOG_TOL = 2e-5    # tests/test_gpu_ddp_halves.py:97
NORM_TOL = 1e-3   # README parity row: gradient norms


def _batch():
    from ld_amd import synthetic
    b = synthetic.synthetic_batch(4, (128, 150), (128, 160), [3, 2, 5, 1], 77)
    return dict(img=b['img'].to(DEV), img_metas=b['img_metas'],
                gt_bboxes=[x.to(DEV) for x in b['gt_bboxes']],
                gt_labels=[x.to(DEV) for x in b['gt_labels']])


def _part(d, lo, hi):
    return dict(img=d['img'][lo:hi].contiguous(), img_metas=d['img_metas'][lo:hi],
                gt_bboxes=d['gt_bboxes'][lo:hi], gt_labels=d['gt_labels'][lo:hi])


def _split(d, W):
    n = len(d['img_metas']) // W
    return [_part(d, r * n, (r + 1) * n) for r in range(W)]


def _detector(kind):
    from ld_amd import model_zoo
    if kind == 'LDHead':  # gibox imitation, the halves test's detector
        det = model_zoo.build_seeded_ld_detector(18, 18, DEV, loss_im_weight=2.0)
    elif kind == 'LDATSSHead':
        det = model_zoo.build_seeded(model_zoo.ld_atss_detector(18, 18), DEV)
    else:
        det = model_zoo.build_seeded(model_zoo.ldv2_detector(18, 18), DEV)
    assert type(det.bbox_head).__name__ == kind
    return det


@contextmanager
def _reducer(fn):
    """``_norm_reducer`` of every dense head replaced by one returning ``fn``."""
    from ld_amd.heads import _DenseHead
    old = _DenseHead.__dict__['_norm_reducer']
    _DenseHead._norm_reducer = staticmethod(lambda: fn)
    try:
        yield
    finally:
        _DenseHead._norm_reducer = old


def _one_rank(det, data):
    """forward + _parse_losses + backward of one rank, no arena: (logged
    values, float64 gradients)."""
    for p in det.parameters():
        p.grad = None
    loss, log_vars = det._parse_losses(det(**data))
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().double().clone()
             for n, p in det.named_parameters()
             if p.requires_grad and p.grad is not None}
    return {k: float(v) for k, v in dict(log_vars).items()}, grads


def _manual(det, parts):
    """The W-rank job's step by hand -> (captured partials, injected mean,
    mean logged values, mean gradients)."""
    W = len(parts)
    seen = []
    with _reducer(lambda norm: seen.append(norm[:2].clone())):
        for h in parts:
            det(**h)
    assert len(seen) == W
    acc = seen[0].clone()
    for s in seen[1:]:
        acc = acc + s
    mean = acc / float(W)  # all-reduce(sum), then div_(world)

    def _inject(norm):
        norm[:2] = mean

    with _reducer(_inject):
        ranks = [_one_rank(det, h) for h in parts]
    logs = {k: sum(r[0][k] for r in ranks) / W for k in ranks[0][0]}
    grads = {n: sum(r[1][n] for r in ranks) / W for n in ranks[0][1]}
    return seen, mean, logs, grads


def _check_step_against_manual(kind):
    from ld_amd.train import SGDTrainer
    det = _detector(kind)
    det.use_teacher_stream = False
    full = _batch()
    halves = _split(full, 2)
    with _reducer(None):
        v4, _ = _one_rank(det, full)  # the 4-image step of ONE rank
    seen, mean, logs, grads = _manual(det, halves)
    tr = SGDTrainer(det, lr=0.0, momentum=0.9, weight_decay=1e-4,
                    virtual_ranks=2)
    out = tr.step(halves)
    torch.cuda.synchronize()
    assert tr.iter == 1 and out['num_samples'] == 4
    # the table holds what the ranks' prepasses left, the mean what was injected
    vr = tr._vranks
    for r in range(2):
        assert torch.equal(vr.partials[r, :2], seen[r]), (r, vr.partials, seen)
    assert torch.equal(vr.norm[:2], mean)
    got = {k: float(v) for k, v in dict(out['log_vars']).items()}
    assert set(got) == set(logs)
    for k, want in logs.items():
        err = abs(got[k] - want)
        print(kind, k, 'virtual', got[k], 'manual', want, '4-image', v4[k])
        assert err <= LOG_TOL * max(abs(want), 1e-3), (k, got[k], want)
    assert abs(float(out['loss']) - logs['loss']) <= \
        LOG_TOL * max(abs(logs['loss']), 1e-3)
    # the reference divides the LD terms by constants: two ranks of 2 images
    # log HALF the 4-image value
    ld_keys = [k for k in KLD if k in got]
    assert ld_keys
    for k in ld_keys:
        assert v4[k] > 0
        assert abs(got[k] - 0.5 * v4[k]) <= LOG_TOL * max(abs(v4[k]), 1e-3), \
            (k, got[k], v4[k])
    names = {id(p): n for n, p in det.named_parameters()}
    assert {names[id(p)] for p in tr.arena.order} == set(grads)
    worst = 0.0
    for p in tr.arena.order:
        n = names[id(p)]
        have = p.grad.detach().double() / 2.0  # the arena holds the rank SUM
        want = grads[n]
        scale = float(want.abs().max())
        if scale < 1e-12:
            assert float(have.abs().max()) < 1e-9, n
            continue
        err = float((have - want).abs().max()) / scale
        worst = max(worst, err)
        assert err < GRAD_TOL, (kind, n, err)
    print(kind, 'worst relative gradient difference', worst)


@pytest.mark.parametrize('kind', ['LDHead', 'LDATSSHead', 'LDv2Head'])
def test_virtual_step_equals_the_manual_two_rank_step(kind):
    _check_step_against_manual(kind)


def test_virtual_step_equals_the_manual_two_rank_step_bf16():
    from ld_amd import layers as Y
    Y.set_precision('bf16')
    try:
        _check_step_against_manual('LDHead')
    finally:
        Y.set_precision('fp32')


@pytest.mark.parametrize('W', [2, 4])
def test_injected_normaliser_is_the_ascending_fp32_mean(W):
    from ld_amd.train import SGDTrainer
    det = _detector('LDHead')
    parts = _split(_batch(), W)
    tr = SGDTrainer(det, lr=0.0, virtual_ranks=W)
    for _ in range(2):  # the second step replays the recorded teacher
        tr.step(parts)
    torch.cuda.synchronize()
    part = tr._vranks.partials.cpu().numpy()
    assert part.dtype == np.float32 and part.shape == (W, 4)
    acc = part[0, :2].copy()
    for r in range(1, W):
        acc = (acc + part[r, :2]).astype(np.float32)
    want = (acc / np.float32(W)).astype(np.float32)
    got = tr._vranks.norm.cpu().numpy()[:2]
    print('partials', part[:, :2].tolist(), 'mean', got.tolist())
    np.testing.assert_array_equal(got, want)
    # the images carry 3, 2, 5, 1 boxes: the ranks' partials really differ
    assert len({float(v) for v in part[:, 0]}) > 1
    assert float(part[:, 0].sum()) > 0 and np.all(part[:, 1] > 0)


def test_teacher_outputs_stay_private_to_their_micro_batch():
    """The frozen teacher's replayed outputs live in rotating slots
    (TEACHER_SLOTS, 3 for a plain step); W = 4 micro-batches hold theirs from
    the forward to the loss block's main part, so the trainer asks for W + 2.
    With lr 0 every step is the same step: once the slots rotate (from the
    third step on) gradients and logged values stay bit-identical."""
    from ld_amd.train import SGDTrainer
    det = _detector('LDHead')
    parts = _split(_batch(), 4)
    tr = SGDTrainer(det, lr=0.0, momentum=0.9, weight_decay=1e-4,
                    virtual_ranks=4)
    assert det.TEACHER_SLOTS == 6
    first = None
    for k in range(5):
        out = tr.step(parts)
        torch.cuda.synchronize()
        got = (tr.arena.flat_grad.clone(), out['log_vars']._tensor.clone())
        if first is None:
            first = got
        assert torch.equal(got[0], first[0]), k
        assert torch.equal(got[1], first[1]), k
    assert getattr(det, 'teacher_replays', 0) >= 8  # steps 3 to 5 replayed


def _twin(clip):
    from ld_amd.train import SGDTrainer
    half = _split(_batch(), 2)[0]
    kw = dict(lr=0.01, momentum=0.9, weight_decay=1e-4)
    if clip:
        kw['grad_clip'] = dict(max_norm=35)
    a, b = _detector('LDHead'), _detector('LDHead')
    tv = SGDTrainer(a, virtual_ranks=2, **kw)
    tp = SGDTrainer(b, **kw)
    ov = tv.step([half, half])
    op = tp.step(half)
    torch.cuda.synchronize()
    assert ov['num_samples'] == 2 * op['num_samples']
    assert [tuple(p.shape) for p in tv.arena.order] == \
        [tuple(p.shape) for p in tp.arena.order]
    worst = 0.0
    for pv, pp in zip(tv.arena.order, tp.arena.order):
        want = pp.data.double()
        scale = float(want.abs().max())
        err = float((pv.data.double() - want).abs().max())
        if scale < 1e-12:
            assert err < 1e-9
            continue
        worst = max(worst, err / scale)
        assert err / scale < GRAD_TOL, (tuple(pv.shape), err / scale)
    print('clip' if clip else 'plain', 'worst relative parameter difference',
          worst)
    for k, v in dict(op['log_vars']).items():
        assert abs(float(ov['log_vars'][k]) - float(v)) <= \
            LOG_TOL * max(abs(float(v)), 1e-3), k
    return ov, op


def test_twin_ranks_equal_one_plain_step():
    _twin(False)


def test_twin_ranks_equal_one_plain_step_with_grad_clip():
    ov, op = _twin(True)
    gv, gp = float(ov['grad_norm']), float(op['grad_norm'])
    print('grad_norm virtual', gv, 'plain', gp)
    assert gp > 0 and abs(gv - gp) <= NORM_TOL * gp


def test_virtual_step_is_deterministic():
    from ld_amd.train import AutoStepper, SGDTrainer
    det = _detector('LDHead')
    halves = _split(_batch(), 2)
    tr = SGDTrainer(det, lr=0.01, momentum=0.9, weight_decay=1e-4,
                    virtual_ranks=2)
    stepper = AutoStepper(tr)  # eager; its state save / restore helpers
    tr.step(halves)            # caches and the teacher's recordings settle
    state = stepper._saved_state()
    runs = []
    for _ in range(2):
        stepper._restore_state(state)
        out = tr.step(halves)
        torch.cuda.synchronize()
        runs.append((tr.arena.flat_grad.clone(), tr.arena.flat_param.clone(),
                     out['log_vars']._tensor.clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    assert float(runs[0][0].abs().max()) > 0


def test_one_virtual_rank_is_the_plain_step():
    from ld_amd.train import SGDTrainer
    full = _batch()
    a, b = _detector('LDHead'), _detector('LDHead')
    kw = dict(lr=0.01, momentum=0.9, weight_decay=1e-4)
    t1 = SGDTrainer(a, virtual_ranks=1, **kw)
    t0 = SGDTrainer(b, **kw)
    assert t1._vranks is None
    for k in range(2):
        # a plain dict as today; a sequence of one is accepted as well
        o1 = t1.step(full if k == 0 else [full])
        o0 = t0.step(full)
        torch.cuda.synchronize()
        assert torch.equal(o1['loss'], o0['loss'])
        assert torch.equal(o1['log_vars']._tensor, o0['log_vars']._tensor)
        assert o1['num_samples'] == o0['num_samples'] == 4
        assert torch.equal(t1.arena.flat_grad, t0.arena.flat_grad)
        assert torch.equal(t1.arena.flat_param, t0.arena.flat_param)
        assert torch.equal(t1.flat_momentum, t0.flat_momentum)
    assert t1.iter == t0.iter == 2
    assert t1._vranks is None and a.TEACHER_SLOTS == b.TEACHER_SLOTS == 3


def test_epoch_runner_one_line_per_optimizer_step(tmp_path_factory, tmp_path):
    from ld_amd.dataloader import build_dataloader
    from ld_amd.runner import EpochRunner
    from ld_amd.train import SGDTrainer
    root = FX.write_fixture(tmp_path_factory.mktemp('fixture'))
    ds = TH.voc(root)
    cfg = dict(
        optimizer=dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001),
        optimizer_config=dict(grad_clip=dict(max_norm=35.0, norm_type=2)),
        lr_config=dict(policy='step', warmup='linear', warmup_iters=3,
                       warmup_ratio=0.001, step=[1]),
        runner=dict(type='EpochBasedRunner', max_epochs=1),
        log_config=dict(interval=1), checkpoint_config=dict(interval=1))
    loader = build_dataloader(ds, 2, 1, seed=5, device=DEV, virtual_ranks=2,
                              num_threads=2)
    one_rank = build_dataloader(ds, 2, 1, dist=True, seed=5, device=DEV,
                                num_replicas=2, rank=0)
    n = len(one_rank)
    assert len(loader) == n > 0
    tr = SGDTrainer.from_config(_detector('LDHead'), cfg, virtual_ranks=2)
    recs = EpochRunner(tr, cfg, tmp_path).run(loader)
    torch.cuda.synchronize()
    loader.close()
    one_rank.close()
    lines = [json.loads(x) for x in
             open(tmp_path / 'train.log.json').read().splitlines()]
    train = [r for r in lines if r['mode'] == 'train']
    assert train == recs and len(train) == n
    assert [r['iter'] for r in train] == list(range(1, n + 1))
    assert train[-1]['iter'] == n == tr.iter
    for r in train:
        assert np.isfinite(r['loss']) and np.isfinite(r['grad_norm'])
    # the warm-up follows the W-rank job's iteration count: one lr per step
    assert len({r['lr'] for r in train}) == min(n, 3)
