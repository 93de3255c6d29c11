"""GPU (-m gpu): the config's optimizer recipe on the device.

ld_sgd_step_classes / ld_grad_norm (csrc/optim.hip) against ld_sgd_step and a
float64 torch.optim.SGD + clip_grad_norm_; then the whole LD-FCOS step with
paramwise_cfg + grad_clip + a linear warmup (eager, step list, checkpoint
resume, EpochRunner).  18 <- 18 detectors at 128 x 150, fp32."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def _f32(x):
    """A Python float as the kernel sees it (the device table is fp32)."""
    return float(np.float32(x))


def _hyper(mu, gscale, max_norm, lrs, wds):
    vals = [mu, gscale, max_norm, 0.0]
    for lr, wd in zip(lrs, wds):
        vals += [lr, wd]
    return torch.tensor(vals, dtype=torch.float32, device=DEV)


def _arena(sizes, seed):
    """A GradArena-like layout: parameters on 64-float boundaries, zero
    padding; |p| in [1, 2) so fp32 rounding stays far below rtol 1e-6."""
    offs, off = [], 0
    for n in sizes:
        offs.append(off)
        off += (n + 63) // 64 * 64
    gen = torch.Generator().manual_seed(seed)
    p = (torch.rand(off, generator=gen) + 1) * \
        torch.sign(torch.randn(off, generator=gen))
    b = torch.randn(off, generator=gen) * 0.01
    live = torch.zeros(off, dtype=torch.bool)
    for o, n in zip(offs, sizes):
        live[o:o + n] = True
    p[~live], b[~live] = 0, 0
    return offs, live, p.to(DEV), b.to(DEV)


def _grad(live, seed):
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(live.numel(), generator=gen) * 0.1
    g[~live] = 0
    return g.to(DEV)


def _chunk_ids(offs, sizes, classes, total):
    ids = torch.zeros(total // 64, dtype=torch.uint8)
    for o, n, c in zip(offs, sizes, classes):
        ids[o // 64:(o + n + 63) // 64] = c
    return ids.to(DEV)


def test_one_class_bit_identical_to_sgd_kernels():
    from ld_amd import layers as Y
    n = 64 * 997 + 37  # n % 4 != 0 and a partial last chunk
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, generator=gen).to(DEV)
    b0 = (torch.randn(n, generator=gen) * 0.1).to(DEV)
    ids = torch.zeros((n + 63) // 64, dtype=torch.uint8, device=DEV)
    lr, mu, wd, gs = 0.0123, 0.9, 1e-4, 0.5
    runs = {}
    for name in ('value', 'dev', 'classes', 'classes_clip1'):
        p, b = p0.clone(), b0.clone()
        for step in range(2):
            g = (torch.randn(n, generator=torch.Generator().manual_seed(
                10 + step))).to(DEV)
            if name == 'value':
                Y.sgd_step(p, g, b, lr, mu, wd, gs)
            elif name == 'dev':
                Y.sgd_step(p, g, b, 0, 0, 0, 0, hyper=torch.tensor(
                    [lr, mu, wd, gs], dtype=torch.float32, device=DEV))
            else:
                clip = torch.tensor([7.0, 1.0], device=DEV) \
                    if name == 'classes_clip1' else None
                Y.sgd_step_classes(p, g, b, ids, 1,
                                   _hyper(mu, gs, 0.0, [lr], [wd]), clip=clip)
        runs[name] = (p, b)
    torch.cuda.synchronize()
    for name in ('dev', 'classes', 'classes_clip1'):
        assert torch.equal(runs[name][0], runs['value'][0]), name
        assert torch.equal(runs[name][1], runs['value'][1]), name


SIZES = [1000, 333, 4097, 64, 5]
CLASSES = [0, 1, 2, 0, 1]
LRS, WDS = [0.01, 0.02, 0.005], [1e-4, 0.0, 5e-4]


def _reference(p, b, offs, live):
    ps = [p[o:o + n].double().cpu().clone().requires_grad_(True)
          for o, n in zip(offs, SIZES)]
    opt = torch.optim.SGD(
        [dict(params=[q], lr=_f32(LRS[c]), weight_decay=_f32(WDS[c]))
         for q, c in zip(ps, CLASSES)], lr=0.1, momentum=_f32(0.9))
    for q, o, n in zip(ps, offs, SIZES):
        opt.state[q]['momentum_buffer'] = b[o:o + n].double().cpu().clone()
    return ps, opt


def _ref_step(ps, opt, g, offs, gscale, max_norm=None):
    for q, o, n in zip(ps, offs, SIZES):
        q.grad = g[o:o + n].double().cpu() * gscale
    total = None
    if max_norm is not None:
        total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type=2))
    opt.step()
    return total


def _check_params(p, ps, offs):
    for q, o, n in zip(ps, offs, SIZES):
        np.testing.assert_allclose(p[o:o + n].double().cpu().numpy(),
                                   q.detach().numpy(), rtol=1e-6, atol=1e-9)


def test_three_classes_match_float64_sgd():
    from ld_amd import layers as Y
    offs, live, p, b = _arena(SIZES, 1)
    ids = _chunk_ids(offs, SIZES, CLASSES, p.numel())
    ps, opt = _reference(p, b, offs, live)
    hyper = _hyper(0.9, 0.5, 0.0, LRS, WDS)
    for step in range(3):
        g = _grad(live, 20 + step)
        Y.sgd_step_classes(p, g, b, ids, 3, hyper)
        _ref_step(ps, opt, g, offs, _f32(0.5))
    torch.cuda.synchronize()
    _check_params(p, ps, offs)
    assert not p[~live.to(DEV)].any()  # padding stays zero


def _norm(g, gscale, max_norm):
    from ld_amd import layers as Y
    from ld_amd import lib as L
    out = torch.empty(2, dtype=torch.float32, device=DEV)
    ws = torch.empty(L.get_lib().ld_grad_norm_workspace_bytes(),
                     dtype=torch.uint8, device=DEV)
    Y.grad_norm(g, _hyper(0.9, gscale, max_norm, [0.0], [0.0]), out, ws)
    return out


@pytest.mark.parametrize('gscale', [1.0, 0.5])
def test_grad_norm_float64_and_deterministic(gscale):
    n = 3 * (1 << 20) + 7
    g = torch.randn(n, generator=torch.Generator().manual_seed(3)).to(DEV)
    ref = gscale * float(torch.linalg.vector_norm(g.double()))
    outs = [_norm(g, gscale, 35.0) for _ in range(10)]
    torch.cuda.synchronize()
    got = outs[0].cpu()
    assert abs(float(got[0]) - ref) <= 1e-6 * ref
    coef = torch.clamp(torch.tensor(35.0) / (got[0] + 1e-6), max=1.0)
    assert float(got[1]) == float(coef) and float(got[1]) < 1.0
    bits = [o.cpu().view(torch.int32) for o in outs]
    assert all(torch.equal(bits[0], x) for x in bits[1:])


def test_clipped_update_matches_float64_clip_grad_norm():
    from ld_amd import layers as Y
    offs, live, p, b = _arena(SIZES, 2)
    ids = _chunk_ids(offs, SIZES, CLASSES, p.numel())
    ps, opt = _reference(p, b, offs, live)
    max_norm = 0.7  # the 0.5-scaled gradient has norm ~3.8: clipped
    hyper = _hyper(0.9, 0.5, max_norm, LRS, WDS)
    for step in range(3):
        g = _grad(live, 30 + step)
        out = _norm(g, 0.5, max_norm)
        Y.sgd_step_classes(p, g, b, ids, 3, hyper, clip=out)
        total = _ref_step(ps, opt, g, offs, _f32(0.5), max_norm)
        torch.cuda.synchronize()
        assert abs(float(out[0]) - total) <= 1e-6 * total
        assert float(out[1]) < 1.0
    _check_params(p, ps, offs)


def test_huge_max_norm_gives_the_unclipped_bits():
    from ld_amd import layers as Y
    offs, live, p, b = _arena(SIZES, 3)
    ids = _chunk_ids(offs, SIZES, CLASSES, p.numel())
    p2, b2 = p.clone(), b.clone()
    hyper = _hyper(0.9, 0.5, 1e30, LRS, WDS)
    for step in range(2):
        g = _grad(live, 40 + step)
        Y.sgd_step_classes(p, g, b, ids, 3, hyper)
        Y.sgd_step_classes(p2, g, b2, ids, 3, hyper, clip=_norm(g, 0.5, 1e30))
    torch.cuda.synchronize()
    assert torch.equal(p, p2) and torch.equal(b, b2)


# ------------------------------------------------------------ the trainer --
def _batch(seed, num_gt=(3, 2)):
    from ld_amd import synthetic
    b = synthetic.synthetic_batch(2, (128, 150), (128, 160), list(num_gt), seed)
    return dict(img=b['img'].to(DEV), img_metas=b['img_metas'],
                gt_bboxes=[x.to(DEV) for x in b['gt_bboxes']],
                gt_labels=[x.to(DEV) for x in b['gt_labels']])


def _cfg(warmup_iters=2, step=(8, 11), max_norm=35.0, **extra):
    """configs/ld/ld_r50_fcos_r101_1x.py's optimizer with a short warmup and
    a gradient clip."""
    cfg = dict(
        optimizer=dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001,
                       paramwise_cfg=dict(bias_lr_mult=2.0,
                                          bias_decay_mult=0.0)),
        optimizer_config=dict(grad_clip=dict(max_norm=max_norm, norm_type=2)),
        lr_config=dict(policy='step', warmup='linear',
                       warmup_iters=warmup_iters, warmup_ratio=0.001,
                       step=list(step)),
        runner=dict(type='EpochBasedRunner', max_epochs=2),
        log_config=dict(interval=1), checkpoint_config=dict(interval=1))
    cfg.update(extra)
    return cfg


def _fcos_trainer(cfg):
    from ld_amd import model_zoo
    from ld_amd.train import SGDTrainer
    det = model_zoo.build_seeded(model_zoo.ld_fcos_detector(18, 18), DEV)
    return SGDTrainer.from_config(det, cfg)


def _ld_trainer(cfg):
    from ld_amd import model_zoo
    from ld_amd.train import SGDTrainer
    det = model_zoo.build_seeded_ld_detector(18, 18, DEV, loss_im_weight=2.0)
    return SGDTrainer.from_config(det, cfg)


def _within_ulps(got, ref, scale, ulps=4):
    """|got - ref| <= ulps * 2^-24 * scale (fp32 rounding of operands of
    magnitude ``scale``), elementwise."""
    err = (got - ref).abs()
    bound = ulps * 2.0**-24 * scale + 1e-30
    bad = err > bound
    assert not bool(bad.any()), (
        f'{int(bad.sum())} of {got.numel()} off: max err '
        f'{float(err[bad].max()):.3g} at scale {float(scale[bad].max()):.3g}')


def test_ld_fcos_step_matches_float64_sgd():
    """Every step: the new parameters and momentum equal float64 torch SGD
    (per-parameter groups) + clip_grad_norm_ applied to the pre-step state and
    that step's flat_grad; grad_norm is the float64 norm."""
    tr = _fcos_trainer(_cfg(warmup_iters=2, max_norm=10.0))
    pc, arena = tr.param_classes, tr.arena
    cls_of = {id(p): c for p, c in zip(pc.params, pc.class_of)}
    assert len(pc) == 2
    batches = [_batch(21), _batch(22), _batch(21)]
    clipped = []
    for k, d in enumerate(batches):
        P = arena.flat_param.double().cpu()
        B = tr.flat_momentum.double().cpu()
        out = tr.step(d)
        torch.cuda.synchronize()
        G = arena.flat_grad.double().cpu()
        max_norm = tr.grad_clip['max_norm']
        lrs = [tr.lr_schedule.lr_at(0.01 * m, 0, k) for m, _ in pc.classes]
        assert tr.lr == tr.lr_schedule.lr_at(0.01, 0, k)
        ps, groups = [], []
        for p, o in zip(arena.order, arena.offsets):
            q = P[o:o + p.numel()].clone().requires_grad_(True)
            q.grad = G[o:o + p.numel()].clone()
            c = cls_of[id(p)]
            ps.append((q, o, p.numel(), c))
            groups.append(dict(params=[q], lr=_f32(lrs[c]),
                               weight_decay=_f32(1e-4 * pc.classes[c][1])))
        opt = torch.optim.SGD(groups, lr=0.1, momentum=_f32(0.9))
        for q, o, n, _ in ps:
            opt.state[q]['momentum_buffer'] = B[o:o + n].clone()
        total = float(torch.nn.utils.clip_grad_norm_([x[0] for x in ps],
                                                     max_norm))
        opt.step()
        assert abs(float(out['grad_norm']) - total) <= 1e-6 * total
        got_p = arena.flat_param.double().cpu()
        got_b = tr.flat_momentum.double().cpu()
        for q, o, n, c in ps:
            # the kernel evaluates the same fp32 operands in fp32: the buffer
            # within a few ulp of its terms (g * (1/world * clip_coef) carries
            # the fp32 clip coefficient: ~3 ulp from the float64 one), the
            # parameter within lr times that plus its own rounding
            ref_p, ref_b = q.detach(), opt.state[q]['momentum_buffer']
            pre_p, pre_b = P[o:o + n], B[o:o + n]
            terms_b = pre_b.abs() + q.grad.abs() + 1e-3 * pre_p.abs()
            _within_ulps(got_b[o:o + n], ref_b, terms_b, ulps=8)
            _within_ulps(got_p[o:o + n], ref_p,
                         ref_p.abs() + 4 * _f32(lrs[c]) * terms_b, ulps=2)
        clipped.append(total > max_norm)
    assert any(clipped) and tr.iter == 3


@pytest.mark.parametrize('launcher', ['graph', 'list'])
def test_captured_step_follows_the_schedule_bit_for_bit(launcher):
    """GraphedStep replays (hipGraphLaunch and the step list) across the
    warmup -> regular boundary (iter 2) and the epoch-1 milestone: the same
    parameters and momentum as eager steps."""
    from ld_amd.train import GraphedStep
    cfg = _cfg(warmup_iters=2, step=(1,))
    d = _batch(21)
    eager = _ld_trainer(cfg)
    outs_e = []
    for k in range(4):
        if k == 3:
            eager.begin_epoch(1)
        outs_e.append(eager.step(d))
    torch.cuda.synchronize()
    lr_e = eager.lr
    tr = _ld_trainer(cfg)
    g = GraphedStep(tr, _batch(21), warmup=1, launcher=launcher)  # iter 0
    assert tr.iter == 1
    outs_g = []
    for k in range(1, 4):
        if k == 3:
            tr.begin_epoch(1)
        outs_g.append(g.replay())
    torch.cuda.synchronize()
    assert tr.lr == lr_e == pytest.approx(0.001, rel=1e-12)
    assert torch.equal(tr.arena.flat_param, eager.arena.flat_param)
    assert torch.equal(tr.flat_momentum, eager.flat_momentum)
    assert float(outs_g[-1]['grad_norm']) == float(outs_e[-1]['grad_norm'])
    assert float(outs_g[-1]['loss']) == float(outs_e[-1]['loss'])


def test_resume_mid_warmup_is_bit_exact(tmp_path):
    from ld_amd import checkpoint as CK
    cfg = _cfg(warmup_iters=500)
    seq = [_batch(21), _batch(22), _batch(23), _batch(24)]
    full = _fcos_trainer(cfg)
    for d in seq:
        full.step(d)
    torch.cuda.synchronize()
    first = _fcos_trainer(cfg)
    for d in seq[:2]:
        first.step(d)
    path = str(tmp_path / 'iter_2.pth')
    CK.save_checkpoint(first.model, path, optimizer=first,
                       meta=dict(epoch=0, iter=first.iter))
    del first
    resumed = _fcos_trainer(cfg)
    CK.resume(resumed, path)
    assert resumed.iter == 2 and resumed.epoch == 0
    for d in seq[2:]:
        resumed.step(d)
    torch.cuda.synchronize()
    assert torch.equal(resumed.arena.flat_param, full.arena.flat_param)
    assert torch.equal(resumed.flat_momentum, full.flat_momentum)
    # mmcv's layout: one group per parameter, each with its initial_lr
    sd = torch.load(path, map_location='cpu')['optimizer']
    pc = resumed.param_classes
    assert len(sd['param_groups']) == len(pc.mults)
    for g, (lm, dm) in zip(sd['param_groups'], pc.mults):
        assert g['initial_lr'] == 0.01 * lm and g['weight_decay'] == 1e-4 * dm
    params = [p.detach().cpu().clone().requires_grad_(p.requires_grad)
              for p in resumed.model.parameters()]
    opt = torch.optim.SGD([dict(params=[p]) for p in params], lr=0.01,
                          momentum=0.9)
    opt.load_state_dict(sd)
    assert [g['lr'] for g in opt.param_groups] == \
        [g['lr'] for g in sd['param_groups']]


def test_epoch_runner_logs_checkpoints_and_resumes(tmp_path):
    from ld_amd.runner import EpochRunner

    def batches(epoch):
        return [_batch(30 + 2 * epoch), _batch(31 + 2 * epoch)]

    cfg = _cfg(warmup_iters=3, step=(1,))
    tr = _fcos_trainer(cfg)
    recs = EpochRunner(tr, cfg, tmp_path / 'a').run(batches)
    torch.cuda.synchronize()
    lines = [json.loads(x) for x in
             open(tmp_path / 'a' / 'train.log.json').read().splitlines()]
    assert lines == recs and len(lines) == 4
    assert [(r['epoch'], r['iter']) for r in lines] == [(1, 1), (1, 2), (2, 1),
                                                        (2, 2)]
    for r in lines:
        assert r['mode'] == 'train' and 'loss_cls' in r and r['grad_norm'] > 0
    assert lines[0]['lr'] == pytest.approx(1e-5, rel=1e-12)
    assert lines[3]['lr'] == pytest.approx(0.001, rel=1e-12)  # epoch-1 milestone
    for k in (1, 2):
        assert os.path.isfile(tmp_path / 'a' / f'epoch_{k}.pth')
    meta = torch.load(tmp_path / 'a' / 'epoch_1.pth', map_location='cpu')['meta']
    assert meta['epoch'] == 1 and meta['iter'] == 2
    cfg2 = dict(cfg, resume_from=str(tmp_path / 'a' / 'epoch_1.pth'))
    tr2 = _fcos_trainer(cfg2)
    recs2 = EpochRunner(tr2, cfg2, tmp_path / 'b').run(batches)
    torch.cuda.synchronize()
    assert [(r['epoch'], r['iter']) for r in recs2] == [(2, 1), (2, 2)]
    assert tr2.iter == tr.iter == 4 and tr2.epoch == tr.epoch == 2
    assert torch.equal(tr2.arena.flat_param, tr.arena.flat_param)
    assert torch.equal(tr2.flat_momentum, tr.flat_momentum)


def test_epoch_runner_pipelined_equals_eager(tmp_path):
    """AutoStepper('pipelined') under EpochRunner over 2 epochs (warmup ->
    regular inside epoch 1, the milestone at epoch 1, the look-ahead across
    the epoch boundary): the same parameters, momentum and log lines as the
    eager trainer under the same runner."""
    from ld_amd.runner import EpochRunner
    from ld_amd.train import AutoStepper

    def batches(epoch):
        for k, gt in enumerate(((3, 2), (5, 1))):
            yield _batch(50 + 2 * epoch + k, gt)

    cfg = _cfg(warmup_iters=3, step=(1,))
    eager = _ld_trainer(cfg)
    rec_e = EpochRunner(eager, cfg, tmp_path / 'e').run(batches)
    torch.cuda.synchronize()
    tr = _ld_trainer(cfg)
    st = AutoStepper(tr, mode='pipelined', max_gt=16)
    rec_p = EpochRunner(st, cfg, tmp_path / 'p').run(batches)
    torch.cuda.synchronize()
    assert st.captures == 1 and tr.iter == eager.iter == 4
    assert torch.equal(tr.arena.flat_param, eager.arena.flat_param)
    assert torch.equal(tr.flat_momentum, eager.flat_momentum)
    assert rec_p == rec_e and len(rec_p) == 4
