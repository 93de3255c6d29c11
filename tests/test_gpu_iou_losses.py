"""GPU tests (-m gpu) of the IoU / DIoU / CIoU box losses against the
reference's own outputs (tests/golden/iou_losses.npz, written by
tools/gen_golden_iou_losses.py): the row modules, the fused loss block with each
``bbox_loss`` in both level layouts, the ATSS / FCOS / Retina heads, GFLHead
with CIoULoss (the teacher-training path) and one whole train step of
configs/ld/ld_r18_gflv1_r101_fpn_voc_1x.py, eager and through the step list.

Tolerances are the project's: tables rtol = atol = 1e-4; loss-block gradients
rtol 5e-4 / atol 1e-7 element-wise and rtol 2e-4 on abs_sum; rows as
tests/test_gpu_modules.py applies to GIoULoss, against the reference's float64
run (tests/_iou_losses.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _iou_losses as IL  # noqa: E402

pytestmark = pytest.mark.gpu

LOSS_RTOL = LOSS_ATOL = 1e-4
LOSS_KEYS = ['loss_cls', 'loss_bbox', 'loss_dfl', 'loss_ld', 'loss_ld_vlr',
             'loss_kd', 'loss_kd_neg', 'loss_im']
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def rows(golden):
    g = golden['iou_losses']
    pred, target = IL.row_inputs(g)
    rng = np.random.RandomState(5)
    weight = rng.rand(len(pred)).astype(np.float32)
    weight[::7] = 0.0
    return g, pred, target, weight


@pytest.mark.parametrize('name', IL.LOSSES)
def test_row_modules_vs_float64_reference(rows, name):
    from ld_amd import build_loss
    g, pred, target, weight = rows
    l64, g64 = g[f'{name}_loss64'], g[f'{name}_grad64']
    l_rtol, g_rtol = IL.bars(g, name)
    t = torch.from_numpy(target).to(DEV)
    w = torch.from_numpy(weight).to(DEV)
    mod = build_loss(dict(loss_weight=2.0, **IL.MODULE_CFG[name]))

    def run(**kw):
        p = torch.from_numpy(pred).to(DEV).requires_grad_(True)
        out = mod(p, t, **kw)
        out.sum().backward()
        return out.detach().cpu().numpy(), p.grad.cpu().numpy()

    # reduction 'none' (257 rows: two 128-thread blocks and one row)
    got, grad = run(reduction_override='none')
    print(name, 'none: max |err| loss', np.abs(got - 2 * l64).max(), 'grad',
          np.abs(grad - 2 * g64).max())
    np.testing.assert_allclose(got, 2 * l64, rtol=l_rtol, atol=2 * IL.LOSS_ATOL)
    np.testing.assert_allclose(grad, 2 * g64, rtol=g_rtol,
                               atol=2 * IL.GRAD_ATOL)
    n = len(pred)
    w64 = weight.astype(np.float64)
    # 'mean' (the default), 'sum', weighted with avg_factor, (n, 4) weights
    for kw, scale, wv in (
            (dict(), 2.0 / n, np.ones(n)),
            (dict(reduction_override='sum'), 2.0, np.ones(n)),
            (dict(weight=w, avg_factor=37.5), 2.0 / 37.5, w64),
            (dict(weight=w[:, None].expand(n, 4), reduction_override='sum'),
             2.0, w64)):
        got, grad = run(**kw)
        want = scale * (wv * l64).sum()
        np.testing.assert_allclose(float(got), want, rtol=l_rtol,
                                   atol=IL.LOSS_ATOL, err_msg=str(kw))
        np.testing.assert_allclose(
            grad, scale * wv[:, None] * g64, rtol=g_rtol,
            atol=abs(scale) * IL.GRAD_ATOL, err_msg=str(kw))
    # no positive weight: exactly 0, zero gradient, whatever the reduction
    for kw in (dict(avg_factor=4.0), dict(reduction_override='sum')):
        got, grad = run(weight=torch.zeros(n, 4, device=DEV), **kw)
        assert float(got) == 0 and not grad.any()
    got, grad = run(weight=torch.zeros(n, device=DEV),
                    reduction_override='none')
    assert not got.any() and not grad.any()


# ------------------------------------------------------------ loss block ----
def _block_inputs(golden, name):
    from ld_amd import synthetic
    g = golden['lossblock']
    cfg = g[name + '_cfg']
    pad, img_shape = tuple(cfg[:2]), tuple(cfg[2:4])
    num_gt = [int(x) for x in g[name + '_num_gt']]
    batch = synthetic.synthetic_batch(len(num_gt), img_shape, pad, num_gt,
                                      int(cfg[4]))
    sizes = synthetic.level_shapes(pad)
    hi = synthetic.synthetic_head_inputs(len(num_gt), sizes, seed=int(cfg[5]))
    return g, batch, sizes, hi


def _run_block(batch, sizes, hi, bbox_loss, packed):
    from ld_amd import lossblock as LB
    dev = torch.device(DEV)
    hp = LB.make_hp(bbox_loss=bbox_loss)
    t = LB.atss_targets(sizes, [8, 16, 32, 64, 128], batch['img_metas'],
                        [b.to(dev) for b in batch['gt_bboxes']],
                        [l.to(dev) for l in batch['gt_labels']], hp, dev)
    N, A = len(batch['img_metas']), sum(h * w for h, w in sizes)

    def to_dev(lst):
        if not packed:
            return [x.to(dev) for x in lst]
        c = lst[0].shape[1]
        arena = torch.empty((N, c, A), device=dev)
        views, off = [], 0
        for x, (h, w) in zip(lst, sizes):
            v = arena[:, :, off:off + h * w].view(N, c, h, w)
            v.copy_(x)
            views.append(v)
            off += h * w
        return views

    d = {k: to_dev(v) for k, v in hi.items()}
    losses, grads, _, _ = LB.loss_block_forward(
        hp, t, d['cls'], d['reg'], d['t_cls'], d['t_reg'], d['x'], d['t_x'])
    torch.cuda.synchronize()
    return losses, grads


@pytest.mark.parametrize('packed', [False, True])
@pytest.mark.parametrize('bbox_loss', ['ciou', 'diou', 'iou'])
@pytest.mark.parametrize('name', ['small', 'small_crowd'])
def test_lossblock_vs_reference(golden, name, bbox_loss, packed):
    base, batch, sizes, hi = _block_inputs(golden, name)
    g = golden['iou_losses']
    key = f'lb_{name}_{bbox_loss}'
    losses, grads = _run_block(batch, sizes, hi, bbox_loss, packed)
    got = losses.cpu().numpy().astype(np.float64)
    ref = g[key + '_losses']
    print(key, 'loss_bbox', got[1], ref[1], 'max |err|', np.abs(got - ref).max())
    np.testing.assert_allclose(got, ref, rtol=LOSS_RTOL, atol=LOSS_ATOL)
    # the box loss must have been the one asked for, not GIoU
    assert not np.allclose(got[1], base[name + '_losses'][1], rtol=1e-3)
    for k in ('cls', 'reg', 'x'):
        for l, gr in enumerate(grads[k]):
            a = gr.cpu().numpy()
            want = base[f'{name}_g{k}_{l}'].copy()
            if k == 'reg':  # the fixture stores where it differs from GIoU's
                idx = g[f'{key}_greg_{l}_idx']
                want.reshape(-1)[idx] = g[f'{key}_greg_{l}_val']
                if l < 2:
                    assert idx.size, 'no positive anchor on this level?'
            np.testing.assert_allclose(a, want, rtol=5e-4, atol=1e-7,
                                       err_msg=f'{k}[{l}]')
            np.testing.assert_allclose(
                np.abs(a.astype(np.float64)).sum(),
                g[f'{key}_g{k}_abs_sum'][l], rtol=2e-4, atol=1e-7)


def test_lossblock_ciou_deterministic(golden):
    """Run twice, bitwise equal: the block has no float atomics."""
    _, batch, sizes, hi = _block_inputs(golden, 'small_crowd')
    a = _run_block(batch, sizes, hi, 'ciou', False)
    b = _run_block(batch, sizes, hi, 'ciou', False)
    assert torch.equal(a[0], b[0])
    for k in ('cls', 'reg', 'x'):
        for x, y in zip(a[1][k], b[1][k]):
            assert torch.equal(x, y)


# ------------------------------------------------------------------ heads ----
def _swap(head, dev, **cfg):
    from ld_amd import build_loss
    cfg.setdefault('loss_weight', head.loss_bbox.loss_weight)
    head.loss_bbox = build_loss(cfg).to(dev)
    return head


@pytest.mark.parametrize('family,typ', [('atss', 'CIoULoss'),
                                        ('fcos', 'CIoULoss'),
                                        ('fcos', 'IoULoss'),
                                        ('retina', 'CIoULoss')])
def test_side_heads_vs_reference(golden, family, typ):
    import test_gpu_atss
    import test_gpu_fcos
    import test_gpu_retina
    import test_oracle_atss
    import test_oracle_retina
    from ld_amd.heads import ATSS_LOSS_KEYS, RETINA_LOSS_KEYS
    dev = torch.device(DEV)
    mod = {'atss': test_gpu_atss, 'fcos': test_gpu_fcos,
           'retina': test_gpu_retina}[family]
    inputs = (test_oracle_retina if family == 'retina'
              else test_oracle_atss).inputs
    batch, sizes, hi = inputs(golden['lossblock_' + family], 'small')
    head = _swap(mod._head(dev), dev, type=typ)
    dv = {k: [t.to(dev) for t in v] for k, v in hi.items()}
    gtb = [b.to(dev) for b in batch['gt_bboxes']]
    gtl = [l.to(dev) for l in batch['gt_labels']]
    if family == 'retina':
        keys = RETINA_LOSS_KEYS
        losses = head.loss(dv['cls'], dv['reg'], gtb, gtl,
                           (dv['t_cls'], dv['t_reg']), batch['img_metas'])
    else:
        keys = ATSS_LOSS_KEYS
        losses = head.loss(dv['cls'], dv['reg'], dv['ctr'], gtb, gtl,
                           (dv['t_cls'], dv['t_reg'], None),
                           batch['img_metas'])
    got = torch.stack([torch.stack(losses[k]) for k in keys])
    got = got.detach().cpu().numpy().astype(np.float64)
    tag = 'ciou' if typ == 'CIoULoss' else 'iou'
    ref = golden['iou_losses'][f'lb_small_{family}_{tag}_losses']
    print(family, typ, 'loss_bbox', got[1], ref[1])
    np.testing.assert_allclose(got, ref, rtol=LOSS_RTOL, atol=LOSS_ATOL)


def test_fcos_gfl_head_default_is_iou_loss():
    """fcos_gfl_head.py:111: the constructor default trains."""
    from ld_amd.losses import IoULoss
    from ld_amd.registry import build_head
    head = build_head(dict(type='FCOSGFLHead', num_classes=80,
                           in_channels=256))
    assert isinstance(head.loss_bbox, IoULoss)
    head._check_loss_cfg()


def test_gfl_head_ciou_vs_reference(golden):
    """GFLHead.loss with CIoULoss, the teacher-training path of
    configs/gfl/gfl_r50_fpn_1x_coco.py:43: no distillation, so its three rows
    are the LDHead fixture's loss_cls / loss_bbox / loss_dfl."""
    from ld_amd import build_head
    from ld_amd.config import ConfigDict
    dev = torch.device(DEV)
    head = build_head(dict(
        type='GFLHead', num_classes=80, in_channels=256,
        loss_bbox=dict(type='CIoULoss', loss_weight=2.0),
        train_cfg=ConfigDict(assigner=dict(type='ATSSAssigner', topk=9),
                             allowed_border=-1, pos_weight=-1, debug=False),
        test_cfg=None)).to(dev)
    _, batch, sizes, hi = _block_inputs(golden, 'small')
    cls = [t.to(dev).requires_grad_(True) for t in hi['cls']]
    reg = [t.to(dev).requires_grad_(True) for t in hi['reg']]
    losses = head.loss(cls, reg, [b.to(dev) for b in batch['gt_bboxes']],
                       [l.to(dev) for l in batch['gt_labels']],
                       batch['img_metas'])
    assert list(losses.keys()) == LOSS_KEYS[:3]
    got = torch.stack([torch.stack(losses[k]) for k in LOSS_KEYS[:3]])
    got.sum().backward()
    ref = golden['iou_losses']['lb_small_ciou_losses'][:3]
    np.testing.assert_allclose(got.detach().cpu().numpy().astype(np.float64),
                               ref, rtol=LOSS_RTOL, atol=LOSS_ATOL)
    assert all(torch.isfinite(t.grad).all() for t in reg)
    assert float(reg[0].grad.abs().sum()) > 0


# ------------------------------------------------------------- whole step ----
def _voc(golden, dev):
    from ld_amd import model_zoo, synthetic
    g = golden['iou_losses']
    cfg = g['voc_cfg']
    pad, img_shape, bseed = tuple(cfg[:2]), tuple(cfg[2:4]), int(cfg[4])
    num_gt = [int(x) for x in g['voc_num_gt']]
    b = synthetic.synthetic_batch(len(num_gt), img_shape, pad, num_gt, bseed)
    det = model_zoo.build_seeded(model_zoo.ld_voc_detector(), dev)
    batch = dict(img=b['img'].to(dev), img_metas=b['img_metas'],
                 gt_bboxes=[x.to(dev) for x in b['gt_bboxes']],
                 gt_labels=[(x % 20).to(dev) for x in b['gt_labels']])
    return g, det, batch


def test_voc_ciou_train_step_vs_reference(golden):
    """One train step of configs/ld/ld_r18_gflv1_r101_fpn_voc_1x.py (the CIoU
    student) against the reference's: loss table, logged values, the gradient
    norm of every trainable parameter (bars of tests/test_gpu_e2e.py)."""
    g, det, batch = _voc(golden, torch.device(DEV))
    assert type(det.bbox_head.loss_bbox).__name__ == 'CIoULoss'
    losses = det(**batch)
    assert list(losses.keys()) == LOSS_KEYS
    table = torch.stack([torch.stack(losses[k]) for k in LOSS_KEYS])
    loss, log_vars = det._parse_losses(losses)
    loss.backward()
    torch.cuda.synchronize()
    got = table.detach().cpu().numpy().astype(np.float64)
    print('voc max |err|', np.abs(got - g['voc_losses']).max())
    np.testing.assert_allclose(got, g['voc_losses'], rtol=1e-4, atol=1e-4)
    for k, r in zip(LOSS_KEYS + ['loss'], g['voc_log_vars']):
        np.testing.assert_allclose(log_vars[k], r, rtol=1e-4, atol=1e-4,
                                   err_msg=k)
    params = dict(det.named_parameters())
    bad = []
    for k, r in zip([str(k) for k in g['voc_grad_names']],
                    g['voc_grad_norms']):
        assert params[k].grad is not None, k
        got_n = float(params[k].grad.double().norm())
        if not np.isclose(got_n, r, rtol=1e-3, atol=1e-6):
            bad.append((k, got_n, r))
    assert not bad, f'{len(bad)} grad norms off, first: {bad[:5]}'


def test_voc_ciou_step_list_equals_eager(golden):
    """The same step replayed through the step list: the same bits as eager."""
    from ld_amd.train import GraphedStep, SGDTrainer
    dev = torch.device(DEV)
    g, det, batch = _voc(golden, dev)
    eager = SGDTrainer(det, lr=0.00375)
    for i in range(3):
        out_e = eager.step(batch)
        if i == 0:  # the step of the fixture
            np.testing.assert_allclose(float(out_e['loss']),
                                       g['voc_log_vars'][-1], rtol=1e-4)
    torch.cuda.synchronize()
    _, det2, static = _voc(golden, dev)
    tr = SGDTrainer(det2, lr=0.00375)
    gs = GraphedStep(tr, static, warmup=2, launcher='list')
    out_g = gs.replay()
    torch.cuda.synchronize()
    assert torch.equal(tr.arena.flat_param, eager.arena.flat_param)
    assert torch.equal(tr.flat_momentum, eager.flat_momentum)
    assert dict(out_g['log_vars']) == dict(out_e['log_vars'])
    assert float(out_g['loss']) == float(out_e['loss'])
    assert np.isfinite(float(out_g['loss']))
