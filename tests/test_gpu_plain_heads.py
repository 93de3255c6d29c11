"""GPU (-m gpu): the plain ATSSHead / RetinaHead -- 4 DeltaXYWH channels per
anchor through the fused loss block (LD_LOSS_DELTA), get_bboxes
(LD_INFER_DELTA), test-time augmentation and a whole train step -- against the
REFERENCE's own ATSSHead / RetinaHead outputs (tests/golden/plain_heads.npz,
tools/gen_golden_plain_heads.py) and a float64 autograd restatement
(tests/_plain_ref64.py).

Geometry: 2 images of 128 x 128, five levels 16^2 .. 1^2, 4 classes.  Cases
(synthetic.PLAIN_CASES): 'multi' -- ATSS positives on three levels, RetinaNet
positives on four with 247 anchors in the ignore band, one positive per head
whose predicted dw sits beyond the clamp; 'empty_img' -- an image without GT;
'no_pos' -- no positive in the batch (bbox_avg_factor < EPS -> 1).

Before the feature every test here failed at the registry lookup of ATSSHead /
RetinaHead / L1Loss."""
import os

import numpy as np
import pytest
import torch

from ld_amd import synthetic as S

import _plain_ref64 as R

pytestmark = pytest.mark.gpu

# the project's bar for losses (tests/test_gpu_lossblock.py LOSS_RTOL / ATOL,
# tests/test_gpu_atss.py:63, tests/test_gpu_retina.py:121)
LOSS_TOL = dict(rtol=1e-4, atol=1e-4)
# gradient maps, element-wise: tests/test_gpu_lossblock.py:227-228
GRAD_TOL = dict(rtol=5e-4, atol=1e-7)

VARIANTS = {
    'atss': ('atss', {}, 'decoded', 2.0, 1.0),
    'retina_l1': ('retina', {}, 'l1', 1.0, 1.0),
    'retina_sl1': ('retina', dict(loss_bbox=dict(
        type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0)), 'smooth_l1',
        1.0, 1.0 / 9.0),
    'retina_giou': ('retina', dict(reg_decoded_bbox=True, loss_bbox=dict(
        type='GIoULoss', loss_weight=2.0)), 'decoded', 2.0, 1.0),
}
LOSS_CASES = [(t, c) for c in S.PLAIN_CASES for t in ('atss', 'retina_l1')] + \
    [('retina_sl1', 'multi'), ('retina_giou', 'multi')]


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                'golden', 'plain_heads.npz'))


def _head(kind, dev, nms_pre=1000, small=True, **over):
    """The head of the zoo config; ``small``: 4 classes, 8 channels (the
    loss and get_bboxes tests feed it head outputs, its convs never run)."""
    from ld_amd import model_zoo
    from ld_amd.config import ConfigDict
    from ld_amd.registry import build_head
    m = (model_zoo.atss_detector if kind == 'atss'
         else model_zoo.retinanet_detector)(50)
    cfg = dict(m['bbox_head'])
    if small:
        cfg.update(num_classes=S.PLAIN_CLASSES, in_channels=S.PLAIN_FEAT,
                   feat_channels=S.PLAIN_FEAT)
        if kind == 'atss':
            cfg['norm_cfg'] = dict(type='GN', num_groups=S.PLAIN_FEAT,
                                   requires_grad=True)
    cfg.update(over)
    cfg.update(train_cfg=ConfigDict.wrap(m['train_cfg']),
               test_cfg=ConfigDict.wrap(dict(m['test_cfg'], nms_pre=nms_pre)))
    return build_head(cfg).to(dev)


def _outs(kind, hi):
    return [hi['cls'], hi['reg']] + ([hi['ctr']] if kind == 'atss' else [])


def _run_loss(kind, head, case, dev):
    batch = S.plain_batch(case, dev)
    if case == 'ragged':
        hi = S.plain_head_inputs(kind, S.RAGGED_SEED, device=dev, clamp=False,
                                 pad=S.RAGGED_PAD)
    else:
        hi = S.plain_head_inputs(kind, S.PLAIN_SEEDS[case], device=dev)
    for v in hi.values():
        for t in v:
            t.requires_grad_(True)
    losses = head.loss(*_outs(kind, hi), batch['gt_bboxes'],
                       batch['gt_labels'], batch['img_metas'])
    table = torch.stack([torch.stack(v) for v in losses.values()])
    table.sum().backward()
    grads = {k: [t.grad.clone() for t in v] for k, v in hi.items()}
    return list(losses.keys()), table.detach(), grads, hi


def _ref_targets(head, kind, C, pad=S.PLAIN_PAD):
    """head.last_targets (the kernels' (N * B, A) arrays) in the row order of
    the reference: per level (image, cell, base anchor)."""
    t = head.last_targets
    B = head.num_anchors
    NB, A = t['labels'].shape
    N = NB // B
    lab = t['labels'].view(N, B, A).cpu()
    wts = t['label_weights'].view(N, B, A).cpu().double()
    gts = t['bbox_targets'].view(N, B, A, 4).cpu().double()
    levels, off = [], 0
    for (h, w) in S.level_shapes(pad):
        n = h * w
        levels.append(dict(
            labels=lab[:, :, off:off + n].permute(0, 2, 1).reshape(-1),
            weights=wts[:, :, off:off + n].permute(0, 2, 1).reshape(-1),
            gts=gts[:, :, off:off + n].permute(0, 2, 1, 3).reshape(-1, 4)))
        off += n
    pos = ((lab >= 0) & (lab < C)).reshape(N, -1).sum(1).tolist()
    return dict(levels=levels, num_pos_img=pos)


def _check_float64(tag, head, hi, t, got, grads, pad):
    """Loss table and every gradient map against tests/_plain_ref64.py on the
    kernels' own targets ``t``; -> the float64 maps with their gradients."""
    kind, _, box_term, lw_bbox, beta = VARIANTS[tag]
    anchors = [a.cpu().double() for a in head.anchor_generator.grid_anchors(
        S.level_shapes(pad), hi['cls'][0].device)]
    maps = {k: [x.detach().cpu().double().requires_grad_(True) for x in v]
            for k, v in hi.items()}
    ref = R.plain_loss(kind, maps, t, anchors, S.PLAIN_CLASSES,
                       S.PLAIN_CODERS[kind], box_term, lw_bbox, beta)
    ref.sum().backward()
    np.testing.assert_allclose(got, ref.detach().numpy(), **LOSS_TOL)
    for k, gs in grads.items():
        for l, g in enumerate(gs):
            np.testing.assert_allclose(g.cpu().numpy(),
                                       maps[k][l].grad.numpy(), **GRAD_TOL,
                                       err_msg=f'{k}[{l}] vs float64')
    return maps


@pytest.mark.parametrize('tag,case', LOSS_CASES,
                         ids=[f'{t}-{c}' for t, c in LOSS_CASES])
def test_loss_block_vs_reference_and_float64(tag, case, gold):
    kind, over, box_term, lw_bbox, beta = VARIANTS[tag]
    dev = torch.device('cuda:0')
    head = _head(kind, dev, **over)
    keys, table, grads, hi = _run_loss(kind, head, case, dev)
    assert keys == ['loss_cls', 'loss_bbox'] + \
        (['loss_centerness'] if kind == 'atss' else [])
    key = f'{tag}_{case}'
    got = table.cpu().numpy().astype(np.float64)
    print(f'{key}: max |loss - golden| '
          f'{np.abs(got - gold[key + "_losses"]).max():.3g}')
    np.testing.assert_allclose(got, gold[key + '_losses'], **LOSS_TOL)
    # the kernels' targets are the reference's: positives per level
    C = S.PLAIN_CLASSES
    t = _ref_targets(head, kind, C)
    pos = [int(((lv['labels'] >= 0) & (lv['labels'] < C)).sum())
           for lv in t['levels']]
    assert pos == gold[key + '_pos'].tolist()
    assert sum(int((lv['weights'] == 0).sum()) for lv in t['levels']) == \
        int(gold[key + '_ignored'])
    # gradients against the reference's, element-wise
    for k, gs in grads.items():
        for l, g in enumerate(gs):
            np.testing.assert_allclose(g.cpu().numpy(),
                                       gold[f'{key}_g{k}_{l}'], **GRAD_TOL,
                                       err_msg=f'{k}[{l}] vs golden')
    # ... and against float64 autograd on the same targets
    maps = _check_float64(tag, head, hi, t, got, grads, S.PLAIN_PAD)
    if case == 'multi':
        # the positive whose dw sits beyond the clamp: exactly zero gradient
        # there, as in the reference (decoded box losses).  The clamped box
        # spans the target's width, so its GIoU does not move with dx either;
        # dy and dh still learn.  L1 / SmoothL1 act on the raw deltas and know
        # no clamp.
        n, l, y, x, b, v = S.PLAIN_CLAMP[kind]
        g = grads['reg'][l][n, b * 4:b * 4 + 4, y, x].cpu().numpy()
        want = gold[f'{key}_greg_{l}'][n, b * 4:b * 4 + 4, y, x]
        assert float(hi['reg'][l][n, b * 4 + 2, y, x]) == v
        if box_term == 'decoded':
            assert g[2] == 0.0 and want[2] == 0.0
            assert g[1] != 0.0 and g[3] != 0.0
            assert maps['reg'][l].grad[n, b * 4 + 2, y, x] == 0.0
        else:
            assert g[2] != 0.0 and want[2] != 0.0
    if case == 'no_pos':
        assert float(table[1:].abs().sum()) == 0.0
        assert all(float(g.abs().sum()) == 0.0 for g in grads['reg'])
    # a second run of the same step: the same bits
    _, table2, grads2, _ = _run_loss(kind, head, case, dev)
    assert torch.equal(table, table2)
    for k in grads:
        for a, b_ in zip(grads[k], grads2[k]):
            assert torch.equal(a, b_)


@pytest.mark.parametrize('tag', ['atss', 'retina_l1'])
def test_ragged_block_tails_vs_float64(tag):
    """The plain prepass (64 cells per block) and positives kernel (256) on
    synthetic.RAGGED_PAD, whose levels of 257, 129, 65, 33 and 17 cells end in
    a partly filled block after a full one -- the PLAIN_PAD levels (256, 64,
    16, 4, 1 cells) never do.  Positives sit in the second 256-block of level
    0 and the second 64-block of level 2; image 1 has no GT.  Against float64
    at this file's bars.  (FCOSHead: tests/test_gpu_fcos_head.py.)"""
    kind = VARIANTS[tag][0]
    dev = torch.device('cuda:0')
    head = _head(kind, dev, **VARIANTS[tag][1])
    _, table, grads, hi = _run_loss(kind, head, 'ragged', dev)
    C = S.PLAIN_CLASSES
    t = _ref_targets(head, kind, C, S.RAGGED_PAD)
    sizes = S.level_shapes(S.RAGGED_PAD)
    assert [h * w for h, w in sizes] == [257, 129, 65, 33, 17]

    def pos_cells(l):  # rows of a level: (image, cell, base anchor)
        lab = t['levels'][l]['labels']
        rows = ((lab >= 0) & (lab < C)).nonzero()[:, 0]
        return (rows // head.num_anchors) % (sizes[l][0] * sizes[l][1])
    assert int(pos_cells(0).max()) >= 256 and int(pos_cells(0).min()) < 256
    assert int(pos_cells(2).max()) >= 64 and int(pos_cells(2).min()) < 64
    assert t['num_pos_img'][0] > 0 and t['num_pos_img'][1] == 0
    got = table.cpu().numpy().astype(np.float64)
    _check_float64(tag, head, hi, t, got, grads, S.RAGGED_PAD)
    assert all(float(g[1].abs().sum()) == 0.0 for g in grads['reg'])
    # a second run of the same step: the same bits
    _, table2, grads2, _ = _run_loss(kind, head, 'ragged', dev)
    assert torch.equal(table, table2)
    for k in grads:
        for a, b_ in zip(grads[k], grads2[k]):
            assert torch.equal(a, b_)


def test_nonunit_upstream_rerun():
    """A weighted sum of the table entries (the rerun-with-upstream path of
    LDLossBlock.backward) scales each term's gradient."""
    dev = torch.device('cuda:0')
    head = _head('atss', dev)
    batch = S.plain_batch('multi', dev)

    def run(w_cls, w_box, w_ctr):
        hi = S.plain_head_inputs('atss', 71, device=dev)
        for v in hi.values():
            for t in v:
                t.requires_grad_(True)
        ls = head.loss(*_outs('atss', hi), batch['gt_bboxes'],
                       batch['gt_labels'], batch['img_metas'])
        (w_cls * sum(ls['loss_cls']) + w_box * sum(ls['loss_bbox']) +
         w_ctr * sum(ls['loss_centerness'])).backward()
        return {k: [t.grad for t in v] for k, v in hi.items()}
    one, w = run(1.0, 1.0, 1.0), run(0.0, 3.0, 0.5)
    for l in range(5):
        np.testing.assert_allclose(w['reg'][l].cpu().numpy(),
                                   3.0 * one['reg'][l].cpu().numpy(),
                                   rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(w['ctr'][l].cpu().numpy(),
                                   0.5 * one['ctr'][l].cpu().numpy(),
                                   rtol=1e-6, atol=1e-12)
        assert float(w['cls'][l].abs().max()) == 0.0


# ------------------------------------------------------------- inference --
# tests/test_gpu_infer.py:212-214 (GFL heads): boxes 2e-3 px, scores 1e-6
BOX_ATOL, SCORE_ATOL = 2e-3, 1e-6


@pytest.mark.parametrize('kind', ['atss', 'retina'])
def test_get_bboxes_vs_reference(kind, gold):
    dev = torch.device('cuda:0')
    head = _head(kind, dev, nms_pre=S.PLAIN_INFER['nms_pre'])
    hi, metas = S.plain_infer_inputs(kind, dev)
    for r in (0, 1):
        res = head.get_bboxes(*_outs(kind, hi), metas, rescale=bool(r))
        for i, (dets, labels) in enumerate(res):
            gd = gold[f'{kind}_r{r}_bboxes_{i}']
            assert labels.cpu().numpy().tolist() == \
                gold[f'{kind}_r{r}_labels_{i}'].tolist()
            dets = dets.cpu().numpy()
            np.testing.assert_allclose(dets[:, :4], gd[:, :4], atol=BOX_ATOL,
                                       rtol=0)
            np.testing.assert_allclose(dets[:, 4], gd[:, 4], atol=SCORE_ATOL,
                                       rtol=0)
    # image 1 is smaller than the pad: the decode clipped to ITS shape
    h, w = S.PLAIN_INFER['img_shapes'][1][:2]
    d1 = head.get_bboxes(*_outs(kind, hi), metas)[1][0]
    assert float(d1[:, 2].max()) <= w and float(d1[:, 3].max()) <= h
    pre = head.get_bboxes(*_outs(kind, hi), metas, with_nms=False)
    for i, rows in enumerate(pre):
        assert len(rows) == (3 if kind == 'atss' else 2)
        np.testing.assert_allclose(rows[0].cpu().numpy(),
                                   gold[f'{kind}_pre_bboxes_{i}'],
                                   atol=BOX_ATOL, rtol=0)
        np.testing.assert_allclose(rows[1].cpu().numpy(),
                                   gold[f'{kind}_pre_scores_{i}'],
                                   atol=SCORE_ATOL, rtol=0)
        if kind == 'atss':
            np.testing.assert_allclose(rows[2].cpu().numpy(),
                                       gold[f'{kind}_pre_factors_{i}'],
                                       atol=SCORE_ATOL, rtol=0)


@pytest.mark.parametrize('kind', ['atss', 'retina'])
def test_aug_test_equals_hand_merge(kind):
    """aug_test over the image and its horizontal flip = ld_aug_merge_nms over
    the two views' get_bboxes(rescale=False, with_nms=False) rows."""
    from ld_amd import lossblock as LB
    dev = torch.device('cuda:0')
    head = _head(kind, dev, nms_pre=100, small=False)  # the config's head
    head.load_state_dict(S.seeded_state_dict(head.state_dict(), seed=3))
    head.eval()
    gen = torch.Generator().manual_seed(9)
    sizes = S.level_shapes(S.PLAIN_PAD)
    x0 = [torch.randn(1, 256, h, w, generator=gen).to(dev)
          for h, w in sizes]
    feats = [x0, [t.flip(-1) for t in x0]]
    shape = (128, 120, 3)
    sf = np.array([1.25] * 4, dtype=np.float32)
    metas = [[dict(img_shape=shape, scale_factor=sf, flip=False,
                   flip_direction=None)],
             [dict(img_shape=shape, scale_factor=sf, flip=True,
                   flip_direction='horizontal')]]
    with torch.no_grad():
        _, (dets, labels) = head.aug_test(feats, metas, rescale=True,
                                          return_device_dets=True)
        views = []
        for x, m in zip(feats, metas):
            res = head.get_bboxes(*head(x), m, rescale=False,
                                  with_nms=False)[0]
            views.append(dict(boxes=res[0], scores=res[1],
                              factors=res[2] if len(res) > 2 else None,
                              **m[0]))
        cfg = head.test_cfg
        d2, l2 = LB.aug_merge_nms(
            views, score_thr=cfg['score_thr'],
            iou_thr=cfg['nms']['iou_threshold'],
            max_per_img=cfg['max_per_img'], rescale=True, num_classes=80)
    assert dets.shape[0] > 0
    assert torch.equal(dets, d2) and torch.equal(labels, l2)


# ------------------------------------------------------------ whole step --
def _det(kind, dev):
    from ld_amd import build_detector, model_zoo
    make = model_zoo.atss_detector if kind == 'atss' \
        else model_zoo.retinanet_detector
    det = build_detector(make(18))
    det.load_state_dict(S.seeded_state_dict(det.state_dict(), seed=1))
    return det.to(dev).train()


def _batch(seed, num_gt, dev):
    b = S.synthetic_batch(2, (128, 128), (128, 128), num_gt, seed)
    return dict(img=b['img'].to(dev), img_metas=b['img_metas'],
                gt_bboxes=[x.to(dev) for x in b['gt_bboxes']],
                gt_labels=[x.to(dev) for x in b['gt_labels']])


@pytest.mark.parametrize('kind', ['atss', 'retina'])
def test_detector_step_equals_head_level_losses(kind):
    """One SGDTrainer step of the seeded R18 detector at 2 x 3 x 128 x 128; its
    logged losses are the head's on the same features."""
    from ld_amd.train import SGDTrainer
    dev = torch.device('cuda:0')
    det = _det(kind, dev)
    d = _batch(41, [3, 2], dev)
    # the train-mode forward the step itself runs, no backward
    feats = det.extract_feat(d['img'])
    ls = det.bbox_head.forward_train(feats, d['img_metas'], d['gt_bboxes'],
                                     d['gt_labels'])
    want = {k: float(sum(v).detach()) for k, v in ls.items()}
    del feats, ls
    assert list(want) == ['loss_cls', 'loss_bbox'] + \
        (['loss_centerness'] if kind == 'atss' else [])
    tr = SGDTrainer(det, lr=0.01)
    before = tr.arena.flat_param.clone()
    out = tr.step(d)
    torch.cuda.synchronize()
    logs = dict(out['log_vars'])
    for k, v in want.items():
        assert np.isfinite(v) and v > 0
        np.testing.assert_allclose(logs[k], v, rtol=1e-6)
    np.testing.assert_allclose(logs['loss'], sum(want.values()), rtol=1e-6)
    assert not torch.equal(before, tr.arena.flat_param)
    assert bool(torch.isfinite(tr.arena.flat_param).all())


def test_atss_graphed_step_list_equals_eager():
    """ATSSHead uses the ATSS targets kernel, so a captured step takes batches
    with different GT counts (GraphedStep.dynamic_gt): the 'list' replay must
    leave the same bits as eager steps on the same two batches."""
    from ld_amd.train import GraphedStep, SGDTrainer
    dev = torch.device('cuda:0')
    d1, d2 = _batch(41, [3, 2], dev), _batch(42, [1, 5], dev)
    eager = SGDTrainer(_det('atss', dev), lr=0.01)
    for d in (d1, d1, d2):
        out_e = eager.step(d)
    torch.cuda.synchronize()
    tr = SGDTrainer(_det('atss', dev), lr=0.01)
    g = GraphedStep(tr, _batch(41, [3, 2], dev), warmup=1, max_gt=8,
                    launcher='list')
    assert g.dynamic_gt
    g.replay()
    g.copy_inputs(d2)
    out_g = g.replay()
    torch.cuda.synchronize()
    assert torch.equal(tr.arena.flat_param, eager.arena.flat_param)
    assert torch.equal(tr.flat_momentum, eager.flat_momentum)
    assert float(out_g['loss']) == float(out_e['loss'])
    assert dict(out_g['log_vars']) == dict(out_e['log_vars'])
