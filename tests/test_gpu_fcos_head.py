"""GPU (-m gpu): the plain FCOSHead -- Scale + exp / relu of the box maps in
one launch each way (ld_scale_act_levels_*), 4 activated distances per point
through the fused loss block (LD_LOSS_DIST), get_bboxes (LD_INFER_DIST),
test-time augmentation and whole train steps -- against the REFERENCE's own
FCOSHead outputs (tests/golden/fcos_head.npz, tools/gen_golden_fcos_head.py)
and a float64 autograd restatement (tests/_fcos_ref64.py).

Geometry: 2 images of 128 x 128, strides 8 .. 128, levels 16^2 .. 1^2, 4
classes, 8 feature channels, the default regress_ranges.  Cases
(synthetic.PLAIN_CASES): 'multi' -- positives on three levels (118 / 48 / 16,
with center_sampling 21 / 4 / 4), a point inside two GT boxes' ranges, and for
the relu variants a positive with four negative pre-activations and one with
exactly one; 'empty_img' -- an image without GT; 'no_pos' -- no positive in
the batch.

bf16 mode: ATSSHead's tests have no bf16 leg, so this file has none.

Before the feature every test here failed at the registry lookup of FCOSHead
(the module's autouse fixture builds the head first)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from ld_amd import synthetic as S

import _fcos_ref64 as R

pytestmark = pytest.mark.gpu

# the constants of tests/test_gpu_plain_heads.py
LOSS_TOL = dict(rtol=1e-4, atol=1e-4)
GRAD_TOL = dict(rtol=5e-4, atol=1e-7)
BOX_ATOL, SCORE_ATOL = 2e-3, 1e-6
EPS32 = 2.0 ** -23

CASES = [(v, c) for v in S.FCOS_VARIANTS for c in S.PLAIN_CASES
         if v == 'plain' or c == 'multi']
BBOX_LOSS = dict(IoULoss='iou', GIoULoss='giou', DIoULoss='diou',
                 CIoULoss='ciou')


@pytest.fixture(scope='module', autouse=True)
def fcos_head_registered():
    """Every test of this file is about FCOSHead: look it up first."""
    from ld_amd.registry import build_head
    return build_head(dict(
        type='FCOSHead', num_classes=S.PLAIN_CLASSES, in_channels=8,
        feat_channels=8, norm_cfg=dict(type='GN', num_groups=8,
                                       requires_grad=True)))


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                'golden', 'fcos_head.npz'))


def _head(dev, variant='plain', nms_pre=1000, small=True, **over):
    """The head of the zoo config; ``small``: 4 classes, 8 channels."""
    from ld_amd import model_zoo
    from ld_amd.config import ConfigDict
    from ld_amd.registry import build_head
    m = model_zoo.fcos_detector(50)
    cfg = dict(m['bbox_head'])
    if small:
        cfg.update(num_classes=S.PLAIN_CLASSES, in_channels=S.PLAIN_FEAT,
                   feat_channels=S.PLAIN_FEAT,
                   norm_cfg=dict(type='GN', num_groups=S.PLAIN_FEAT,
                                 requires_grad=True))
    cfg.update(S.FCOS_VARIANTS[variant])
    cfg.update(over)
    cfg.update(train_cfg=ConfigDict.wrap(m['train_cfg']),
               test_cfg=ConfigDict.wrap(dict(m['test_cfg'], nms_pre=nms_pre)))
    head = build_head(cfg).to(dev)
    with torch.no_grad():
        for s, v in zip(head.scales, S.FCOS_SCALES):
            s.scale.fill_(v)
    return head.train()


def _run_loss(head, case, dev):
    """head.loss on the fixture's conv outputs, the raw box maps going through
    the head's own Scale + activation launch: (keys, table (3, L), grads of
    cls / raw / ctr, grads of the scales (L,), inputs)."""
    from ld_amd import layers as Y
    batch = S.plain_batch(case, dev)
    if case == 'ragged':
        hi = S.fcos_head_inputs(S.RAGGED_SEED, device=dev,
                                relu=head.norm_on_bbox, pad=S.RAGGED_PAD)
    else:
        hi = S.fcos_head_inputs(S.PLAIN_SEEDS[case], device=dev,
                                relu=head.norm_on_bbox)
    for v in hi.values():
        for t in v:
            t.requires_grad_(True)
    for s in head.scales:
        s.scale.grad = None
    raw3, levels = Y.pack_levels(hi['raw'])
    reg = Y.split_levels(head._scale(raw3, levels), levels)
    losses = head.loss(hi['cls'], reg, hi['ctr'], batch['gt_bboxes'],
                       batch['gt_labels'], batch['img_metas'])
    table = torch.stack([torch.stack(v) for v in losses.values()])
    table.sum().backward()
    grads = {k: [t.grad.clone() for t in v] for k, v in hi.items()}
    gs = torch.stack([s.scale.grad.clone() for s in head.scales])
    return list(losses.keys()), table.detach(), grads, gs, hi


def _ref64(head, hi, bbox_loss=None):
    """tests/_fcos_ref64.fcos_loss on the kernels' own targets."""
    t = head.last_targets
    labels = t['labels'].cpu()
    targets = t['bbox_targets'].cpu().double()
    maps = {k: [x.detach().cpu().double().requires_grad_(True) for x in v]
            for k, v in hi.items()}
    scales = torch.tensor(S.FCOS_SCALES, dtype=torch.float64,
                          requires_grad=True)
    ref = R.fcos_loss(
        maps, scales, labels, targets, head.strides, head.num_classes,
        norm_on_bbox=head.norm_on_bbox,
        bbox_loss=bbox_loss or BBOX_LOSS[type(head.loss_bbox).__name__],
        eps=head.loss_bbox.eps, lw_bbox=head.loss_bbox.loss_weight)
    ref.sum().backward()
    return ref.detach(), maps, scales


def _pos_levels(head, pad=S.PLAIN_PAD):
    """Per level the (N, cells) mask of the positives."""
    lab = head.last_targets['labels'].cpu()
    off, pos = 0, []
    for h, w in S.level_shapes(pad):
        part = lab[:, off:off + h * w]
        pos.append((part >= 0) & (part < head.num_classes))
        off += h * w
    return pos


def _pos_per_level(head):
    return [int(p.sum()) for p in _pos_levels(head)]


def _check_grads(grads, gs, want, want_gs, what):
    for k, g_l in grads.items():
        for l, g in enumerate(g_l):
            np.testing.assert_allclose(g.cpu().numpy(), want(k, l),
                                       **GRAD_TOL,
                                       err_msg=f'{k}[{l}] vs {what}')
    # ds_l sums up to 2 * 4 * 256 products x * y' * dy that partly cancel: the
    # relative bar of the elements; the fp32 rounding of the terms (6e-8 of
    # each, their magnitudes summing to order 10) is 1e-6 absolute
    np.testing.assert_allclose(gs.cpu().numpy(), want_gs, rtol=5e-4,
                               atol=1e-6, err_msg=f'scales vs {what}')


@pytest.mark.parametrize('variant,case', CASES,
                         ids=[f'{v}-{c}' for v, c in CASES])
def test_loss_block_vs_reference_and_float64(variant, case, gold):
    dev = torch.device('cuda:0')
    head = _head(dev, variant)
    keys, table, grads, gs, hi = _run_loss(head, case, dev)
    assert keys == ['loss_cls', 'loss_bbox', 'loss_centerness']
    key = f'{variant}_{case}'
    got = table.cpu().numpy().astype(np.float64)
    print(f'{key}: max |loss - golden| '
          f'{np.abs(got.sum(1) - gold[key + "_losses"]).max():.3g}')
    # the reference returns one scalar per key: the sum over the levels
    np.testing.assert_allclose(got.sum(1), gold[key + '_losses'], **LOSS_TOL)
    assert _pos_per_level(head) == gold[key + '_pos'].tolist()
    _check_grads(grads, gs, lambda k, l: gold[f'{key}_g{k}_{l}'],
                 gold[key + '_gscales'], 'golden')
    ref, maps, scales = _ref64(head, hi)
    np.testing.assert_allclose(got, ref.numpy(), **LOSS_TOL)
    _check_grads(grads, gs, lambda k, l: maps[k][l].grad.numpy(),
                 scales.grad.numpy(), 'float64')
    if head.norm_on_bbox:
        n, l, y, x = S.FCOS_NEG['all']
        assert float(grads['raw'][l][n, :, y, x].abs().sum()) == 0.0
        n, l, y, x = S.FCOS_NEG['one']
        g = grads['raw'][l][n, :, y, x]
        assert float(g[S.FCOS_NEG_CH]) == 0.0 and int((g != 0).sum()) == 3
    if case == 'no_pos':
        # the values equal the golden (above) and nothing moves the box or the
        # centerness branch
        assert float(table[1:].abs().sum()) == 0.0
        assert all(float(g.abs().sum()) == 0.0
                   for k in ('raw', 'ctr') for g in grads[k])
        assert float(gs.abs().sum()) == 0.0
    if case == 'empty_img':
        assert all(float(g[1].abs().sum()) == 0.0
                   for k in ('raw', 'ctr') for g in grads[k])
    # every cell of the box gradient is written: zeros off the positives
    lab = head.last_targets['labels']
    off = 0
    for l, (h, w) in enumerate(S.level_shapes(S.PLAIN_PAD)):
        neg = ~((lab[:, off:off + h * w] >= 0) &
                (lab[:, off:off + h * w] < head.num_classes)).view(-1, 1, h, w)
        assert float((grads['raw'][l] * neg).abs().sum()) == 0.0
        off += h * w
    # a second run of the same step: the same bits
    _, table2, grads2, gs2, _ = _run_loss(head, case, dev)
    assert torch.equal(table, table2) and torch.equal(gs, gs2)
    for k in grads:
        for a, b_ in zip(grads[k], grads2[k]):
            assert torch.equal(a, b_)


@pytest.mark.parametrize('loss_type', list(BBOX_LOSS) + ['IoULoss-linear'])
def test_five_box_losses_vs_float64(loss_type):
    dev = torch.device('cuda:0')
    cfg = dict(type=loss_type.split('-')[0], loss_weight=1.5)
    mode = BBOX_LOSS[cfg['type']]
    if loss_type.endswith('-linear'):
        cfg['linear'], mode = True, 'iou_linear'
    head = _head(dev, 'plain', loss_bbox=cfg)
    _, table, grads, gs, hi = _run_loss(head, 'multi', dev)
    ref, maps, scales = _ref64(head, hi, bbox_loss=mode)
    print(f'{loss_type}: loss_bbox {table[1].sum().item():.6g} '
          f'float64 {ref[1].sum().item():.6g}')
    np.testing.assert_allclose(table.cpu().numpy(), ref.numpy(), **LOSS_TOL)
    _check_grads(grads, gs, lambda k, l: maps[k][l].grad.numpy(),
                 scales.grad.numpy(), 'float64')


def test_nonunit_upstream_rerun():
    """A weighted sum of the table entries (the rerun-with-upstream path of
    LDLossBlock.backward) scales each term's gradient."""
    dev = torch.device('cuda:0')
    head = _head(dev, 'tricks')
    from ld_amd import layers as Y
    batch = S.plain_batch('multi', dev)

    def run(w_cls, w_box, w_ctr):
        hi = S.fcos_head_inputs(71, device=dev, relu=True)
        for v in hi.values():
            for t in v:
                t.requires_grad_(True)
        raw3, levels = Y.pack_levels(hi['raw'])
        reg = Y.split_levels(head._scale(raw3, levels), levels)
        ls = head.loss(hi['cls'], reg, hi['ctr'], batch['gt_bboxes'],
                       batch['gt_labels'], batch['img_metas'])
        (w_cls * sum(ls['loss_cls']) + w_box * sum(ls['loss_bbox']) +
         w_ctr * sum(ls['loss_centerness'])).backward()
        return {k: [t.grad for t in v] for k, v in hi.items()}
    one, w = run(1.0, 1.0, 1.0), run(0.0, 3.0, 0.5)
    for l in range(5):
        np.testing.assert_allclose(w['raw'][l].cpu().numpy(),
                                   3.0 * one['raw'][l].cpu().numpy(),
                                   rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(w['ctr'][l].cpu().numpy(),
                                   0.5 * one['ctr'][l].cpu().numpy(),
                                   rtol=1e-6, atol=1e-12)
        assert float(w['cls'][l].abs().max()) == 0.0


# ------------------------------------------------- the activation kernels --
# 3 * 5 = 15 rows (no multiple of anything), 333 positions (two 256-thread
# blocks, the second partly empty), a level of 1 x 1
ACT_LEVELS = ((17, 19), (3, 3), (1, 1))
ACT_STRIDES = (8, 16, 32)


@pytest.mark.parametrize('mode', ['exp', 'relu', 'relu_stride'])
def test_scale_act_levels_vs_float64(mode):
    from ld_amd import layers as Y
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(17)
    P = sum(h * w for h, w in ACT_LEVELS)
    x = torch.randn(3, 5, P, generator=gen)
    # exact zeros, +0 and -0, at the ReLU kink; one per level
    x[0, 0, 0], x[1, 2, 17 * 19 + 4], x[2, 4, P - 1] = 0.0, -0.0, 0.0
    dy = torch.randn(3, 5, P, generator=gen)
    s = torch.tensor([0.75, 1.5, -1.25])

    def run():
        xd = x.to(dev).requires_grad_(True)
        sd = s.to(dev).requires_grad_(True)
        y = Y.scale_act_levels(xd, sd, ACT_LEVELS, mode, ACT_STRIDES)
        y.backward(dy.to(dev))
        return y.detach().cpu(), xd.grad.cpu(), sd.grad.cpu()
    y, dx, ds = run()
    x64 = x.double().requires_grad_(True)
    s64 = s.double().requires_grad_(True)
    lv, off = [], 0
    for h, w in ACT_LEVELS:
        lv.append(x64[:, :, off:off + h * w])
        off += h * w
    ref = torch.cat(R.activate(lv, s64, ACT_STRIDES, mode != 'exp',
                               training=mode != 'relu_stride'), dim=2)
    ref.backward(dy.double())
    umax = float((x.abs() * 1.5).max())
    # u = x * s is rounded once (half an ulp of u moves exp(u) by |u| / 2 ulp)
    # and expf is within 1 ulp; relu(u) [* stride] is one or two roundings
    rtol_y = (1.0 + 0.5 * umax) * EPS32 if mode == 'exp' else 2 * EPS32
    err = ((y.double() - ref.detach()).abs() /
           ref.detach().abs().clamp(min=1e-30)).max()
    print(f'{mode}: max rel err y {float(err):.3g} (bar {rtol_y:.3g})')
    np.testing.assert_allclose(y.numpy(), ref.detach().numpy(), rtol=rtol_y,
                               atol=0)
    # dx = s * (y' * dy): y' carries y's error, two more roundings
    np.testing.assert_allclose(dx.numpy(), x64.grad.numpy(),
                               rtol=rtol_y + 2 * EPS32, atol=0)
    # ds_l: fp64 sum of fp32 products x * (y' * dy); against the sum of the
    # terms' magnitudes
    terms = (x64.detach() * x64.grad / s64.detach()[
        torch.repeat_interleave(torch.arange(3), torch.tensor(
            [h * w for h, w in ACT_LEVELS]))]).abs()
    off = 0
    for l, (h, w) in enumerate(ACT_LEVELS):
        bar = (rtol_y + 2 * EPS32) * float(terms[:, :, off:off + h * w].sum())
        assert abs(float(ds[l]) - float(s64.grad[l])) <= bar + 1e-30, (l, bar)
        off += h * w
    # the kink: y = 0 and no gradient at exactly zero
    if mode != 'exp':
        for idx in ((0, 0, 0), (1, 2, 17 * 19 + 4), (2, 4, P - 1)):
            assert float(y[idx]) == 0.0 and float(dx[idx]) == 0.0
        assert float(y.min()) == 0.0
    if mode == 'relu_stride':
        y1 = Y.scale_act_levels(x.to(dev), s.to(dev), ACT_LEVELS, 'relu',
                                ACT_STRIDES).cpu()
        mul = torch.repeat_interleave(
            torch.tensor(ACT_STRIDES, dtype=torch.float32),
            torch.tensor([h * w for h, w in ACT_LEVELS]))
        assert torch.equal(y, y1 * mul)
    # two backwards: the same bits
    y2, dx2, ds2 = run()
    assert torch.equal(y, y2) and torch.equal(dx, dx2)
    assert torch.equal(ds, ds2)


# --------------------------------------------------- the real head's forward --
def _torch_head64(head, feats):
    """The head's convs in float64 torch ops from its state_dict: per-level
    cls, raw (conv_reg's output, before Scale and activation) and ctr."""
    import torch.nn.functional as F
    sd = {k: v.detach().cpu().double() for k, v in head.state_dict().items()}
    G = head.norm_cfg['num_groups']

    def tower(name, x):
        for i in range(head.stacked_convs):
            x = F.conv2d(x, sd[f'{name}.{i}.conv.weight'],
                         sd.get(f'{name}.{i}.conv.bias'), padding=1)
            x = F.relu(F.group_norm(x, G, sd[f'{name}.{i}.gn.weight'],
                                    sd[f'{name}.{i}.gn.bias'], eps=1e-5))
        return x

    def conv(name, x):
        return F.conv2d(x, sd[f'{name}.weight'], sd[f'{name}.bias'],
                        padding=1)
    maps = dict(cls=[], raw=[], ctr=[])
    for x in feats:
        cf, rf = tower('cls_convs', x), tower('reg_convs', x)
        maps['cls'].append(conv('conv_cls', cf))
        maps['raw'].append(conv('conv_reg', rf))
        maps['ctr'].append(conv('conv_centerness',
                                rf if head.centerness_on_reg else cf))
    scales = torch.stack([sd[f'scales.{l}.scale']
                          for l in range(len(feats))])
    return maps, scales


@pytest.mark.parametrize('variant', ['plain', 'tricks'])
def test_forward_vs_reference_and_feature_gradient(variant, gold):
    dev = torch.device('cuda:0')
    head = _head(dev, variant)
    head.load_state_dict({k: v.to(dev) for k, v in S.seeded_state_dict(
        head.state_dict(), seed=3).items()})
    assert head.centerness_on_reg == (variant == 'tricks')
    feats = S.fcos_feats(device=dev)
    # conv + GN + relu five layers deep in fp32 on both sides, 72-term dot
    # products in another order: ~5 * sqrt(72) * 2^-24 = 2.5e-6 of an
    # activation of order 1; the bar is the project's loss bar, 1e-4 relative,
    # with 1e-5 absolute for the outputs that relu or a small logit put near 0
    tol = dict(rtol=1e-4, atol=1e-5)
    for mode in (('train', ) if variant == 'plain' else ('train', 'eval')):
        head.train(mode == 'train')
        with torch.no_grad():
            outs = head(feats)
        for name, maps in zip(('cls', 'reg', 'ctr'), outs):
            assert len(maps) == 5
            for l, t in enumerate(maps):
                want = gold[f'fwd_{variant}_{mode}_{name}_{l}']
                assert tuple(t.shape) == want.shape
                np.testing.assert_allclose(
                    t.cpu().numpy(), want, **tol,
                    err_msg=f'{variant} {mode} {name}[{l}]')
    # the gradient of the summed losses of 'multi' to the features: the class
    # tower feeds conv_cls and (plain) conv_centerness, the reg tower conv_reg
    # and (tricks) conv_centerness -- two consumers each way, summed by the
    # fan-in protocol -- against float64 autograd through the same head
    head.train()
    batch = S.plain_batch('multi', dev)
    xs = [f.clone().requires_grad_(True) for f in feats]
    losses = head.loss(*head(xs), batch['gt_bboxes'], batch['gt_labels'],
                       batch['img_metas'])
    sum(sum(v) for v in losses.values()).backward()
    x64 = [f.detach().cpu().double().requires_grad_(True) for f in feats]
    maps, scales = _torch_head64(head, x64)
    t = head.last_targets
    R.fcos_loss(maps, scales, t['labels'].cpu(),
                t['bbox_targets'].cpu().double(), head.strides,
                head.num_classes, norm_on_bbox=head.norm_on_bbox,
                bbox_loss=BBOX_LOSS[type(head.loss_bbox).__name__],
                eps=head.loss_bbox.eps).sum().backward()
    for l, (a, b) in enumerate(zip(xs, x64)):
        got, want = a.grad.cpu().numpy(), b.grad.numpy()
        bad = np.abs(got - want) - (GRAD_TOL['atol'] +
                                    GRAD_TOL['rtol'] * np.abs(want))
        print(f'{variant} dfeat[{l}]: max |err| '
              f'{np.abs(got - want).max():.3g} of max |g| '
              f'{np.abs(want).max():.3g}, worst margin {bad.max():.3g}')
        assert np.abs(want).max() > 0
        np.testing.assert_allclose(got, want, **GRAD_TOL,
                                   err_msg=f'dfeat[{l}]')


# ------------------------------------------------------------- inference --
def test_get_bboxes_vs_reference(gold):
    dev = torch.device('cuda:0')
    head = _head(dev, nms_pre=S.PLAIN_INFER['nms_pre']).eval()
    hi, metas = S.fcos_infer_inputs(dev)
    outs = (hi['cls'], hi['reg'], hi['ctr'])
    for r in (0, 1):
        res = head.get_bboxes(*outs, metas, rescale=bool(r))
        for i, (dets, labels) in enumerate(res):
            gd = gold[f'r{r}_bboxes_{i}']
            assert labels.cpu().numpy().tolist() == \
                gold[f'r{r}_labels_{i}'].tolist()
            dets = dets.cpu().numpy()
            np.testing.assert_allclose(dets[:, :4], gd[:, :4], atol=BOX_ATOL,
                                       rtol=0)
            np.testing.assert_allclose(dets[:, 4], gd[:, 4], atol=SCORE_ATOL,
                                       rtol=0)
    # image 1 is smaller than the pad: the decode clipped to ITS shape
    h, w = S.PLAIN_INFER['img_shapes'][1][:2]
    pre = head.get_bboxes(*outs, metas, with_nms=False)
    assert float(pre[1][0][:, 2].max()) == w
    assert float(pre[1][0][:, 3].max()) == h
    assert float(pre[0][0][:, 2].max()) > w
    for i, rows in enumerate(pre):
        assert len(rows) == 3
        np.testing.assert_allclose(rows[0].cpu().numpy(),
                                   gold[f'pre_bboxes_{i}'], atol=BOX_ATOL,
                                   rtol=0)
        np.testing.assert_allclose(rows[1].cpu().numpy(),
                                   gold[f'pre_scores_{i}'], atol=SCORE_ATOL,
                                   rtol=0)
        np.testing.assert_allclose(rows[2].cpu().numpy(),
                                   gold[f'pre_factors_{i}'], atol=SCORE_ATOL,
                                   rtol=0)


def test_aug_test_equals_hand_merge():
    """aug_test over the image and its horizontal flip = ld_aug_merge_nms over
    the two views' get_bboxes(rescale=False, with_nms=False) rows."""
    from ld_amd import lossblock as LB
    dev = torch.device('cuda:0')
    head = _head(dev, 'tricks', nms_pre=100)
    head.load_state_dict({k: v.to(dev) for k, v in S.seeded_state_dict(
        head.state_dict(), seed=3).items()})
    with torch.no_grad():  # class scores above score_thr
        head.conv_cls.bias.fill_(-1.0)
    head.eval()
    x0 = S.fcos_feats(seed=9, num_imgs=1, device=dev)
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
            views.append(dict(boxes=res[0], scores=res[1], factors=res[2],
                              **m[0]))
        cfg = head.test_cfg
        d2, l2 = LB.aug_merge_nms(
            views, score_thr=cfg['score_thr'],
            iou_thr=cfg['nms']['iou_threshold'],
            max_per_img=cfg['max_per_img'], rescale=True,
            num_classes=S.PLAIN_CLASSES)
    assert dets.shape[0] > 0
    assert torch.equal(dets, d2) and torch.equal(labels, l2)
    # the eval-mode maps are pixels: boxes reach beyond one stride
    assert float((dets[:, 2] - dets[:, 0]).max()) > 8.0


def test_ragged_block_tails_vs_float64():
    """The dist form of tests/test_gpu_plain_heads.py::
    test_ragged_block_tails_vs_float64: synthetic.RAGGED_PAD's levels of 257,
    129, 65, 33 and 17 points end in a partly filled block after a full one.
    Positives in the second 256-block of level 0 and the second 64-block of
    level 2; image 1 has no GT.  Against float64 at this file's bars."""
    dev = torch.device('cuda:0')
    head = _head(dev)
    _, table, grads, gs, hi = _run_loss(head, 'ragged', dev)
    pos = _pos_levels(head, S.RAGGED_PAD)
    assert [p.shape[1] for p in pos] == [257, 129, 65, 33, 17]
    assert bool(pos[0][0, 256]) and bool(pos[0][0, :256].any())
    assert bool(pos[2][0, 64]) and bool(pos[2][0, :64].any())
    assert not any(bool(p[1].any()) for p in pos)
    ref, maps, scales = _ref64(head, hi)
    np.testing.assert_allclose(table.cpu().numpy().astype(np.float64),
                               ref.numpy(), **LOSS_TOL)
    _check_grads(grads, gs, lambda k, l: maps[k][l].grad.numpy(),
                 scales.grad.numpy(), 'float64')
    assert all(float(g[1].abs().sum()) == 0.0 for g in grads['raw'])
    # a second run of the same step: the same bits
    _, table2, grads2, gs2, _ = _run_loss(head, 'ragged', dev)
    assert torch.equal(table, table2) and torch.equal(gs, gs2)
    for k in grads:
        for a, b_ in zip(grads[k], grads2[k]):
            assert torch.equal(a, b_)


# ---------------------------------------------------- C entry points: EINVAL --
def test_entry_points_refuse_illegal_flag_combinations():
    from ld_amd import lib as L
    from ld_amd import lossblock as LB
    dev = torch.device('cuda:0')
    lib = L.get_lib()
    sizes = S.level_shapes(S.PLAIN_PAD)
    geom = L.make_geom(sizes, list(S.FCOS_STRIDES), 2, 8)
    A = geom.num_anchors
    hi = S.fcos_head_inputs(1, device=dev)
    reg = [r.exp() for r in hi['raw']]
    m_cls, m_reg = L.make_maps(hi['cls']), L.make_maps(reg)
    g_reg = [torch.zeros_like(r) for r in reg]
    mg_reg = L.make_maps(g_reg)
    labels = torch.full((2, A), S.PLAIN_CLASSES, dtype=torch.int64,
                        device=dev)
    tg = torch.zeros((2, A, 4), device=dev)
    counts = torch.zeros(2 + 2 * 5 + 1, dtype=torch.int32, device=dev)
    wt, score = torch.zeros((2, A), device=dev), torch.zeros((2, A),
                                                            device=dev)
    norm = torch.zeros(4, device=dev)
    ws = LB.workspace(dev, lib.ld_loss_workspace_bytes(C.byref(geom)),
                      'loss')
    ok = L.LD_LOSS_DIST | L.LD_LOSS_ATSS | L.LD_LOSS_FCOS

    def pre(flags, delta=None, anchors=None, geom=geom):
        hp = LB.make_hp(num_classes=S.PLAIN_CLASSES, flags=flags,
                        bbox_loss='iou', lw_ctr=1.0)
        return lib.ld_loss_plain_prepass(
            C.byref(geom), C.byref(hp),
            None if delta is None else C.byref(delta), L.ptr(anchors),
            L.ptr(labels), L.ptr(tg), L.ptr(counts), L.ptr(wt), L.ptr(score),
            L.ptr(norm), L.ptr(ws), ws.numel(), L.stream_ptr(dev))

    def pos(flags, delta=None, anchors=None, geom=geom):
        hp = LB.make_hp(num_classes=S.PLAIN_CLASSES, flags=flags,
                        bbox_loss='iou', lw_ctr=1.0)
        return lib.ld_loss_plain_pos(
            C.byref(geom), C.byref(hp),
            None if delta is None else C.byref(delta), L.ptr(anchors),
            C.byref(m_cls), C.byref(m_reg), L.ptr(labels), L.ptr(tg),
            L.ptr(score), L.ptr(norm), None, C.byref(mg_reg), L.ptr(ws),
            ws.numel(), L.stream_ptr(dev))
    assert pre(ok) == 0 and pos(ok) == 0
    assert pre(ok | L.LD_LOSS_DIST_NORM) == 0
    bad = [L.LD_LOSS_DIST, L.LD_LOSS_DIST | L.LD_LOSS_ATSS,
           L.LD_LOSS_DIST | L.LD_LOSS_FCOS, L.LD_LOSS_ATSS | L.LD_LOSS_FCOS,
           ok | L.LD_LOSS_DELTA, ok | L.LD_LOSS_RETINA,
           ok | L.LD_LOSS_PROB_CLS,
           L.LD_LOSS_ATSS | L.LD_LOSS_FCOS | L.LD_LOSS_DIST_NORM]
    for flags in bad:
        assert pre(flags) == -1, flags   # LD_EINVAL
        assert pos(flags) == -1, flags
    # the delta side: `delta` is non-null exactly with LD_LOSS_DELTA
    atss = L.LD_LOSS_ATSS | L.LD_LOSS_DELTA
    from ld_amd.core import DeltaXYWHBBoxCoder
    coder = DeltaXYWHBBoxCoder(*S.PLAIN_CODERS['atss'])
    dc = coder.delta_t()
    assert pre(atss, dc) == 0 and pos(atss, dc) == 0
    assert pre(atss) == -1 and pos(atss) == -1
    assert pre(ok, dc) == -1 and pos(ok, dc) == -1
    # L1 on the deltas is RetinaHead's alone
    l1 = coder.delta_t(box_term='l1')
    assert pre(atss, l1) == -1 and pos(atss, l1) == -1
    # explicit anchors: whole images of num_base pseudo-images each
    b3 = DeltaXYWHBBoxCoder(*S.PLAIN_CODERS['retina']).delta_t(num_base=3)
    anchors = torch.zeros((A * 3, 4), device=dev)
    retina = L.LD_LOSS_RETINA | L.LD_LOSS_DELTA
    assert geom.num_imgs == 2
    assert pre(retina, b3, anchors) == -1 and pos(retina, b3, anchors) == -1
    b2 = DeltaXYWHBBoxCoder(*S.PLAIN_CODERS['retina']).delta_t(num_base=2)
    assert pre(retina, b2, anchors) == 0 and pos(retina, b2, anchors) == 0
    # the distribution prepass does not read 4-channel maps
    hp = LB.make_hp(num_classes=S.PLAIN_CLASSES, flags=ok, bbox_loss='iou')
    assert lib.ld_loss_prepass_ex(
        C.byref(geom), C.byref(hp), C.byref(m_cls), C.byref(m_reg),
        L.ptr(labels), L.ptr(tg), L.ptr(wt), L.ptr(counts), L.ptr(wt),
        L.ptr(score), L.ptr(norm), L.ptr(ws), ws.numel(),
        L.stream_ptr(dev)) == -1
    torch.cuda.synchronize()
    # inference: LD_INFER_DIST only with LD_INFER_POINTS and num_base = 1
    head = _head(dev, nms_pre=100)
    hi2, metas = S.fcos_infer_inputs(dev)
    kw = dict(strides=list(S.FCOS_STRIDES),
              img_shapes=[m['img_shape'] for m in metas], nms_pre=100,
              centernesses=hi2['ctr'])
    LB.get_bboxes(hi2['cls'], hi2['reg'], points=True, dist=True, **kw)
    with pytest.raises(L.LdError, match='LD_EINVAL'):
        LB.get_bboxes(hi2['cls'], hi2['reg'], points=False, dist=True, **kw)
    with pytest.raises(L.LdError, match='LD_EINVAL'):
        LB.get_bboxes(hi2['cls'], hi2['reg'], points=False, dist=True,
                      with_nms=False, **kw)
    with pytest.raises(L.LdError, match='LD_EINVAL'):
        LB.get_bboxes([torch.cat([c, c], 1) for c in hi2['cls']],
                      [torch.cat([r, r], 1) for r in hi2['reg']],
                      points=True, dist=True, num_base=2,
                      **dict(kw, centernesses=None))
    # the activation entry points: mode, strides
    from ld_amd import layers as Y
    lv = Y.levels_desc(ACT_LEVELS)
    x = torch.zeros(2, 333, device=dev)
    s = torch.ones(3, device=dev)
    st = (C.c_int32 * 3)(8, 16, 32)
    for mode, strides in ((3, st), (-1, st), (2, None),
                          (2, (C.c_int32 * 3)(8, 0, 32))):
        assert lib.ld_scale_act_levels_forward(
            C.byref(lv), L.ptr(x), L.ptr(s), strides, mode, 2, L.ptr(x),
            L.stream_ptr(dev)) == -1
    assert head is not None


# ------------------------------------------------------------ whole steps --
def _det(tricks, dev):
    from ld_amd import build_detector, model_zoo
    det = build_detector(model_zoo.fcos_detector(50, tricks=tricks))
    det.load_state_dict(S.seeded_state_dict(det.state_dict(), seed=1))
    return det.to(dev).train()


def _batch(seed, num_gt, dev):
    b = S.synthetic_batch(2, (128, 128), (128, 128), num_gt, seed)
    return dict(img=b['img'].to(dev), img_metas=b['img_metas'],
                gt_bboxes=[x.to(dev) for x in b['gt_bboxes']],
                gt_labels=[x.to(dev) for x in b['gt_labels']])


@pytest.mark.parametrize('tricks', [False, True], ids=['plain', 'tricks'])
def test_train_step_eager_list_graph_bit_identical(tricks):
    """SGDTrainer steps of fcos_detector(50) at 2 x 3 x 128 x 128: the eager
    step, the step-list replay and the hipGraph replay leave the same bits,
    over three batches with different GT counts, one of them without a box
    (GraphedStep.dynamic_gt: the point targets read the padded buffers)."""
    from ld_amd.train import GraphedStep, SGDTrainer
    dev = torch.device('cuda:0')
    batches = [_batch(41, [3, 2], dev), _batch(42, [1, 5], dev),
               _batch(43, [0, 0], dev)]
    eager = SGDTrainer(_det(tricks, dev), lr=0.01)
    before = eager.arena.flat_param.clone()
    outs_e = [eager.step(d) for d in [batches[0]] + batches]
    torch.cuda.synchronize()
    logs = dict(outs_e[1]['log_vars'])
    assert sorted(logs) == ['loss', 'loss_bbox', 'loss_centerness',
                            'loss_cls']
    assert all(np.isfinite(v) and v > 0 for v in logs.values())
    assert dict(outs_e[3]['log_vars'])['loss_bbox'] == 0.0
    assert not torch.equal(before, eager.arena.flat_param)
    assert bool(torch.isfinite(eager.arena.flat_param).all())
    for launcher in ('list', 'graph'):
        tr = SGDTrainer(_det(tricks, dev), lr=0.01)
        g = GraphedStep(tr, _batch(41, [3, 2], dev), warmup=1, max_gt=8,
                        launcher=launcher)
        assert g.dynamic_gt
        out_g = g.replay()
        for d in batches[1:]:
            g.copy_inputs(d)
            out_g = g.replay()
        torch.cuda.synchronize()
        assert torch.equal(tr.arena.flat_param, eager.arena.flat_param), \
            launcher
        assert torch.equal(tr.flat_momentum, eager.flat_momentum), launcher
        assert float(out_g['loss']) == float(outs_e[-1]['loss'])
        assert dict(out_g['log_vars']) == dict(outs_e[-1]['log_vars'])
