"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/iou_losses.npz by EXECUTING THE
REFERENCE's IoU / DIoU / CIoU losses on CPU (the reference package is imported,
unmodified, through oracle/ref_shim.py).  Run from the repo root in the build
container, never on the GPU machine:

    python tools/gen_golden_iou_losses.py

Reference entry points exercised (file:line under the reference tree):
  mmdet/models/losses/iou_loss.py:14-36,222-288   iou_loss / IoULoss
  mmdet/models/losses/iou_loss.py:107-157,363-398 diou_loss / DIoULoss
  mmdet/models/losses/iou_loss.py:162-219,401-436 ciou_loss / CIoULoss
  mmdet/models/dense_heads/ld_head.py:116-375     LDHead.loss
  mmdet/models/dense_heads/ld_atss.py / ld_fcos_head.py / ld_retina.py  .loss
  mmdet/models/detectors/kd_one_stage.py:46-81    forward_train
  (configs/ld/ld_r18_gflv1_r101_fpn_voc_1x.py, the CIoU student)

Only reference outputs and the hand-written boxes are stored; every other input
is regenerated from seeds (ld_amd.synthetic).

ROWS -- ``rows_hand`` (H, 2, 4): hand-written (pred, target) pairs, listed at
HAND below; rows H..256 are synthetic.box_loss_rows(257 - H, ROWS_SEED).  Per
loss L in iou, iou_linear, diou, ciou (modules with their default eps = 1e-6,
loss_weight = 1, reduction_override='none'):
  L_loss64 (257,), L_grad64 (257, 4)  the reference run on float64 tensors
  L_loss32, L_grad32                  the reference run on float32 tensors
  L_loss_ref32_dev, L_grad_ref32_dev  the reference's own fp32-vs-float64
      deviation: max over elements of (|x32 - x64| - atol) / |x64|, floored at 0,
      i.e. the smallest rtol its fp32 run meets at the project's atol (ATOL_LOSS
      for values, ATOL_GRAD for gradients)
ATOL_LOSS = 5e-7: every loss here is 1 - x or -log(x) with x <= 1 formed by
float32 operations, so a value near 0 carries the absolute rounding error of
x (half an ulp of 1 = 6e-8 per operation, a handful of operations) whatever its
own magnitude.  ATOL_GRAD = 1e-7 is what tests/test_gpu_modules.py applies to
GIoULoss gradients.

LOSS BLOCK -- ``lb_{case}_{L}_*`` for the `small` and `small_crowd`
LOSSBLOCK_CASES and L in ciou, diou, iou: LDHead.loss with loss_bbox replaced:
  _losses (8, 5) float64; _g{cls,reg,x}_abs_sum, _g{cls,reg,x}_sum (5,);
  _greg_{l}_idx, _greg_{l}_val: the gradient wrt the regression map of level l
  where it differs from the GIoU run's ``{case}_greg_{l}`` of
  tests/golden/lossblock.npz (flat indices and values: the side bins of the
  positive anchors); everywhere else it is that array, bit for bit.
The gradients wrt the class maps and the features do not depend on the box loss
(the QFL quality target is bbox_overlaps' IoU whichever loss is configured): the
generator ASSERTS they are bit-identical to lossblock.npz's ``{case}_gcls_{l}``
/ ``{case}_gx_{l}`` and does not store them a second time.
  lb_small_{atss,fcos,retina}_ciou_losses, lb_small_fcos_iou_losses: the tables
  of the LDATSSHead / LDFCOSHead / LDRetinaHead reference heads (FCOS 'iou' is
  FCOSGFLHead's constructor default IoULoss(loss_weight=1.0)).

WHOLE STEP -- ``voc_*``: one train step of
configs/ld/ld_r18_gflv1_r101_fpn_voc_1x.py with the geometry and seeds of the
e2e case 'tiny_r18' (gen_golden.E2E_CASES); the synthetic labels are taken
modulo the config's 20 classes.  _losses (8, 5), _log_vars, _grad_names,
_grad_norms as in e2e.npz.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'oracle'))
sys.path.insert(0, REPO)

import gen_golden as G  # noqa: E402  (installs ref_shim)

from ld_amd import synthetic  # noqa: E402

N_ROWS = 257  # two 128-thread blocks and one row
ROWS_SEED = 31
ATOL_LOSS, ATOL_GRAD = 5e-7, 1e-7
LOSSES = [('iou', 'IoULoss', {}), ('iou_linear', 'IoULoss', dict(linear=True)),
          ('diou', 'DIoULoss', {}), ('ciou', 'CIoULoss', {})]

# (pred, target[, replacement pred = target])
HAND = [
    # disjoint
    ((10., 10., 20., 20.), (30., 35., 50., 60.)),
    # touching along an edge; y1 and y2 tie in every min / max
    ((10., 10., 20., 20.), (20., 10., 30., 20.)),
    # target inside pred, pred inside target
    ((10., 10., 60., 50.), (20., 18., 40., 35.)),
    ((22., 19., 38., 33.), (10., 10., 60., 50.)),
    # equal aspect ratio: v = 0
    ((10., 10., 30., 20.), (15., 12., 55., 32.)),
    # pred == target.  As (12.5, 20.25, 48.5, 70.75) the reference's own fp32
    # CIoU is 0 / 0 = NaN (union + eps rounds to the union, so IoU = 1 and
    # v^2 / (1 - IoU + v) has a zero denominator); the generator replaces such
    # a row by the 2 x 2 box, where eps survives the rounding
    ((12.5, 20.25, 48.5, 70.75), (12.5, 20.25, 48.5, 70.75),
     (1., 1., 3., 3.)),
    # zero-area pred (zero width)
    ((25., 20., 25., 40.), (10., 10., 40., 50.)),
    # negative width (legal for the row API)
    ((30., 20., 22., 40.), (10., 10., 40., 50.)),
    # under one pixel
    ((5.1, 5.2, 5.6, 5.5), (5.0, 5.15, 5.7, 5.6)),
]


def _reference_rows(pred, target, dtype):
    from mmdet.models import build_loss
    out = {}
    for name, typ, kw in LOSSES:
        mod = build_loss(dict(type=typ, **kw))
        p = pred.to(dtype).clone().requires_grad_(True)
        loss = mod(p, target.to(dtype), reduction_override='none')
        loss.sum().backward()
        out[name] = (loss.detach().double().numpy(),
                     p.grad.double().numpy())
    return out


def _dev(x32, x64, atol):
    return float(np.max(np.maximum(np.abs(x32 - x64) - atol, 0.0) /
                        np.maximum(np.abs(x64), 1e-300)))


def gen_rows(d):
    hand = []
    for i, row in enumerate(HAND):
        p, t = torch.tensor([row[0]]), torch.tensor([row[1]])
        ok = all(np.isfinite(v).all()
                 for dt in (torch.float32, torch.float64)
                 for lg in _reference_rows(p, t, dt).values() for v in lg)
        if not ok:
            assert len(row) == 3, f'hand row {i}: non-finite, no replacement'
            print(f'[rows] hand row {i} replaced: the reference is not finite '
                  f'on {row[0]}')
            p = t = torch.tensor([row[2]])
        hand.append(torch.stack([p[0], t[0]]))
    hand = torch.stack(hand)  # (H, 2, 4)
    jp, jt = synthetic.box_loss_rows(N_ROWS - len(hand), ROWS_SEED)
    pred, target = torch.cat([hand[:, 0], jp]), torch.cat([hand[:, 1], jt])
    assert pred.shape == (N_ROWS, 4)
    d['rows_hand'] = hand.numpy()
    d['rows_seed'] = np.array([N_ROWS, ROWS_SEED])
    r32 = _reference_rows(pred, target, torch.float32)
    r64 = _reference_rows(pred, target, torch.float64)
    for name, _, _ in LOSSES:
        (l32, g32), (l64, g64) = r32[name], r64[name]
        for v in (l32, g32, l64, g64):
            assert np.isfinite(v).all(), name
        d[f'{name}_loss64'], d[f'{name}_grad64'] = l64, g64
        d[f'{name}_loss32'] = l32.astype(np.float32)
        d[f'{name}_grad32'] = g32.astype(np.float32)
        d[f'{name}_loss_ref32_dev'] = np.array(_dev(l32, l64, ATOL_LOSS))
        d[f'{name}_grad_ref32_dev'] = np.array(_dev(g32, g64, ATOL_GRAD))
        print(f'[rows] {name}: loss in [{l64.min():.3g}, {l64.max():.3g}], '
              f'ref32 dev loss {d[f"{name}_loss_ref32_dev"]:.3g} grad '
              f'{d[f"{name}_grad_ref32_dev"]:.3g}', flush=True)


def _swap_bbox_loss(head, typ, **kw):
    from mmdet.models import build_loss
    kw.setdefault('loss_weight', head.loss_bbox.loss_weight)
    head.loss_bbox = build_loss(dict(type=typ, **kw))
    return head


def _case_inputs(case, num_anchors=1, ctr=False):
    name, pad, img_shape, num_gt, bseed, hseed, _ = case
    batch = synthetic.synthetic_batch(num_imgs=len(num_gt), img_shape=img_shape,
                                      pad_shape=pad, num_gt=num_gt, seed=bseed)
    sizes = synthetic.level_shapes(pad)
    kw = dict(num_anchors=num_anchors) if num_anchors != 1 else {}
    hi = synthetic.synthetic_head_inputs(len(num_gt), sizes, seed=hseed, **kw)
    if ctr:
        hi['ctr'] = synthetic.synthetic_centerness(len(num_gt), sizes,
                                                   seed=hseed)
    return batch, hi


def _table(losses, keys):
    return np.stack([np.array([float(v.detach()) for v in losses[k]])
                     for k in keys]).astype(np.float64)


def gen_lossblock(d):
    base = np.load(os.path.join(G.OUT, 'lossblock.npz'))
    cases = [c for c in G.LOSSBLOCK_CASES if c[0] in ('small', 'small_crowd')]
    for case in cases:
        name = case[0]
        for tag, typ in (('ciou', 'CIoULoss'), ('diou', 'DIoULoss'),
                         ('iou', 'IoULoss')):
            head = _swap_bbox_loss(G._ld_head(), typ)
            batch, hi = _case_inputs(case)
            for k in ('cls', 'reg', 'x'):
                for t in hi[k]:
                    t.requires_grad_(True)
            losses = head.loss(hi['cls'], hi['reg'], batch['gt_bboxes'],
                               batch['gt_labels'], (hi['t_cls'], hi['t_reg']),
                               hi['x'], hi['t_x'], batch['img_metas'])
            key = f'lb_{name}_{tag}'
            d[key + '_losses'] = _table(losses, G.LOSS_KEYS)
            total = sum(sum(v) for v in losses.values())
            total.backward()
            assert np.isfinite(d[key + '_losses']).all()
            for k in ('cls', 'reg', 'x'):
                gs = [t.grad if t.grad is not None else torch.zeros_like(t)
                      for t in hi[k]]
                d[f'{key}_g{k}_abs_sum'] = np.array(
                    [float(g.double().abs().sum()) for g in gs])
                d[f'{key}_g{k}_sum'] = np.array(
                    [float(g.double().sum()) for g in gs])
                for l, g in enumerate(gs):
                    assert torch.isfinite(g).all()
                    g, b = G._np(g), base[f'{name}_g{k}_{l}']
                    if k == 'reg':
                        idx = np.flatnonzero(g != b)
                        d[f'{key}_greg_{l}_idx'] = idx.astype(np.int32)
                        d[f'{key}_greg_{l}_val'] = g.reshape(-1)[idx]
                    else:  # independent of the box loss: see the docstring
                        assert np.array_equal(g, b), (key, k)
            print(f'[lossblock] {key}: total {float(total):.6f} loss_bbox '
                  f'{d[key + "_losses"][1]}', flush=True)
    case = cases[0]
    for tag, mk, keys, na in (('atss', G._ld_atss_head, G.ATSS_KEYS, 1),
                              ('fcos', G._ld_fcos_head, G.ATSS_KEYS, 1),
                              ('retina', G._ld_retina_head, G.RETINA_KEYS, 9)):
        for ltag, typ in (('ciou', 'CIoULoss'), ) + \
                ((('iou', 'IoULoss'), ) if tag == 'fcos' else ()):
            head = _swap_bbox_loss(mk(), typ)
            batch, hi = _case_inputs(case, na, ctr=tag != 'retina')
            with torch.no_grad():
                if tag == 'retina':
                    losses = head.loss(hi['cls'], hi['reg'],
                                       batch['gt_bboxes'], batch['gt_labels'],
                                       (hi['t_cls'], hi['t_reg']),
                                       batch['img_metas'])
                else:
                    losses = head.loss(hi['cls'], hi['reg'], hi['ctr'],
                                       batch['gt_bboxes'], batch['gt_labels'],
                                       (hi['t_cls'], hi['t_reg'], None),
                                       batch['img_metas'])
            key = f'lb_small_{tag}_{ltag}_losses'
            d[key] = _table(losses, keys)
            assert np.isfinite(d[key]).all()
            print(f'[lossblock] {key}: loss_bbox {d[key][1]}', flush=True)


VOC_CFG = 'configs/ld/ld_r18_gflv1_r101_fpn_voc_1x.py'


def gen_step(d):
    name, _, pad, img_shape, num_gt, bseed = G.E2E_CASES[0]
    assert name == 'tiny_r18'
    torch.manual_seed(0)
    # as gen_e2e: the shipped imitation_method ('gibox', CUDA-only) has weight
    # 0 in this config and is evaluated as 'finegrained' x 0
    det = G.build_reference_detector(VOC_CFG, imitation_method='finegrained')
    assert type(det.bbox_head.loss_bbox).__name__ == 'CIoULoss'
    assert det.bbox_head.loss_im.loss_weight == 0
    det.load_state_dict(synthetic.seeded_state_dict(det.state_dict(), seed=1))
    det.teacher_model.load_state_dict(synthetic.seeded_state_dict(
        det.teacher_model.state_dict(), seed=2))
    det.train()
    batch = synthetic.synthetic_batch(num_imgs=len(num_gt), img_shape=img_shape,
                                      pad_shape=pad, num_gt=num_gt, seed=bseed)
    labels = [l % det.bbox_head.num_classes for l in batch['gt_labels']]
    losses = det.forward_train(batch['img'], batch['img_metas'],
                               batch['gt_bboxes'], labels)
    d['voc_cfg'] = np.array(list(pad) + list(img_shape) + [bseed])
    d['voc_num_gt'] = np.array(num_gt)
    d['voc_losses'] = _table(losses, G.LOSS_KEYS)
    loss, log_vars = det._parse_losses(losses)
    loss.backward()
    d['voc_log_vars'] = np.array(
        [log_vars[k] for k in G.LOSS_KEYS + ['loss']], dtype=np.float64)
    names, norms = [], []
    for k, p in det.named_parameters():
        if p.grad is not None:
            names.append(k)
            norms.append(float(p.grad.double().norm()))
    assert np.isfinite(norms).all() and np.isfinite(d['voc_losses']).all()
    d['voc_grad_names'], d['voc_grad_norms'] = np.array(names), np.array(norms)
    print('[step] voc:', {k: round(v, 6) for k, v in log_vars.items()},
          flush=True)


def main():
    d = {}
    gen_rows(d)
    gen_lossblock(d)
    gen_step(d)
    path = os.path.join(G.OUT, 'iou_losses.npz')
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    print(f'iou_losses.npz: {size} bytes')
    assert size <= os.path.getsize(os.path.join(G.OUT, 'lossblock.npz'))


if __name__ == '__main__':
    main()
