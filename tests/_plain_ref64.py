"""float64 autograd restatement of the plain heads' losses, written from the
reference's formulas (not from ld_amd's kernels):

  ATSSHead.loss / loss_single   mmdet/models/dense_heads/atss_head.py:145-313
  AnchorHead.loss / loss_single mmdet/models/dense_heads/anchor_head.py:376-495
  delta2bbox / bbox2delta       core/bbox/coder/delta_xywh_bbox_coder.py:87-220
  py_sigmoid_focal_loss         models/losses/focal_loss.py:12-47
  giou_loss / bbox_overlaps     models/losses/iou_loss.py:85-102,
                                core/bbox/iou_calculators/iou2d_calculator.py
  l1_loss / smooth_l1_loss      models/losses/smooth_l1_loss.py:9-56
  binary_cross_entropy          models/losses/cross_entropy_loss.py:52-90

It takes the TARGETS as given (labels, label weights and matched GT boxes per
anchor, in the reference's (image, level, cell, base anchor) order) and the
anchors, and returns the per-level loss table as a float64 tensor that autograd
differentiates.  No cross-rank reduction (one process)."""
import math

import torch

MAX_RATIO = abs(math.log(16 / 1000))
EPS = 1e-12  # atss_head.py:11


def bbox2delta(p, g, means, stds):
    px, py = (p[:, 0] + p[:, 2]) * 0.5, (p[:, 1] + p[:, 3]) * 0.5
    pw, ph = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    gx, gy = (g[:, 0] + g[:, 2]) * 0.5, (g[:, 1] + g[:, 3]) * 0.5
    gw, gh = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    d = torch.stack([(gx - px) / pw, (gy - py) / ph, torch.log(gw / pw),
                     torch.log(gh / ph)], dim=-1)
    return (d - d.new_tensor(means)) / d.new_tensor(stds)


def delta2bbox(r, d, means, stds):
    d = d * d.new_tensor(stds) + d.new_tensor(means)
    dw = d[:, 2].clamp(min=-MAX_RATIO, max=MAX_RATIO)
    dh = d[:, 3].clamp(min=-MAX_RATIO, max=MAX_RATIO)
    px, py = (r[:, 0] + r[:, 2]) * 0.5, (r[:, 1] + r[:, 3]) * 0.5
    pw, ph = r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
    gw, gh = pw * dw.exp(), ph * dh.exp()
    gx, gy = px + pw * d[:, 0], py + ph * d[:, 1]
    return torch.stack([gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5,
                        gy + gh * 0.5], dim=-1)


def giou_loss(pred, target, eps=1e-6):
    a1 = (pred[:, 2] - pred[:, 0]) * (pred[:, 3] - pred[:, 1])
    a2 = (target[:, 2] - target[:, 0]) * (target[:, 3] - target[:, 1])
    lt = torch.max(pred[:, :2], target[:, :2])
    rb = torch.min(pred[:, 2:], target[:, 2:])
    wh = (rb - lt).clamp(min=0)
    overlap = wh[:, 0] * wh[:, 1]
    union = (a1 + a2 - overlap).clamp(min=eps)
    ious = overlap / union
    elt = torch.min(pred[:, :2], target[:, :2])
    erb = torch.max(pred[:, 2:], target[:, 2:])
    ewh = (erb - elt).clamp(min=0)
    earea = (ewh[:, 0] * ewh[:, 1]).clamp(min=eps)
    return 1 - (ious - (earea - union) / earea)


def focal(pred, labels, alpha=0.25, gamma=2.0):
    """(rows, C) element losses; labels == C (or more) is background."""
    C = pred.shape[1]
    t = torch.nn.functional.one_hot(labels.clamp(max=C), C + 1)[:, :C]
    t = t.to(pred.dtype)
    p = pred.sigmoid()
    pt = (1 - p) * t + p * (1 - t)
    w = (alpha * t + (1 - alpha) * (1 - t)) * pt.pow(gamma)
    return torch.nn.functional.binary_cross_entropy_with_logits(
        pred, t, reduction='none') * w


def centerness_target(anchors, gts):
    cx = (anchors[:, 2] + anchors[:, 0]) / 2
    cy = (anchors[:, 3] + anchors[:, 1]) / 2
    lr = torch.stack([cx - gts[:, 0], gts[:, 2] - cx], dim=1)
    tb = torch.stack([cy - gts[:, 1], gts[:, 3] - cy], dim=1)
    return torch.sqrt((lr.min(-1)[0] / lr.max(-1)[0]) *
                      (tb.min(-1)[0] / tb.max(-1)[0]))


def _rows(t, ch):
    """(N, B * ch, H, W) -> (N * H * W * B, ch), the reference's permute."""
    return t.permute(0, 2, 3, 1).reshape(-1, ch)


def plain_loss(kind, maps, targets, anchors, num_classes, coder, box_term,
               lw_bbox, beta=1.0, lw_cls=1.0, lw_ctr=1.0, alpha=0.25):
    """``maps``: dict of per-level float64 tensors (cls, reg[, ctr]) with
    requires_grad.  ``targets``: per level dict(labels (rows,), weights
    (rows,), gts (rows, 4)) in the row order of ``_rows``; ``anchors``: per
    level (rows / N, 4).  ``num_pos_img``: positives per image.
    -> table (K, L): loss_cls, loss_bbox[, loss_centerness]."""
    means, stds = coder
    N = maps['cls'][0].shape[0]
    nts = float(max(sum(max(int(p), 1) for p in targets['num_pos_img']), 1.0))
    cls_rows, box_rows, ctr_rows, ctr_sum = [], [], [], 0.0
    for l, (c, r) in enumerate(zip(maps['cls'], maps['reg'])):
        t = targets['levels'][l]
        an = anchors[l].repeat(N, 1)
        pred_c, pred_r = _rows(c, num_classes), _rows(r, 4)
        lc = (focal(pred_c, t['labels'], alpha) *
              t['weights'][:, None]).sum() / nts
        cls_rows.append(lw_cls * lc)
        pos = ((t['labels'] >= 0) & (t['labels'] < num_classes)).nonzero()[:, 0]
        if kind == 'atss':
            ctr = _rows(maps['ctr'][l], 1)[:, 0]
            if len(pos) == 0:
                box_rows.append(pred_r.sum() * 0)
                ctr_rows.append(ctr.sum() * 0)
                continue
            tdelta = bbox2delta(an[pos], t['gts'][pos], means, stds)
            tgt = delta2bbox(an[pos], tdelta, means, stds)
            ct = centerness_target(an[pos], tgt)
            box = delta2bbox(an[pos], pred_r[pos], means, stds)
            box_rows.append(lw_bbox * (giou_loss(box, tgt) * ct).sum())
            bce = torch.nn.functional.binary_cross_entropy_with_logits(
                ctr[pos], ct, reduction='none')
            ctr_rows.append(lw_ctr * bce.sum() / nts)
            ctr_sum = ctr_sum + float(ct.sum())
        elif len(pos) == 0:
            box_rows.append(pred_r.sum() * 0)
        elif box_term == 'decoded':
            box = delta2bbox(an[pos], pred_r[pos], means, stds)
            box_rows.append(lw_bbox * giou_loss(box, t['gts'][pos]).sum() /
                            nts)
        else:
            d = (pred_r[pos] - bbox2delta(an[pos], t['gts'][pos], means,
                                          stds)).abs()
            el = d if box_term == 'l1' else torch.where(
                d < beta, 0.5 * d * d / beta, d - 0.5 * beta)
            box_rows.append(lw_bbox * el.sum() / nts)
    if kind == 'atss':
        avg = ctr_sum if ctr_sum >= EPS else 1.0
        return torch.stack([torch.stack(cls_rows),
                            torch.stack(box_rows) / avg,
                            torch.stack(ctr_rows)])
    return torch.stack([torch.stack(cls_rows), torch.stack(box_rows)])
