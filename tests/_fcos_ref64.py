"""float64 autograd restatement of the plain FCOS head's box branch, loss and
decode, written from the reference's formulas (not from ld_amd's kernels):

  FCOSHead.forward_single  mmdet/models/dense_heads/fcos_head.py:145-153
  FCOSHead.loss            fcos_head.py:157-254
  centerness_target        fcos_head.py:590-608
  points                   fcos_head.py:456-466
  norm_on_bbox targets     fcos_head.py:524-525
  distance2bbox            core/bbox/transforms.py:135-154
  py_sigmoid_focal_loss    models/losses/focal_loss.py:12-47 (_plain_ref64.focal)
  the five box losses      models/losses/iou_loss.py (_loss_ref64.box_loss_rows)
  binary_cross_entropy     models/losses/cross_entropy_loss.py:52-90

It takes the TARGETS as given -- labels and (l, t, r, b) pixel distances per
point, (N, A) / (N, A, 4) in the level-concatenated order of the kernels -- and
returns the per-level loss table (3, L) as a float64 tensor that autograd
differentiates down to the raw maps and the scales.  One process, no cross-rank
reduction."""
import torch
import torch.nn.functional as F

from _loss_ref64 import box_loss_rows
from _plain_ref64 import focal


def activate(raw, scales, strides, norm_on_bbox, training=True):
    """exp(scale_l * x), or relu(scale_l * x) [* stride_l in eval mode]."""
    out = []
    for l, (r, stride) in enumerate(zip(raw, strides)):
        u = r * scales[l]
        if not norm_on_bbox:
            out.append(u.exp())
        else:
            u = torch.relu(u)
            out.append(u if training else u * stride)
    return out


def points(h, w, stride, dtype=torch.float64):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype),
                            torch.arange(w, dtype=dtype), indexing='ij')
    return torch.stack([xs.reshape(-1) * stride + stride // 2,
                        ys.reshape(-1) * stride + stride // 2], dim=-1)


def distance2bbox(pts, d, max_shape=None):
    x1, y1 = pts[:, 0] - d[:, 0], pts[:, 1] - d[:, 1]
    x2, y2 = pts[:, 0] + d[:, 2], pts[:, 1] + d[:, 3]
    if max_shape is not None:
        x1, x2 = x1.clamp(0, max_shape[1]), x2.clamp(0, max_shape[1])
        y1, y2 = y1.clamp(0, max_shape[0]), y2.clamp(0, max_shape[0])
    return torch.stack([x1, y1, x2, y2], dim=-1)


def centerness_target(t):
    lr, tb = t[:, [0, 2]], t[:, [1, 3]]
    return torch.sqrt((lr.min(-1)[0] / lr.max(-1)[0]) *
                      (tb.min(-1)[0] / tb.max(-1)[0]))


INF = 1e8
REGRESS_RANGES = ((-1, 64), (64, 128), (128, 256), (256, 512), (512, INF))


def fcos_targets(gt_bboxes, gt_labels, sizes, strides, num_classes,
                 center_sampling=False, radius=1.5,
                 regress_ranges=REGRESS_RANGES):
    """_get_target_single (fcos_head.py:529-612) per image, in float64 (every
    coordinate of the fixtures is exact in fp32): labels (N, A) and (l, t, r,
    b) pixel targets (N, A, 4) over the level-concatenated points; a point
    inside several boxes takes the one of minimal area."""
    pts = torch.cat([points(h, w, s) for (h, w), s in zip(sizes, strides)])
    rr = torch.cat([torch.tensor([r], dtype=torch.float64).expand(h * w, 2)
                    for (h, w), r in zip(sizes, regress_ranges)])
    st = torch.cat([torch.full((h * w, ), float(s) * radius,
                               dtype=torch.float64)
                    for (h, w), s in zip(sizes, strides)])
    A = pts.shape[0]
    labels, targets = [], []
    for gb, gl in zip(gt_bboxes, gt_labels):
        gb = gb.double().cpu()
        if gb.shape[0] == 0:
            labels.append(torch.full((A, ), num_classes, dtype=torch.long))
            targets.append(torch.zeros((A, 4), dtype=torch.float64))
            continue
        areas = ((gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1]))[None] \
            .repeat(A, 1)
        xs, ys = pts[:, 0:1], pts[:, 1:2]
        t = torch.stack([xs - gb[None, :, 0], ys - gb[None, :, 1],
                         gb[None, :, 2] - xs, gb[None, :, 3] - ys], -1)
        if center_sampling:
            cx, cy = (gb[:, 0] + gb[:, 2]) / 2, (gb[:, 1] + gb[:, 3]) / 2
            x0 = torch.max(cx[None] - st[:, None], gb[None, :, 0])
            y0 = torch.max(cy[None] - st[:, None], gb[None, :, 1])
            x1 = torch.min(cx[None] + st[:, None], gb[None, :, 2])
            y1 = torch.min(cy[None] + st[:, None], gb[None, :, 3])
            inside = torch.stack([xs - x0, ys - y0, x1 - xs, y1 - ys],
                                 -1).min(-1)[0] > 0
        else:
            inside = t.min(-1)[0] > 0
        far = t.max(-1)[0]
        in_range = (far >= rr[:, 0:1]) & (far <= rr[:, 1:2])
        areas[~inside] = INF
        areas[~in_range] = INF
        amin, idx = areas.min(dim=1)
        lab = gl.cpu()[idx].clone()
        lab[amin == INF] = num_classes
        labels.append(lab)
        targets.append(t[torch.arange(A), idx])
    return torch.stack(labels), torch.stack(targets)


def _rows(t, ch):
    """(N, ch, H, W) -> (N, H * W, ch)."""
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, ch)


def fcos_loss(maps, scales, labels, bbox_targets, strides, num_classes,
              norm_on_bbox=False, bbox_loss='iou', eps=1e-6, lw_cls=1.0,
              lw_bbox=1.0, lw_ctr=1.0, alpha=0.25):
    """``maps``: dict of per-level float64 tensors ``cls`` (N, C, h, w), ``raw``
    (N, 4, h, w) before Scale and activation, ``ctr`` (N, 1, h, w); ``scales``
    (L,) float64; ``labels`` (N, A), ``bbox_targets`` (N, A, 4) float64 pixels.
    -> table (3, L): loss_cls, loss_bbox, loss_centerness per level (their sums
    over the levels are the reference's three scalars)."""
    reg = activate(maps['raw'], scales, strides, norm_on_bbox, training=True)
    pos_all = (labels >= 0) & (labels < num_classes)
    num_pos = max(float(pos_all.sum()), 1.0)
    rows, off, ctr_sum = [], 0, 0.0
    for l, (c, r, k) in enumerate(zip(maps['cls'], reg, maps['ctr'])):
        N, _, h, w = c.shape
        n = h * w
        lab = labels[:, off:off + n].reshape(-1)
        tgt = bbox_targets[:, off:off + n].reshape(-1, 4)
        off += n
        if norm_on_bbox:
            tgt = tgt / strides[l]
        loss_cls = lw_cls * focal(_rows(c, num_classes).reshape(
            -1, num_classes), lab, alpha).sum() / num_pos
        pos = ((lab >= 0) & (lab < num_classes)).nonzero()[:, 0]
        if len(pos) == 0:
            rows.append((loss_cls, r.sum() * 0, k.sum() * 0))
            continue
        pts = points(h, w, strides[l]).repeat(N, 1)[pos]
        ct = centerness_target(tgt[pos])
        box = distance2bbox(pts, _rows(r, 4).reshape(-1, 4)[pos])
        tbox = distance2bbox(pts, tgt[pos])
        loss_bbox = lw_bbox * (box_loss_rows(bbox_loss, box, tbox, eps) *
                               ct).sum()
        bce = F.binary_cross_entropy_with_logits(
            _rows(k, 1).reshape(-1)[pos], ct, reduction='none')
        rows.append((loss_cls, loss_bbox, lw_ctr * bce.sum() / num_pos))
        ctr_sum += float(ct.sum())
    denorm = max(ctr_sum, 1e-6)
    return torch.stack([torch.stack([r[0] for r in rows]),
                        torch.stack([r[1] for r in rows]) / denorm,
                        torch.stack([r[2] for r in rows])])


def decode_level(cls, reg, ctr, stride, img_shape, nms_pre):
    """fcos_head.py:373-405 for ONE image and level: (boxes (K, 4), scores
    (K, C), factors (K,)) of the nms_pre best points by max_c score * ctr, in
    torch.topk's order."""
    C = cls.shape[0]
    h, w = cls.shape[-2:]
    scores = cls.permute(1, 2, 0).reshape(-1, C).sigmoid()
    fac = ctr.permute(1, 2, 0).reshape(-1).sigmoid()
    d = reg.permute(1, 2, 0).reshape(-1, 4)
    pts = points(h, w, stride, dtype=d.dtype)
    if 0 < nms_pre < scores.shape[0]:
        _, idx = (scores * fac[:, None]).max(-1)[0].topk(nms_pre)
        scores, fac, d, pts = scores[idx], fac[idx], d[idx], pts[idx]
    return distance2bbox(pts, d, max_shape=img_shape), scores, fac
