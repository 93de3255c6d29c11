"""The fused loss block restated in float64 torch on the CPU, gradients by
``torch.autograd`` alone.

``loss_block(flavour, maps, targets, hp, upstream)`` computes what
``ld_amd.lossblock.loss_block_forward`` computes for one batch: the (8, L) loss
table, ``num_total_samples``, the avg factor, and the gradients of
``sum(upstream * table)`` with respect to the student's maps.  No gradient
formula is written down here; the numpy oracle (oracle/ld_oracle.py) and the
kernels (ld_amd/csrc/loss.hip) both carry hand-derived ones, by the same
hands.  Shared by tests/test_loss_ref64_host.py and
tests/test_gpu_loss_edges.py.

Flavours (``hp`` = the keyword arguments of ``lossblock.make_hp``):
  'ld'      LDHead.loss                     (ld_head.py:116-375)
  'v2'      LDv2Head.loss, LD_LOSS_PROB_CLS (ld_gflv2.py:116-380): ``cls`` holds
            probabilities over ``cls_channels``, the KD term runs on kd_s / kd_t
  'atss'    LDATSSHead.loss, LD_LOSS_ATSS   (ld_atss.py:44-250)
  'fcos'    LDFCOSHead.loss, LD_LOSS_ATSS | LD_LOSS_FCOS (ld_fcos_head.py:46-217)
  'retina'  LDRetinaHead.loss, LD_LOSS_RETINA (ld_retina.py:41-254) in the
            pseudo-image layout: the B anchors of a cell are B images

Rows of the table: 0 cls, 1 bbox, 2 dfl, 3 ld, 4 ld_vlr, 5 kd, 6 centerness
(atss / fcos; 0 otherwise), 7 im.

Detached, as the reference detaches them: ``weight_targets`` (max class
score), the IoU ``score`` inside the quality focal loss, the centerness
targets, and both normalisers (the reference takes them through ``.item()``).

An image without a ground-truth box -- the project's definition:
  * it has no positive, no VLR cell and no IM cell; its valid cells are
    background with label weight 1;
  * it counts max(0, 1) = 1 towards ``num_total_samples`` = sum_i max(P_i, 1)
    (anchor_head.py's per-image floor; FCOS: max(sum_i P_i, 1));
  * a level without a positive has rows 1-3, 5 and 7 equal to 0
    (ld_head.py:246-252 zeroes loss_im there too, although the level may hold
    IM cells of another image: "IM cells but no positive"); row 4, VLR-LD, is
    computed whether or not the level has a positive (ld_head.py:254-274);
  * the reference itself gives no answer for LDHead / LDv2Head / LDATSSHead /
    LDRetinaHead: their ``_get_target_single`` raises on an empty image
    (``get_vlr_region`` returns an AssignResult that ``unmap`` cannot take);
    LDFCOSHead is defined there.

``wrong``: names of WRONG_RULES to evaluate a deliberately wrong definition
(the mutation test: the bar of the GPU tests must see each of them).

DFL targets are clamped at float32(16 - 0.1) as the reference's fp32
``bbox2distance`` clamps them; every other constant is exact in both
precisions."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from _iou_losses import LOSSES

BBOX_MODES = ('giou', ) + tuple(LOSSES)
FLAVOURS = ('ld', 'v2', 'atss', 'fcos', 'retina')
WRONG_RULES = (
    'nts_no_image_floor',  # num_total_samples without the per-image max(., 1)
    'im_without_pos',      # IM kept on a level with IM cells and no positive
    'kd_batch_count',      # KD / the batch's positives, not the level's
    'avg_no_guard',        # avg factor without + 1e-6 / < EPS -> 1 / max(., 1)
    'vlr_at_T_ld',         # VLR-LD evaluated at T_ld instead of T_ld_vlr
    'score_attached',      # the IoU score of QFL not detached
)
HP_DEFAULT = dict(
    num_classes=80, reg_max=16, feat_channels=256, lw_cls=1.0, lw_bbox=2.0,
    giou_eps=1e-6, lw_dfl=0.25, lw_ld=0.25, T_ld=10.0, lw_ld_vlr=0.25,
    T_ld_vlr=10.0, lw_kd=10.0, T_kd=2.0, lw_im=2.0, cls_channels=0,
    lw_ctr=0.0, focal_alpha=0.25, bbox_loss='giou')
DFL_MAX = float(np.float32(16.0) - np.float32(0.1))
DT = torch.float64


def _t64(a):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().to(DT).clone()
    return torch.from_numpy(np.ascontiguousarray(a)).to(DT)


def _rows(t):
    """(N, C, H, W) -> (N * H * W, C), image-major like the dense targets."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _kl_rows(s, t, T):
    """kd_loss.py:10-36 per row: T^2 * mean_j p_t (log p_t - log p_s)."""
    ls, lt = F.log_softmax(s / T, 1), F.log_softmax(t / T, 1)
    return (lt.exp() * (lt - ls)).mean(1) * (T * T)


def _overlap(p, t):
    lt, rb = torch.max(p[:, :2], t[:, :2]), torch.min(p[:, 2:], t[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, 0] * wh[:, 1]
    ap = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    at = (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])
    return inter, ap + at - inter


def _enclose(p, t):
    lt, rb = torch.min(p[:, :2], t[:, :2]), torch.max(p[:, 2:], t[:, 2:])
    return (rb - lt).clamp(min=0)


def iou_aligned(p, t):
    """bbox_overlaps(is_aligned=True), mode 'iou', eps = 1e-6."""
    inter, union = _overlap(p, t)
    return inter / torch.max(union, union.new_tensor(1e-6))


def box_loss_rows(mode, p, t, eps):
    """The five box losses on aligned xyxy rows (iou_loss.py; conventions as
    ld_amd/csrc/ld_math.h states them)."""
    if mode == 'giou':
        inter, union = _overlap(p, t)
        union = torch.max(union, union.new_tensor(eps))
        e = _enclose(p, t)
        ea = torch.max(e[:, 0] * e[:, 1], union.new_tensor(eps))
        return 1 - (inter / union - (ea - union) / ea)
    if mode in ('iou', 'iou_linear'):
        i = iou_aligned(p, t).clamp(min=eps)
        return 1 - i if mode == 'iou_linear' else -i.log()
    assert mode in ('diou', 'ciou'), mode
    inter, union = _overlap(p, t)
    iou = inter / (union + eps)
    e = _enclose(p, t)
    c2 = e[:, 0] ** 2 + e[:, 1] ** 2 + eps
    rho2 = ((t[:, 0] + t[:, 2]) - (p[:, 0] + p[:, 2])) ** 2 / 4 + \
        ((t[:, 1] + t[:, 3]) - (p[:, 1] + p[:, 3])) ** 2 / 4
    pen = rho2 / c2
    if mode == 'ciou':
        w1, h1 = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1] + eps
        w2, h2 = t[:, 2] - t[:, 0], t[:, 3] - t[:, 1] + eps
        v = (4 / math.pi ** 2) * (torch.atan(w2 / h2) - torch.atan(w1 / h1)) ** 2
        pen = pen + v ** 2 / (1 - iou + v)
    return 1 - (iou - pen)


def _focal(x, onehot, alpha):
    """py_sigmoid_focal_loss, gamma = 2 (losses/focal_loss.py:12-47)."""
    p = x.sigmoid()
    pt = (1 - p) * onehot + p * (1 - onehot)
    fw = (alpha * onehot + (1 - alpha) * (1 - onehot)) * pt ** 2
    return F.binary_cross_entropy_with_logits(x, onehot, reduction='none') * fw


def _qfl(x, score_map, prob):
    """quality_focal_loss, beta = 2 (gfocal_loss.py:8-50): ``score_map`` holds
    the IoU score at a positive's label channel and 0 elsewhere."""
    if prob:
        return F.binary_cross_entropy(x, score_map, reduction='none') * \
            (score_map - x) ** 2
    return F.binary_cross_entropy_with_logits(
        x, score_map, reduction='none') * (score_map - x.sigmoid()) ** 2


def level_slices(sizes):
    out, s = [], 0
    for h, w in sizes:
        out.append(slice(s, s + h * w))
        s += h * w
    return out


def counts(targets, sizes, num_classes=80, num_base=1):
    """What the tests count with numpy alone: positives per level and per
    (real) image, VLR / IM cells per level."""
    lab = np.asarray(targets['labels'])
    pos = (lab >= 0) & (lab < num_classes)
    sl = level_slices(sizes)
    vlr = np.asarray(targets['vlr']) > 0
    im = np.asarray(targets['im']) > 0 if 'im' in targets else np.zeros_like(pos)
    return dict(
        pos_per_level=[int(pos[:, s].sum()) for s in sl],
        pos_per_image=[int(v) for v in
                       pos.reshape(-1, num_base * pos.shape[1]).sum(1)],
        vlr_per_level=[int(vlr[:, s].sum()) for s in sl],
        im_per_level=[int(im[:, s].sum()) for s in sl])


def loss_block(flavour, maps, targets, hp=None, upstream=None, wrong=(),
               num_base=1, strides=(8, 16, 32, 64, 128)):
    """-> dict(losses (8, L) float64 ndarray, num_total_samples, avg_factor,
    grads {cls, reg, x, kd, ctr: per-level float64 ndarrays or None})."""
    assert flavour in FLAVOURS, flavour
    assert all(w in WRONG_RULES for w in wrong), wrong
    H = dict(HP_DEFAULT)
    H.update(hp or {})
    assert H['bbox_loss'] in BBOX_MODES and H['reg_max'] == 16
    NC = int(H['num_classes'])
    prob, retina, fcos = flavour == 'v2', flavour == 'retina', flavour == 'fcos'
    ctr_head = flavour in ('atss', 'fcos')
    L = len(maps['cls'])
    sizes = [tuple(int(v) for v in m.shape[2:]) for m in maps['cls']]

    def leaves(key):
        if maps.get(key) is None:
            return None
        return [_t64(m).requires_grad_(True) for m in maps[key]]

    def consts(key):
        if maps.get(key) is None:
            return None
        return [_t64(m) for m in maps[key]]

    cls, reg = leaves('cls'), leaves('reg')
    x, kd_s, ctr = leaves('x'), leaves('kd_s'), leaves('ctr')
    t_cls, t_reg, t_x, kd_t = (consts(k) for k in
                               ('t_cls', 't_reg', 't_x', 'kd_t'))
    assert prob == (kd_s is not None) and ctr_head == (ctr is not None)
    labels = torch.from_numpy(np.asarray(targets['labels']).astype(np.int64))
    lw_all = _t64(targets['label_weights'])
    bt_all = _t64(targets['bbox_targets'])
    vlr_all = _t64(targets['vlr'])
    im_all = _t64(targets['im']) if 'im' in targets else \
        torch.zeros_like(vlr_all)
    NI, A = labels.shape
    assert A == sum(h * w for h, w in sizes) and cls[0].shape[0] == NI
    pos_all = (labels >= 0) & (labels < NC)
    per_image = pos_all.reshape(NI // num_base, -1).sum(1)
    total_pos = int(per_image.sum())
    if fcos or 'nts_no_image_floor' in wrong:
        nts_raw = float(total_pos)
    else:
        nts_raw = float(per_image.clamp(min=1).sum())
    nts = max(nts_raw, 1.0)

    # ---- pass 1: per-level pieces that need the global avg factor later ----
    lv = []
    wsum = torch.zeros((), dtype=DT)
    for l, sl in enumerate(level_slices(sizes)):
        h, w = sizes[l]
        s = float(strides[l])
        lab = labels[:, sl].reshape(-1)
        pos = torch.nonzero(pos_all[:, sl].reshape(-1)).reshape(-1)
        c_r, r_r = _rows(cls[l]), _rows(reg[l])
        smax = (c_r if prob else c_r.sigmoid()).max(1).values.detach()
        d = dict(lab=lab, pos=pos, c_r=c_r, r_r=r_r, smax=smax,
                 lw=lw_all[:, sl].reshape(-1))
        if pos.numel():
            cell = pos % (h * w)
            cx = (cell % w).to(DT) + (0.5 if fcos else 0.0)
            cy = torch.div(cell, w, rounding_mode='floor').to(DT) + \
                (0.5 if fcos else 0.0)
            bt = bt_all[:, sl].reshape(-1, 4)[pos]
            if fcos:
                tgt = torch.stack([cx - bt[:, 0] / s, cy - bt[:, 1] / s,
                                   cx + bt[:, 2] / s, cy + bt[:, 3] / s], 1)
                lr, tb = bt[:, [0, 2]], bt[:, [1, 3]]
            else:
                tgt = bt / s
                lr = torch.stack([cx * s - bt[:, 0], bt[:, 2] - cx * s], 1)
                tb = torch.stack([cy * s - bt[:, 1], bt[:, 3] - cy * s], 1)
            ct = ((lr.min(1).values / lr.max(1).values) *
                  (tb.min(1).values / tb.max(1).values)).sqrt()
            p17 = F.softmax(r_r[pos].reshape(-1, 4, 17), 2)
            dist = (p17 * torch.arange(17, dtype=DT)).sum(2)
            box = torch.stack([cx - dist[:, 0], cy - dist[:, 1],
                               cx + dist[:, 2], cy + dist[:, 3]], 1)
            score = iou_aligned(box, tgt)
            if 'score_attached' not in wrong:
                score = score.detach()
            edge = torch.stack([cx - tgt[:, 0], cy - tgt[:, 1],
                                tgt[:, 2] - cx, tgt[:, 3] - cy], 1)
            d.update(tgt=tgt, box=box, ct=ct.detach(), score=score,
                     wt=smax[pos], ydfl=edge.clamp(0.0, DFL_MAX))
            wsum = wsum + (d['ct'] if ctr_head else d['wt']).sum()
        lv.append(d)
    guard = 'avg_no_guard' not in wrong
    if retina:
        avg = max(nts_raw, 1.0) if guard else nts_raw
    elif ctr_head:
        avg = float(wsum)
        avg = 1.0 if guard and avg < 1e-12 else avg
    else:
        avg = float(wsum) + (1e-6 if guard else 0.0)

    # ---- pass 2: the table ---------------------------------------------------
    zero = torch.zeros((), dtype=DT)
    table = [[zero] * L for _ in range(8)]
    for l, sl in enumerate(level_slices(sizes)):
        d = lv[l]
        pos, lab, lw, c_r, r_r = d['pos'], d['lab'], d['lw'], d['c_r'], d['r_r']
        tr_r = _rows(t_reg[l])
        P_l = int(pos.numel())
        # -- classification over every cell
        smap = torch.zeros_like(c_r)
        if P_l:
            smap = smap.index_put(
                (pos, lab[pos]),
                torch.ones(P_l, dtype=DT) if ctr_head or retina else d['score'])
        q = _focal(c_r, smap, H['focal_alpha']) if ctr_head or retina \
            else _qfl(c_r, smap, prob)
        table[0][l] = H['lw_cls'] * (q.sum(1) * lw).sum() / nts
        # -- VLR-LD
        v = vlr_all[:, sl].reshape(-1).clone()
        if fcos:
            v = v * d['smax']
        if retina:
            v[pos] = 0.0
        rem = torch.nonzero(v > 0).reshape(-1)
        T_vlr = H['T_ld'] if 'vlr_at_T_ld' in wrong else H['T_ld_vlr']
        if rem.numel() and retina:
            kl = _kl_rows(r_r[rem], tr_r[rem], T_vlr)
            table[4][l] = H['lw_ld_vlr'] * (kl * v[rem]).sum() / 16
        elif rem.numel():
            kl = _kl_rows(r_r[rem].reshape(-1, 17), tr_r[rem].reshape(-1, 17),
                          T_vlr).reshape(-1, 4)
            table[4][l] = H['lw_ld_vlr'] * (kl * v[rem, None]).sum() / 16
        # -- imitation (quirk: zero on a level without a positive)
        fg = torch.nonzero(im_all[:, sl].reshape(-1) > 0).reshape(-1)
        if x is not None and H['lw_im'] != 0 and fg.numel() and \
                (P_l or 'im_without_pos' in wrong):
            dx = _rows(x[l])[fg] - _rows(t_x[l])[fg]
            table[7][l] = H['lw_im'] * (dx * dx).mean()
        if not P_l:
            continue
        wt = d['wt']
        wb = d['ct'] if ctr_head else (torch.ones_like(wt) if retina else wt)
        gl = box_loss_rows(H['bbox_loss'], d['box'], d['tgt'], H['giou_eps'])
        table[1][l] = H['lw_bbox'] * (gl * wb).sum() / avg
        # -- DFL (gfocal_loss.py:53-74), avg_factor = 4
        y = d['ydfl'].reshape(-1)
        yl = y.long()
        ls = F.log_softmax(r_r[pos].reshape(-1, 17), 1)
        dfl = -ls.gather(1, yl[:, None])[:, 0] * ((yl + 1).to(DT) - y) - \
            ls.gather(1, yl[:, None] + 1)[:, 0] * (y - yl.to(DT))
        table[2][l] = H['lw_dfl'] * (dfl.reshape(-1, 4) *
                                     wt[:, None]).sum() / 4 / avg
        # -- LD on the positives
        if retina:
            kl = _kl_rows(r_r[pos], tr_r[pos], H['T_ld'])
            table[3][l] = H['lw_ld'] * (kl * wt).sum() / 4
        else:
            kl = _kl_rows(r_r[pos].reshape(-1, 17), tr_r[pos].reshape(-1, 17),
                          H['T_ld']).reshape(-1, 4)
            table[3][l] = H['lw_ld'] * (kl * wt[:, None]).sum() / 4
        # -- KD on the class maps of the positives, avg_factor = P_l
        ks = _rows(kd_s[l]) if prob else c_r
        kt = _rows(kd_t[l] if prob else t_cls[l])
        kl = _kl_rows(ks[pos], kt[pos], H['T_kd'])
        div = total_pos if 'kd_batch_count' in wrong else P_l
        table[5][l] = H['lw_kd'] * (kl * lw[pos]).sum() / div
        if ctr_head:
            bce = F.binary_cross_entropy_with_logits(
                _rows(ctr[l])[pos, 0], d['ct'], reduction='none')
            table[6][l] = H['lw_ctr'] * bce.sum() / nts
    tab = torch.stack([torch.stack([e + zero for e in row]) for row in table])
    up = torch.ones((8, L), dtype=DT) if upstream is None else _t64(upstream)
    total = (up * tab).sum()
    groups = dict(cls=cls, reg=reg, x=x, kd=kd_s, ctr=ctr)
    flat = [t for g in groups.values() if g is not None for t in g]
    if total.requires_grad:
        got = torch.autograd.grad(total, flat, allow_unused=True)
    else:
        got = [None] * len(flat)
    grads, i = {}, 0
    for k, g in groups.items():
        if g is None:
            grads[k] = None
            continue
        grads[k] = [(torch.zeros_like(t) if got[i + j] is None
                     else got[i + j]).numpy() for j, t in enumerate(g)]
        i += len(g)
    return dict(losses=tab.detach().numpy(), num_total_samples=nts,
                num_total_raw=nts_raw, avg_factor=avg, grads=grads)
