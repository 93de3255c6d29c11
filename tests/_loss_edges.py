"""Named edge cases of the fused loss block (ld_amd/csrc/loss.hip): the states
the four synthetic batches of the parity tests never reach.  Pattern of
tests/_target_edges.py: every case is a builder returning a dict

  flavour, sizes, strides, metas, boxes, labels   geometry and ground truth
  maps        head outputs, per-level float32 CPU tensors (cls, reg, t_cls,
              t_reg, x, t_x and kd_s / kd_t / ctr where the flavour has them;
              LDRetinaHead in the (N * 9, C, H, W) pseudo-image layout)
  hp          keyword arguments of lossblock.make_hp (without the flavour flag)
  overrides   [(image, anchor, box)] written over bbox_targets (box_ties)
  claims      what the case contains, as counts; tests/test_loss_ref64_host.py
              recounts every one with oracle/ld_oracle.py and numpy alone

``build(name, flavour)`` is cached; nothing here touches a GPU.

Geometries (no shape larger than these):
  pad 128x128   levels of 256, 64, 16, 4, 1 cells: exactly one 256-anchor
                block, exactly one 64-lane prepass wave
  pad 136x264   levels of 561, 153, 45, 15, 6 cells: ragged tails, and in the
                packed (N, C, A) arena odd level bases (561, 714, 759, 774)
  pad 256x320   10 blocks of 256 anchors per image: a full group of 32
                (block, side) pairs plus a tail for the one-XCD block order
  pad 64x96     levels of 96, 24, 6, 2, 1 cells with a positive on each
The ``ragged`` image with boxes carries pad_shape (120, 232) in its meta, so
its valid region is 15x29 of the 17x33 level-0 cells (and 8x15, 4x8, 2x4, 1x2
of the coarser ones): the cells outside have label weight 0."""
import functools

import numpy as np
import torch

import ld_oracle as O
from ld_amd import synthetic

F32 = np.float32
STRIDES = [8, 16, 32, 64, 128]
RETINA_B = 9
SIDE = ('atss', 'fcos', 'retina')

# per flavour: what the heads hand to make_hp (ld_amd/heads.py _hp / _ld_hp
# with the loss weights of configs/ld/*.py)
HP = dict(
    ld=dict(),
    v2=dict(cls_channels=81),
    atss=dict(lw_dfl=0.0, lw_ctr=1.0, lw_ld=0.25, T_ld=10.0,
              lw_ld_vlr=0.15 * 4.0 * 0.25, T_ld_vlr=10.0, lw_kd=10.0, T_kd=2.0,
              lw_im=0.0),
    fcos=dict(lw_bbox=1.0, lw_dfl=0.0, lw_ctr=1.0, lw_ld=0.25, T_ld=10.0,
              lw_ld_vlr=0.25 * 4.0 * 0.25, T_ld_vlr=10.0, lw_kd=10.0, T_kd=2.0,
              lw_im=0.0),
    retina=dict(lw_dfl=0.0, lw_ld=5.0, T_ld=10.0, lw_ld_vlr=0.03 * 4.0 * 5.0,
                T_ld_vlr=10.0, lw_kd=10.0, T_kd=8.0, lw_im=0.0),
)

# name -> (pad, image shape, num_gt, batch seed, per-image pad_shape or None)
GEOMETRY = dict(
    empty_beside_full=((128, 128), (128, 128), [0, 3], 4, None),
    all_empty=((136, 264), (130, 260), [0, 0], 6, None),
    one_empty=((136, 264), (130, 260), [0], 6, None),
    ragged=((136, 264), (130, 260), [0, 5], 7, [None, (120, 232)]),
    ten_blocks=((256, 320), (250, 300), [4, 0, 1], 5, None),
)
# one GT per level, each about 0.97 x the side of that level's anchor and
# centred next to one of its anchor centres (generic offsets: no ties)
POS_EVERY_LEVEL = [
    [[-500.5, -497.25, 500.25, 499.5],          # level 4, anchor at (0, 0)
     [-186.5, -247.25, 313.25, 251.5],          # level 3, anchor at (64, 0)
     [-92.5, -93.25, 158.25, 155.5]],           # level 2, anchor at (32, 32)
    [[-14.5, -29.25, 110.25, 94.5],             # level 1, anchor at (48, 32)
     [9.5, -6.75, 71.25, 54.5]],                # level 0, anchor at (40, 24)
]


def _meta(shape, pad):
    return dict(img_shape=tuple(shape) + (3, ), pad_shape=tuple(pad) + (3, ),
                ori_shape=tuple(shape) + (3, ), scale_factor=1.0, flip=False)


def geometry(name):
    """-> dict(pad, sizes, metas, boxes, labels) of a named geometry."""
    if name == 'pos_every_level':
        pad = (64, 96)
        boxes = [np.asarray(b, F32) for b in POS_EVERY_LEVEL]
        labels = [np.asarray([3, 17, 42], np.int64),
                  np.asarray([7, 79], np.int64)]
        metas = [_meta(pad, pad) for _ in boxes]
    else:
        pad, shape, num_gt, seed, pads = GEOMETRY[name]
        b = synthetic.synthetic_batch(len(num_gt), shape, pad, num_gt, seed)
        boxes = [x.numpy() for x in b['gt_bboxes']]
        labels = [x.numpy() for x in b['gt_labels']]
        metas = [_meta(shape, (pads[i] if pads and pads[i] else pad))
                 for i in range(len(num_gt))]
    return dict(pad=pad, sizes=synthetic.level_shapes(pad), metas=metas,
                boxes=boxes, labels=labels)


def head_inputs(flavour, N, sizes, seed, num_classes=80, feat_channels=256):
    """Seeded head outputs in the layout the flavour's loss block reads."""
    B = RETINA_B if flavour == 'retina' else 1
    C = num_classes + 1 if flavour == 'v2' else num_classes
    hi = synthetic.synthetic_head_inputs(N, sizes, seed=seed, num_classes=C,
                                         feat_channels=feat_channels,
                                         num_anchors=B)
    if flavour == 'retina':
        hi = {k: [t.view(N * B, t.shape[1] // B, *t.shape[2:]) for t in v]
              for k, v in hi.items() if k not in ('x', 't_x')}
    if flavour == 'v2':
        # cls_score = sigmoid(cls_feat) * quality: probabilities in (0, 1)
        gen = torch.Generator().manual_seed(seed + 1)
        hi['kd_s'], hi['kd_t'] = hi['cls'], hi['t_cls']
        hi['cls'] = [(torch.sigmoid(c + 3.0) *
                      (0.3 + 0.7 * torch.rand(c.shape, generator=gen))).float()
                     for c in hi['kd_s']]
    if flavour in ('atss', 'fcos'):
        hi['ctr'] = synthetic.synthetic_centerness(N, sizes, seed=seed)
    if flavour in SIDE:
        hi['x'] = hi['t_x'] = None   # no imitation term: these heads read none
    return hi


def _pseudo(arr, num_level, B):
    """(N, sum_l A_l * B[, 4]) in the reference's (cell, base anchor) order ->
    the (N * B, A[, 4]) pseudo-image layout of the loss block."""
    N, out, s = arr.shape[0], [], 0
    for n in num_level:
        a = arr[:, s:s + n].reshape((N, n // B, B) + arr.shape[2:])
        out.append(np.moveaxis(a, 2, 1).reshape((N * B, n // B) +
                                                arr.shape[2:]))
        s += n
    return np.ascontiguousarray(np.concatenate(out, 1))


def oracle_targets(case):
    """Dense targets in the loss block's layout from oracle/ld_oracle.py, and
    the oracle's own dict (``raw``) for its loss functions."""
    fl, NC = case['flavour'], case['hp'].get('num_classes', 80)
    sizes, boxes, labels = case['sizes'], case['boxes'], case['labels']
    if fl == 'fcos':
        raw = O.fcos_targets(sizes, boxes, labels, num_classes=NC)
        t = dict(labels=raw['labels'], bbox_targets=raw['bbox_targets'],
                 label_weights=np.ones(raw['labels'].shape, F32),
                 vlr=(raw['labels'] == NC + 1).astype(F32),
                 im=np.zeros(raw['labels'].shape, F32))
    elif fl == 'retina':
        raw = O.retina_targets(sizes, case['metas'], boxes, labels,
                               num_classes=NC)
        t = {k: _pseudo(raw[k], raw['num_level'], RETINA_B)
             for k in ('labels', 'label_weights', 'bbox_targets', 'vlr')}
        t['im'] = np.zeros(t['vlr'].shape, F32)
    else:
        raw = O.get_targets(sizes, case['metas'], boxes, labels,
                            num_classes=NC)
        t = {k: raw[k] for k in ('labels', 'label_weights', 'bbox_targets',
                                 'vlr', 'im')}
    for n, a, box in case.get('overrides', ()):
        t['bbox_targets'] = t['bbox_targets'].copy()
        t['bbox_targets'][n, a] = box
        raw['bbox_targets'] = t['bbox_targets']
    t['raw'] = raw
    return t


_ORACLE_HP = ('num_classes', 'lw_cls', 'lw_bbox', 'lw_dfl', 'lw_ld', 'T_ld',
              'lw_ld_vlr', 'T_ld_vlr', 'lw_kd', 'T_kd', 'lw_im', 'giou_eps',
              'lw_ctr', 'focal_alpha')


def oracle_block(case, targets):
    """The float32 numpy oracle on the case -> dict(losses (8, L), grads) in
    the loss block's layout, or None where the oracle has no such mode (the
    box losses other than GIoU)."""
    fl, hp = case['flavour'], case['hp']
    if hp.get('bbox_loss', 'giou') != 'giou':
        return None
    m = {k: (None if v is None else [t.numpy() for t in v])
         for k, v in case['maps'].items()}
    ohp = {k: hp[k] for k in _ORACLE_HP if k in hp}
    raw, L = targets['raw'], len(case['sizes'])
    table = np.zeros((8, L), F32)
    if fl in ('ld', 'v2'):
        kd = (m['kd_s'], m['kd_t']) if fl == 'v2' else None
        if fl == 'v2':
            ohp['num_classes'] = hp.get('num_classes', 80)
        o = O.ld_loss_block(m['cls'], m['reg'], m['t_cls'], m['t_reg'],
                            m['x'], m['t_x'], raw, ohp, kd=kd)
        table[:] = o['losses']
        g = o['grads']
        return dict(losses=table, grads=dict(
            cls=g['cls'], reg=g['reg'], x=g['x'], kd=g.get('kd'), ctr=None))
    if fl == 'retina':
        ohp.pop('lw_ld_vlr', None), ohp.pop('T_ld_vlr', None)
        N = len(case['boxes'])
        full = {k: [a.reshape(N, -1, *a.shape[2:]) for a in m[k]]
                for k in ('cls', 'reg', 't_cls', 't_reg')}
        o = O.ld_retina_loss_block(full['cls'], full['reg'], full['t_cls'],
                                   full['t_reg'], raw, ohp)
        table[[0, 1, 3, 4, 5]] = o['losses']
        g = {k: [a.reshape(b.shape) for a, b in zip(o['grads'][k], m[k])]
             for k in ('cls', 'reg')}
        return dict(losses=table, grads=dict(cls=g['cls'], reg=g['reg'],
                                             x=None, kd=None, ctr=None))
    ohp.pop('lw_ld_vlr', None), ohp.pop('T_ld_vlr', None)
    ohp.pop('lw_dfl', None), ohp.pop('lw_im', None)
    fn = O.ld_atss_loss_block if fl == 'atss' else O.ld_fcos_loss_block
    o = fn(m['cls'], m['reg'], m['ctr'], m['t_cls'], m['t_reg'], raw, ohp)
    table[[0, 1, 3, 4, 5, 6]] = o['losses']
    g = o['grads']
    return dict(losses=table, grads=dict(cls=g['cls'], reg=g['reg'], x=None,
                                         kd=None, ctr=g['ctr']))


def _n(pos_per_level, pos_per_image, vlr_per_level, im_per_level=(0, ) * 5):
    return dict(pos_per_level=list(pos_per_level),
                pos_per_image=list(pos_per_image),
                vlr_per_level=list(vlr_per_level),
                im_per_level=list(im_per_level))


_Z = [0] * 5
# (geometry, target kernel) -> positives per level and per image, VLR cells and
# IM cells per level.  Every case carries its row as claims['counts']; the
# host test recounts it from the oracle's targets with ``==``.  LDHead,
# LDv2Head and LDATSSHead share the ATSS targets; FCOS "VLR" = its "remain"
# points; FCOS and Retina have no IM region.
COUNTS = {
    ('empty_beside_full', 'atss'): _n([6, 9, 0, 0, 0], [0, 15],
                                      [178, 63, 16, 0, 0], [121, 33, 0, 0, 0]),
    ('all_empty', 'atss'): _n(_Z, [0, 0], _Z),
    ('one_empty', 'atss'): _n(_Z, [0], _Z),
    ('ragged', 'atss'): _n([11, 27, 0, 0, 0], [0, 38], [227, 100, 30, 0, 0],
                           [221, 77, 3, 0, 0]),
    ('ten_blocks', 'atss'): _n([31, 9, 0, 0, 0], [31, 0, 9],
                               [270, 152, 37, 0, 0], [417, 152, 25, 0, 0]),
    ('pos_every_level', 'atss'): _n([7, 5, 6, 2, 1], [9, 12],
                                    [65, 24, 6, 2, 1], [21, 18, 6, 2, 1]),
    ('empty_beside_full', 'fcos'): _n([6, 13, 0, 0, 0], [0, 19],
                                      [250, 51, 16, 4, 1]),
    ('all_empty', 'fcos'): _n(_Z, [0, 0], _Z),
    ('ragged', 'fcos'): _n([6, 30, 2, 0, 0], [0, 38], [496, 93, 30, 7, 2]),
    ('ten_blocks', 'fcos'): _n([19, 10, 6, 0, 0], [29, 0, 6],
                               [438, 115, 15, 12, 2]),
    ('pos_every_level', 'fcos'): _n([9, 9, 6, 2, 1], [9, 18],
                                    [183, 39, 6, 2, 1]),
    ('empty_beside_full', 'retina'): _n([9, 37, 22, 0, 0], [0, 68],
                                        [1022, 469, 144, 21, 0]),
    ('all_empty', 'retina'): _n(_Z, [0, 0], _Z),
    ('ragged', 'retina'): _n([18, 53, 25, 0, 0], [0, 96],
                             [1402, 657, 259, 34, 0]),
    ('ten_blocks', 'retina'): _n([52, 10, 7, 0, 0], [62, 0, 7],
                                 [1812, 952, 329, 74, 0]),
    ('pos_every_level', 'retina'): _n([18, 31, 24, 13, 8], [32, 62],
                                      [291, 147, 54, 18, 9]),
}


def _base(geom, flavour, seed, hp=None, **kw):
    g = geometry(geom)
    H = dict(HP[flavour])
    H.update(hp or {})
    if flavour == 'v2':   # GFocalHead: cls_out_channels = num_classes + 1
        H['cls_channels'] = H.get('num_classes', 80) + 1
    N = len(g['boxes'])
    maps = head_inputs(flavour, N, g['sizes'], seed,
                       num_classes=H.get('num_classes', 80),
                       feat_channels=H.get('feat_channels', 256))
    NC = H.get('num_classes', 80)
    labels = [l % NC for l in g['labels']]
    fam = flavour if flavour in ('fcos', 'retina') else 'atss'
    kw['claims'] = dict(kw['claims'], counts=COUNTS[geom, fam])
    return dict(flavour=flavour, geometry=geom, sizes=g['sizes'],
                strides=STRIDES, metas=g['metas'], boxes=g['boxes'],
                labels=labels, maps=maps, hp=H, overrides=[],
                num_base=RETINA_B if flavour == 'retina' else 1, **kw)


# ------------------------------------------------------------ the cases ----
def empty_beside_full(flavour):
    """An image without a GT box beside one with three; level 0 is exactly one
    256-anchor block, level 1 exactly one 64-lane wave."""
    claims = dict(empty_images=1, level_cells=[256, 64, 16, 4, 1])
    return _base('empty_beside_full', flavour, 31, claims=claims)


def all_empty(flavour):
    """No positive in the batch: every divisor guard, every P_l == 0 guard."""
    return _base('all_empty', flavour, 32,
                 claims=dict(empty_images=2, total_pos=0))


def one_empty(flavour):
    """N = 1 and no GT box."""
    return _base('one_empty', flavour, 33,
                 claims=dict(empty_images=1, total_pos=0))


def ragged(flavour, **hp):
    """Level tails (561 = 2 * 256 + 49 cells), odd packed bases, a margin of
    label weight 0 around the image with boxes, an empty image first."""
    claims = dict(empty_images=1, level_cells=[561, 153, 45, 15, 6])
    if flavour != 'fcos':   # FCOS has no valid-region mask
        claims.update(lw_zero_min=1)
    return _base('ragged', flavour, 34, hp=hp, claims=claims)


def ten_blocks(flavour):
    """10 blocks per image; an empty image in the middle; for the ATSS
    targets level 2 holds IM cells and no positive."""
    claims = dict(empty_images=1, blocks_per_image=10)
    if flavour in ('ld', 'v2', 'atss'):   # the ATSS target kernel
        claims.update(im_without_pos_levels=[2])
    return _base('ten_blocks', flavour, 35, claims=claims)


def pos_every_level(flavour):
    """A positive on every level, the 1-cell level included."""
    claims = dict(empty_images=0, level_cells=[96, 24, 6, 2, 1],
                  levels_with_pos=5)
    return _base('pos_every_level', flavour, 36, claims=claims)


def two_temperatures(flavour='ld', equal=False):
    """T_ld != T_ld_vlr (the dense kernel's third branch), and T = 1."""
    hp = dict(T_ld=1.0, T_ld_vlr=1.0, T_kd=1.0) if equal else \
        dict(T_ld=10.0, T_ld_vlr=4.0, T_kd=1.0)
    c = ragged(flavour, **hp)
    c['claims'] = dict(c['claims'], temperatures_differ=not equal)
    return c


def saturated(flavour='ld'):
    """Class logits from {+-30, +-100}; student reg rows one-hot x 200 or
    all-equal with the teacher the opposite."""
    c = _base('empty_beside_full', flavour, 37,
              claims=dict(empty_images=1, max_abs_logit=200.0))
    gen = torch.Generator().manual_seed(41)
    vals = torch.tensor([-100.0, -30.0, 30.0, 100.0])
    m = c['maps']
    # LDv2Head: the KD term's raw maps saturate, ``cls`` stays probabilities
    for k in ('kd_s', 'kd_t') if flavour == 'v2' else ('cls', 't_cls'):
        m[k] = [vals[torch.randint(0, 4, t.shape, generator=gen)] for t in m[k]]
    for l, r in enumerate(m['reg']):
        N, _, h, w = r.shape
        hot = torch.randint(0, 17, (N, 4, 1, h, w), generator=gen)
        onehot = torch.zeros(N, 4, 17, h, w).scatter_(2, hot, 200.0)
        flat = torch.zeros(N, 4, 17, h, w) + 7.0
        pick = (torch.rand(N, 4, 1, h, w, generator=gen) < 0.5)
        m['reg'][l] = torch.where(pick, onehot, flat).reshape(r.shape)
        m['t_reg'][l] = torch.where(pick, flat, onehot).reshape(r.shape)
    return c


def student_is_teacher(flavour='ld', eps=0.0):
    """reg, cls and x equal to the teacher's (KL as a difference of O(1) terms
    cancels exactly), or 1e-3 away from it."""
    c = _base('ragged', flavour, 38, claims=dict(
        empty_images=1, equal=eps == 0.0))
    gen = torch.Generator().manual_seed(43)
    m = c['maps']
    for s, t in EQUAL_MAPS[flavour == 'v2']:
        m[s] = [(v + eps * (torch.rand(v.shape, generator=gen) - 0.5) * 2
                 ).float() if eps else v.clone() for v in m[t]]
    return c


# the student maps a distillation term reads, and the teacher's (LDv2Head: KD
# runs on the raw cls_feat maps, ``cls`` holds probabilities)
EQUAL_MAPS = {False: (('reg', 't_reg'), ('cls', 't_cls'), ('x', 't_x')),
              True: (('reg', 't_reg'), ('kd_s', 'kd_t'), ('x', 't_x'))}


def box_ties(flavour='ld', bbox_loss='giou'):
    """Positives whose four reg rows put 0.5 / 0.5 on two adjacent bins (the
    expectation is exactly k + 0.5 in both precisions, its derivative is not
    zero) and whose box target is rewritten so that predicted and target edges
    coincide on one, two and all four sides: the 0.5 / 0.5 sub-gradients of
    min / max in every box loss."""
    c = _base('empty_beside_full', flavour, 39, hp=dict(bbox_loss=bbox_loss),
              claims=dict(empty_images=1, tied_edges=[1, 2, 4]))
    t = oracle_targets(c)
    lab = t['labels']
    pos = np.argwhere((lab >= 0) & (lab < 80))
    assert len(pos) >= 3
    offs = np.cumsum([0] + [h * w for h, w in c['sizes']])
    bins = (3, 5, 4, 2)                     # k of (left, top, right, bottom)
    for i, tied in enumerate((1, 2, 4)):
        n, a = (int(v) for v in pos[i])
        l = int(np.searchsorted(offs, a, side='right') - 1)
        r, (h, w), s = a - offs[l], c['sizes'][l], STRIDES[l]
        cx, cy = float(r % w), float(r // w)
        for side, k in enumerate(bins):
            row = torch.full((17, ), -1000.0)
            row[k] = row[k + 1] = 0.0
            c['maps']['reg'][l][n, side * 17:(side + 1) * 17, r // w,
                                r % w] = row
        pred = np.array([cx - 3.5, cy - 5.5, cx + 4.5, cy + 2.5]) * s
        shift = np.array([-1.25, -0.75, 1.5, 0.5]) * s   # target edges off
        box = pred + shift
        box[:tied] = pred[:tied]                         # ... but `tied` of them
        c['overrides'].append((n, a, box.astype(F32)))
    return c


def classes(flavour='ld', n=17):
    """num_classes other than 80: 1, 17 (a ragged second chunk of 16), 128
    (kZMax chunks)."""
    ch = n + 1 if flavour == 'v2' else n
    return _base('ragged', flavour, 40, hp=dict(num_classes=n),
                 claims=dict(empty_images=1, cls_chunks=(ch + 15) // 16))


def feats(flavour='ld', n=48):
    """feat_channels other than 256: 8, 48 (a ragged chunk), 264 (chunks of
    33)."""
    chunk = max(32, (n + 7) // 8)
    return _base('ragged', flavour, 41, hp=dict(feat_channels=n),
                 claims=dict(empty_images=1, im_chunks=(n + chunk - 1) // chunk))


def prob_ends(flavour='v2'):
    """LD_LOSS_PROB_CLS: probabilities of exactly 0 and 1 at a positive's
    label channel and at negative entries (bce_prob's -100 clamp and its 1e-12
    floor)."""
    assert flavour == 'v2'
    c = _base('empty_beside_full', 'v2', 42,
              claims=dict(empty_images=1, prob_zero_one=[4, 4]))
    t = oracle_targets(c)
    pos = np.argwhere((t['labels'] >= 0) & (t['labels'] < 80))
    offs = np.cumsum([0] + [h * w for h, w in c['sizes']])
    for i, (n, a) in enumerate(pos[:4]):
        l = int(np.searchsorted(offs, a, side='right') - 1)
        r, (h, w) = a - offs[l], c['sizes'][l]
        lab = int(t['labels'][n, a])
        m = c['maps']['cls'][l]
        m[n, lab, r // w, r % w] = float(i % 2)            # label channel: 0, 1
        m[n, (lab + 1) % 81, r // w, r % w] = float(1 - i % 2)
        # and at a background cell of the empty image
        m[0, i, 0, i % w] = float(i % 2)
    return c


CASES = dict(
    empty_beside_full=empty_beside_full, all_empty=all_empty,
    one_empty=one_empty, ragged=ragged, ten_blocks=ten_blocks,
    pos_every_level=pos_every_level,
    two_temperatures=two_temperatures,
    two_temperatures_t1=functools.partial(two_temperatures, equal=True),
    saturated=saturated, student_is_teacher=student_is_teacher,
    student_near_teacher=functools.partial(student_is_teacher, eps=1e-3),
    classes_1=functools.partial(classes, n=1),
    classes_17=functools.partial(classes, n=17),
    classes_128=functools.partial(classes, n=128),
    feat_8=functools.partial(feats, n=8),
    feat_48=functools.partial(feats, n=48),
    feat_264=functools.partial(feats, n=264),
    prob_ends=prob_ends,
    **{f'box_ties_{m}': functools.partial(box_ties, bbox_loss=m)
       for m in ('giou', 'iou', 'iou_linear', 'diou', 'ciou')})

SIDE_CASES = ('empty_beside_full', 'all_empty', 'ragged', 'pos_every_level',
              'ten_blocks')
# LDv2Head's class maps hold num_classes + 1 channels: 127 classes are its
# kZMax chunks (128 classes = 129 channels are refused, as 129 are for LDHead)
CASES['classes_127'] = functools.partial(classes, n=127)
NOT_LD = ('prob_ends', 'classes_127')   # LD_LOSS_PROB_CLS only
NOT_V2 = ('classes_128', )
# (case, flavour): LDHead and LDv2Head run the whole table where it applies,
# ATSS, FCOS and Retina the five geometry cases
PAIRS = [(c, 'ld') for c in CASES if c not in NOT_LD] + \
    [(c, 'v2') for c in CASES if c not in NOT_V2] + \
    [(c, f) for f in SIDE for c in SIDE_CASES]


def without_empty(case):
    """The case with its images without a GT box removed: what the reference
    itself can run (oracle/gen_golden.py --only loss_edges)."""
    keep = [i for i, b in enumerate(case['boxes']) if len(b)]
    B = case['num_base']
    rows = [i * B + j for i in keep for j in range(B)]
    c = dict(case)
    for k in ('metas', 'boxes', 'labels'):
        c[k] = [case[k][i] for i in keep]
    c['maps'] = {k: None if v is None else [t[rows].contiguous() for t in v]
                 for k, v in case['maps'].items()}
    assert not case['overrides']
    c['targets'] = oracle_targets(c)
    return c


@functools.lru_cache(maxsize=None)
def build(name, flavour):
    c = CASES[name](flavour)
    c['name'] = name
    c['targets'] = oracle_targets(c)
    return c


# ------------------------------------------------- the bar of the GPU tests ---
# max|gpu - ref64| <= K_ORACLE * e_oracle + F_SCALE * max|ref64| per output
# (tests/test_gpu_loss_edges.py states where the constants come from); the
# mutation test of tests/test_loss_ref64_host.py holds every wrong rule against
# the same bar.
K_ORACLE = 12.0
F_SCALE = 2.0 ** -22


@functools.lru_cache(maxsize=None)
def ref64(name, flavour):
    c = build(name, flavour)
    import _loss_ref64 as R
    return R.loss_block(flavour, c['maps'], c['targets'], c['hp'],
                        num_base=c['num_base'])


def outputs(res):
    """{output name: flat float64 array}: 8 loss rows + the gradient families."""
    out = {f'row{r}': np.asarray(res['losses'][r], np.float64)
           for r in range(8)}
    for k, g in res['grads'].items():
        if g is not None:
            out['g' + k] = np.concatenate(
                [np.asarray(a, np.float64).reshape(-1) for a in g])
    return out


@functools.lru_cache(maxsize=None)
def oracle_error(name, flavour):
    """{output: max|oracle - ref64|} of the float32 numpy oracle."""
    c = build(name, flavour)
    if c['hp'].get('bbox_loss', 'giou') != 'giou':
        assert name.startswith('box_ties')
        return oracle_error('box_ties_giou', flavour)
    o = oracle_block(c, c['targets'])
    ref = outputs(ref64(name, flavour))
    return {k: float(np.abs(v - ref[k]).max())
            for k, v in outputs(o).items()}


