"""The dense heads with mmdet's constructor arguments, state_dict keys and
method signatures (reference: mmdet/models/dense_heads/gfl_head.py:15-625,
ld_head.py:43-637, anchor_head.py:14-173, base_dense_head.py:6-59 and the
atss_gfl / fcos_gfl / retina_gfl / gfocal heads with their ld_* variants).

Class layout (plain inheritance, one private base):

    _DenseHead            towers + init, packed forward trunk, _hp defaults,
      |                   config checks, _run_block (the ONE loss-block call),
      |                   _loss_dict, both forward_train bodies, _get_bboxes
      +- GFLHead          <- LDHead (_FeatureLD)
      |    +- ATSSGFLHead <- LDATSSHead (_SideLD)
      |    +- GFocalHead  <- LDv2Head (_FeatureLD)
      +- FCOSGFLHead      <- LDFCOSHead (_SideLD)
      +- RetinaGFLHead    <- LDRetinaHead (_SideLD)
      +- ATSSHead, RetinaHead   plain_heads.py (_DeltaBox: 4 deltas per
                                anchor); they share _ATSSFamily / _RetinaFamily
                                with ATSSGFLHead / RetinaGFLHead

A head states its constructor, its predictor convs (``_predictors``), its
targets and what differs in ``_hp`` / ``_check_loss_cfg``.  ``_FeatureLD`` is
the LD loss that reads the neck features (imitation), ``_SideLD`` the one that
does not.  Modules are registered in the reference's order (``integral`` after
the layers): state_dict, parameter and init-draw order are part of the
checkpoint and optimizer formats (tests/test_heads_contract_host.py).

MI355X-native execution:
  * forward: the five FPN levels are concatenated into one (N, C, P) tensor
    and every weight-shared tower conv / GroupNorm / predictor runs as ONE
    launch over all levels (the reference runs 5 x 10 small convs);
  * loss: anchors are never materialised, targets come from two batched
    launches (targets.hip) and the whole loss_single x 5 levels, forward AND
    gradient, is the fused block of loss.hip, reading the NCHW head outputs in
    place.  No host synchronisation: the two normalisers stay on the device
    (the reference does ~90 .item()/nonzero syncs per step).
"""
import torch
import torch.nn as nn

from . import layers as Y
from . import lib as L
from . import lossblock as LB
from .losses import bbox_loss_mode
from .cnn import ConvModule, Conv2d, Scale, bias_init_with_prob, normal_init
from .registry import (HEADS, build_anchor_generator, build_assigner,
                       build_bbox_coder, build_iou_calculator, build_loss,
                       build_sampler)

LOSS_KEYS = L.LOSS_KEYS


class Integral(nn.Module):
    """gfl_head.py:15-44: expectation of the softmax over {0..reg_max}."""

    def __init__(self, reg_max=16):
        super().__init__()
        self.reg_max = reg_max
        self.register_buffer('project',
                             torch.linspace(0, self.reg_max, self.reg_max + 1))

    def forward(self, x):
        return _IntegralFn.apply(x.reshape(-1, 4 * (self.reg_max + 1)))


class _IntegralFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x):
        x = L.require_device(x.contiguous(), torch.float32, 'integral input')
        if x.shape[1] != 68:
            raise NotImplementedError('reg_max != 16')
        out = x.new_empty((x.shape[0], 4))
        if x.shape[0]:
            L.check(L.get_lib().ld_integral_rows(L.ptr(x), x.shape[0],
                                                 L.ptr(out),
                                                 L.stream_ptr(x.device)),
                    'ld_integral_rows')
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        gx = torch.empty_like(x)
        if x.shape[0]:
            L.check(L.get_lib().ld_integral_rows_bwd(L.ptr(x),
                                                     L.ptr(g.contiguous()),
                                                     x.shape[0], L.ptr(gx),
                                                     L.stream_ptr(x.device)),
                    'ld_integral_rows_bwd')
        return gx


class LossDict(dict):
    """dict[str, list[Tensor]] as the reference returns, plus the (8, L) device
    table it is a view of, so _parse_losses can reduce it in two launches."""
    table = None
    rows = None


def _imitation_flags(method, lw_im):
    """hp flags of the imitation region (ld_head.py:170-191,580-611).
    'finegrained': IoU > 0.5 max IoU per GT.  'fitnet': anchor centre strictly
    inside a GT.  'gibox': the GI boxes (selected after the forward; the region
    flag only matters for its weight-0 evaluation).  'decouple' adds
    ``2 * mse(x[outside], teacher_x[inside])`` -- two row sets of different
    sizes, which F.mse_loss cannot broadcast: the reference itself raises on
    that branch, so there is nothing to reproduce."""
    if method == 'decouple' and lw_im != 0.0:
        raise NotImplementedError(
            "imitation_method='decouple': ld_head.py:176-183 evaluates "
            'mse_loss(x[ng_inds], teacher_x[fg_inds]) on row sets of different '
            'sizes, which raises in the reference as well')
    return L.LD_IM_CENTER_INSIDE if method in ('fitnet', 'decouple',
                                               'gibox') else 0


class LazyScalars(dict):
    """dict of python floats backed by one device tensor; the single D2H copy
    happens on first access (the reference syncs 9 times per step).

    It stays a ``dict`` subclass because mmcv's LogBuffer.update asserts
    ``isinstance(vars, dict)``; every read path -- including the ones CPython
    serves from the raw table for plain dicts (``dict(x)``, ``{**x}``,
    ``OrderedDict(x)``, ``copy()``) -- is routed through the sync: overriding
    ``__iter__``/``keys`` takes ``dict_merge`` off its fast path."""

    def __init__(self, keys, tensor):
        super().__init__()
        self._keys, self._tensor, self._done = list(keys), tensor, False
        for k in keys:
            dict.__setitem__(self, k, None)

    def _sync(self):
        if not self._done:
            vals = self._tensor.detach().cpu().tolist()
            for k, v in zip(self._keys, vals):
                dict.__setitem__(self, k, v)
            self._done = True

    def __getitem__(self, k):
        self._sync()
        return dict.__getitem__(self, k)

    def get(self, k, default=None):
        self._sync()
        return dict.get(self, k, default)

    def __iter__(self):
        self._sync()
        return dict.__iter__(self)

    def keys(self):
        self._sync()
        return dict.keys(self)

    def items(self):
        self._sync()
        return dict.items(self)

    def values(self):
        self._sync()
        return dict.values(self)

    def copy(self):
        self._sync()
        return dict(dict.items(self))

    def pop(self, *a):
        self._sync()
        return dict.pop(self, *a)

    def setdefault(self, k, default=None):
        self._sync()
        return dict.setdefault(self, k, default)

    def __eq__(self, other):
        self._sync()
        return dict.__eq__(self, other)

    def __ne__(self, other):
        return not self.__eq__(other)

    __hash__ = None

    def __repr__(self):
        self._sync()
        return dict.__repr__(self)

    def __reduce__(self):
        self._sync()
        return (dict, (dict(dict.items(self)), ))


def _tower(convs, x3, levels):
    """A stack of ConvModules on the level-concatenated tensor.  Every layer but
    the last is told that its output feeds another conv of the stack (c8_out): a
    frozen conv + GN layer in bf16 mode then keeps only the bf16 C8 image of its
    output (the teacher's towers; cnn.ConvModule.forward3)."""
    last = len(convs) - 1
    for i, m in enumerate(convs):
        x3, _ = m.forward3(x3, levels, c8_out=i < last)
    return x3


class BBoxTestMixin:
    """Test-time augmentation of the dense heads (anchor_head.py:729,
    anchor_free_head.py:324 -> dense_test_mixins.py:38-100): per view the
    head forward and get_bboxes(rescale=False, with_nms=False), then ONE
    device call (ld_aug_merge_nms) maps every view back to the original image,
    merges them view-major and runs multiclass_nms over the merged set."""

    def aug_test(self, feats, img_metas, rescale=False,
                 return_device_dets=False):
        """``feats``: per view the FPN levels of ONE image; ``img_metas``: per
        view a one-element list of metas (img_shape, scale_factor, flip,
        flip_direction).  -> bbox2result per-class arrays of the image; with
        ``return_device_dets`` ``(arrays, (dets (k, 5), labels (k,)))``, the
        merged device detections beside them."""
        from .core import bbox2result
        cfg = self.test_cfg
        if cfg is None:
            raise ValueError('aug_test needs a test_cfg')
        if len(feats) != len(img_metas):
            raise ValueError(f'{len(feats)} views of features but '
                             f'{len(img_metas)} of image metas')
        get = cfg.get if hasattr(cfg, 'get') else lambda k, d=None: cfg[k]
        nms = get('nms')
        nms_type = nms.get('type', 'nms')
        views = []
        for x, metas in zip(feats, img_metas):
            # the reference reads image 0 of every view (dense_test_mixins.py:71)
            if len(metas) != 1:
                raise ValueError('aug_test: one image per view (the reference '
                                 'reads only image 0 of each view, '
                                 'dense_test_mixins.py:71)')
            outs = self(x)
            res = self.get_bboxes(*outs, metas, rescale=False,
                                  with_nms=False)[0]
            m = metas[0]
            views.append(dict(
                boxes=res[0], scores=res[1],
                factors=res[2] if len(res) > 2 else None,
                img_shape=m['img_shape'], scale_factor=m['scale_factor'],
                flip=m.get('flip', False),
                flip_direction=m.get('flip_direction')))
        voting = nms_type == 'voting_cluster_diounms'
        if voting and views[0]['factors'] is not None:
            raise NotImplementedError('score voting with centerness factors')
        dets, labels = LB.aug_merge_nms(
            views, score_thr=get('score_thr'), iou_thr=nms['iou_threshold'],
            max_per_img=get('max_per_img'), voting=voting, rescale=rescale,
            num_classes=self.cls_out_channels)
        result = bbox2result(dets, labels, self.num_classes)
        return (result, (dets, labels)) if return_device_dets else result


ATSS_LOSS_KEYS = ['loss_cls', 'loss_bbox', 'loss_ld', 'loss_ld_neg',
                  'loss_cls_kd', 'loss_centerness']
# rows of the fused block's (8, L) table that carry them (LD_LOSS_ATSS)
_ATSS_ROWS = [0, 1, 3, 4, 5, 6]
RETINA_LOSS_KEYS = ['loss_cls', 'loss_bbox', 'loss_ld', 'loss_ld_vlr',
                    'loss_cls_kd']
# rows of the fused block's (8, L) table that carry them (LD_LOSS_RETINA)
_RETINA_ROWS = [0, 1, 3, 4, 5]

# the loss_bbox types the fused block evaluates, by their make_hp names
_BOX_LOSSES = 'one of the box losses ' + ', '.join(L.LD_LOSS_BBOX_MODES)


class _DenseHead(BBoxTestMixin, nn.Module):
    """What the five plain heads share: the two towers and their init, the
    level-packed forward trunk, the hyper-parameter struct, the config checks,
    the fused loss-block call with its loss dict, forward_train and the
    device-side get_bboxes.  A subclass states its constructor, its predictor
    convs (``_predictors``), its targets and what differs in ``_hp``."""
    # predictor attributes in the reference's init order; the first one gets
    # the bias prior
    _predictors = ()
    # LDHead / LDv2Head: their loss reads the features
    _wants_packed_feats = False
    # keys of the loss dict, the table rows that carry them (None: row i for
    # key i) and the keys of the plain (teacher-less) loss
    _loss_keys, _loss_rows = LOSS_KEYS, None
    _plain_keys = ('loss_cls', 'loss_bbox', 'loss_dfl')

    # ------------------------------------------------------------- layers --
    # channels per anchor of the box branch
    @property
    def _reg_out(self):
        return 4 * (self.reg_max + 1)

    def _init_anchor_head(self, num_classes, in_channels, feat_channels,
                          stacked_convs, conv_cfg, norm_cfg, anchor_generator,
                          bbox_coder, reg_decoded_bbox, loss_cls, loss_bbox,
                          train_cfg, test_cfg):
        """AnchorHead.__init__ (anchor_head.py:31-96) with the tower arguments
        its subclasses add; ends with the head's ``_init_layers()``."""
        self.stacked_convs, self.conv_cfg, self.norm_cfg = (stacked_convs,
                                                            conv_cfg, norm_cfg)
        self.in_channels, self.num_classes = in_channels, num_classes
        self.feat_channels = feat_channels
        self.use_sigmoid_cls = loss_cls.get('use_sigmoid', False)
        self.sampling = loss_cls['type'] not in [
            'FocalLoss', 'GHMC', 'QualityFocalLoss']
        self.cls_out_channels = num_classes if self.use_sigmoid_cls \
            else num_classes + 1
        if self.cls_out_channels <= 0:
            raise ValueError(f'num_classes={num_classes} is too small')
        self.reg_decoded_bbox = reg_decoded_bbox
        self.bbox_coder = build_bbox_coder(bbox_coder)
        self.loss_cls = build_loss(loss_cls)
        self.loss_bbox = build_loss(loss_bbox)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        if self.train_cfg:
            self.assigner = build_assigner(self.train_cfg.assigner)
            self.sampler = build_sampler(dict(type='PseudoSampler'),
                                         context=self)
        self.fp16_enabled = False
        self.anchor_generator = build_anchor_generator(anchor_generator)
        self.num_anchors = self.anchor_generator.num_base_anchors[0]
        # d(total)/d(loss_k) == 1 is promised by BaseDetector._parse_losses;
        # SGDTrainer.step sets this for the duration of a train step so the
        # backward reuses the gradient the fused forward launch already produced
        self.unit_upstream = False
        self._init_layers()

    def _build_towers(self, bias='auto'):
        """The cls / reg conv stacks (gfl_head.py:102-121 and the same loop of
        atss_gfl_head.py, fcos_gfl_head.py and retina_gfl_head.py; ``bias``:
        anchor_free_head.py:93-127 hands its conv_bias to every layer)."""
        self.relu = nn.ReLU(inplace=True)
        self.cls_convs = nn.ModuleList()
        self.reg_convs = nn.ModuleList()
        for i in range(self.stacked_convs):
            chn = self.in_channels if i == 0 else self.feat_channels
            self.cls_convs.append(
                ConvModule(chn, self.feat_channels, 3, stride=1, padding=1,
                           conv_cfg=self.conv_cfg, norm_cfg=self.norm_cfg,
                           bias=bias))
            self.reg_convs.append(
                ConvModule(chn, self.feat_channels, 3, stride=1, padding=1,
                           conv_cfg=self.conv_cfg, norm_cfg=self.norm_cfg,
                           bias=bias))

    def _build_scales(self, strides):
        self.scales = nn.ModuleList([Scale(1.0) for _ in strides])

    def init_weights(self):
        """gfl_head.py:135-143, atss_gfl_head.py:127-137, fcos_gfl_head.py:
        167-176, retina_gfl_head.py:266-274: towers, then the predictors."""
        for m in self.cls_convs:
            normal_init(m.conv, std=0.01)
        for m in self.reg_convs:
            normal_init(m.conv, std=0.01)
        for i, name in enumerate(self._predictors):
            normal_init(getattr(self, name), std=0.01,
                        bias=bias_init_with_prob(0.01) if i == 0 else 0)

    # ------------------------------------------------------------ forward --
    def _trunk(self, feats):
        """feats: tuple of per-level (N, C, H, W) -> the two tower outputs on
        the level-concatenated tensor, one launch per layer for all levels."""
        scales = getattr(self, 'scales', None)
        assert scales is None or len(feats) == len(scales)
        return self._trunk3(*self._pack(feats))

    def _trunk3(self, x3, levels):
        return (_tower(self.cls_convs, x3, levels),
                _tower(self.reg_convs, x3, levels), levels)

    def forward_packed(self, x3, levels):
        """``forward`` on a head input that is already level-concatenated:
        ``x3`` (N, C, P) contiguous fp32 and its ``levels`` ((H, W), ...), as
        ``layers.pack_levels`` returns them.  Nothing is packed or copied; the
        outputs are those of ``forward`` on the level views of ``x3``."""
        levels = tuple((int(h), int(w)) for h, w in levels)
        scales = getattr(self, 'scales', None)
        if scales is not None and len(levels) != len(scales):
            raise ValueError(f'forward_packed: {len(levels)} levels for a head '
                             f'of {len(scales)}')
        if x3.dim() != 3 or x3.shape[1] != self.in_channels or \
                x3.shape[2] != sum(h * w for h, w in levels):
            raise ValueError(
                f'forward_packed: input {tuple(x3.shape)} is not (N, '
                f'{self.in_channels}, P) with P the positions of {levels}')
        if not x3.is_contiguous():
            raise ValueError('forward_packed: the input must be contiguous')
        self._packed = None
        return self._predict(*self._trunk3(x3, levels))

    def _scale(self, reg3, levels):
        """The per-level learnable Scale of the box branch."""
        return Y.scale_levels(reg3, torch.stack([s.scale for s in self.scales]),
                              levels)

    def _pack(self, feats):
        """The level-concatenated head input; remembered for ``_loss_feats``
        while a gradient is wanted."""
        x3, levels = Y.pack_levels(feats)
        self._packed = (x3, levels) if self._wants_packed_feats and \
            torch.is_grad_enabled() and x3.requires_grad and \
            len(feats) > 1 else None
        return x3, levels

    def _loss_feats(self, x):
        """The neck features the LD loss block reads (ld_head.py:284-375: ``x``
        for the imitation term): the level VIEWS of the packed head input --
        the same values as ``x``, but the imitation gradient then re-enters the
        graph at the packed tensor, where the first tower conv's data gradient
        sums it in its epilogue (layers.fan_*), instead of five per-level
        elementwise adds at the neck outputs."""
        pk, self._packed = getattr(self, '_packed', None), None
        return x if pk is None else Y.split_levels(*pk)

    def forward_single(self, x, scale):
        raise NotImplementedError(
            'use forward(feats): all levels run in one launch per layer')

    def anchor_center(self, anchors):
        """gfl_head.py:185-194."""
        cx = (anchors[..., 2] + anchors[..., 0]) / 2
        cy = (anchors[..., 3] + anchors[..., 1]) / 2
        return torch.stack([cx, cy], dim=-1)

    def get_anchors(self, featmap_sizes, img_metas, device='cuda'):
        """anchor_head.py:145-173 (API compatibility; the loss never calls
        it)."""
        num_imgs = len(img_metas)
        multi_level_anchors = self.anchor_generator.grid_anchors(
            featmap_sizes, device)
        anchor_list = [multi_level_anchors for _ in range(num_imgs)]
        valid_flag_list = []
        for meta in img_metas:
            valid_flag_list.append(
                self.anchor_generator.valid_flags(featmap_sizes,
                                                  meta['pad_shape'], device))
        return anchor_list, valid_flag_list

    # --------------------------------------------------------------- loss --
    def _hp(self, **over):
        """The loss block's hyper-parameters.  Here: what every head reads off
        its loss modules, no DFL, no distillation; a subclass passes what
        differs."""
        kw = dict(
            num_classes=self.num_classes,
            reg_max=getattr(self, 'reg_max', 16), topk=9,
            feat_channels=self.feat_channels,
            lw_cls=self.loss_cls.loss_weight, qfl_beta=2.0,
            lw_bbox=self.loss_bbox.loss_weight,
            giou_eps=getattr(self.loss_bbox, 'eps', 1e-6),
            bbox_loss=bbox_loss_mode(self.loss_bbox) or 'giou', lw_dfl=0.0,
            lw_ld=0.0, T_ld=1.0, lw_ld_vlr=0.0, T_ld_vlr=1.0, lw_kd=0.0,
            T_kd=1.0, lw_im=0.0)
        kw.update(over)
        return LB.make_hp(**kw)

    def _check_train_cfg(self):
        if self.train_cfg.get('allowed_border', -1) >= 0:
            raise NotImplementedError('allowed_border >= 0')
        if self.train_cfg.get('pos_weight', -1) > 0:
            raise NotImplementedError('pos_weight > 0')

    def _check_focal_cfg(self, family, centerness):
        """The heads that train with FocalLoss (and a sigmoid-CE centerness)."""
        from .losses import CrossEntropyLoss, FocalLoss
        ok = isinstance(self.loss_cls, FocalLoss) and \
            bbox_loss_mode(self.loss_bbox) is not None
        if centerness:
            ok = ok and isinstance(self.loss_centerness, CrossEntropyLoss) \
                and self.loss_centerness.use_sigmoid
        if not ok:
            raise NotImplementedError(
                f'the fused {family} loss block implements FocalLoss + '
                f'{_BOX_LOSSES}' +
                (' + sigmoid CrossEntropyLoss centerness' if centerness else
                 ''))
        if self.loss_cls.gamma != 2.0:
            raise NotImplementedError('FocalLoss gamma != 2')

    @staticmethod
    def _norm_reducer():
        """Cross-rank mean of (num_total_pos, sum weight_targets): ONE device
        side all-reduce instead of the reference's two reduce_mean(...).item()
        host syncs (ld_head.py:338-341,362-363)."""
        import torch.distributed as dist
        from .train import _diag_skip, all_reduce_or_record, collectives_on
        slot = LB.virtual_norm_slot()
        if slot is not None:
            # SGDTrainer(virtual_ranks=W): this micro-batch's partials go into
            # its row of the step's table; the block's main part runs once the
            # mean over the W rows exists (lossblock.DeferredNorm)
            return slot
        if not collectives_on() or _diag_skip('norm'):
            return None
        ws = float(dist.get_world_size())

        def _r(norm):
            all_reduce_or_record(norm)
            norm.div_(ws)

        return _r

    def _loss_dict(self, table, keys=LOSS_KEYS, rows=None, want=None):
        """The (8, L) table as the reference's dict of per-level scalars:
        ``keys[i]`` from row ``rows[i]``, only the keys in ``want``."""
        pairs = [(k, r) for k, r in zip(keys, rows or range(len(keys)))
                 if want is None or k in want]
        d = LossDict((k, [table[r, l] for l in range(table.shape[1])])
                     for k, r in pairs)
        d.table, d.rows = table, [r for _, r in pairs]
        return d

    def _level_sizes(self, cls_scores, num_levels):
        sizes = [tuple(int(v) for v in f.shape[-2:]) for f in cls_scores]
        assert len(sizes) == num_levels
        return sizes

    def get_targets_batched(self, featmap_sizes, img_metas, gt_bboxes,
                            gt_labels, hp, device):
        """AnchorHead.get_anchors + LDHead.get_targets for the whole batch in
        two launches (ld_head.py:377-577)."""
        strides = [s[0] for s in self.anchor_generator.strides]
        if not self.anchor_generator.single_square:
            # the implicit-anchor kernels build the one square anchor of a cell
            # from an INTEGER scale (octave_base_scale * stride)
            raise NotImplementedError(
                f'{type(self).__name__}: one anchor per cell with a non-integer '
                'scale or ratio != 1 (anchor_generator.py:78-98); the '
                'single-anchor target kernels take ratios=[1.0] with an integer '
                'octave_base_scale')
        if gt_labels is None:
            gt_labels = [b.new_zeros(b.shape[0], dtype=torch.long)
                         for b in gt_bboxes]
        return LB.atss_targets(featmap_sizes, strides, img_metas, gt_bboxes,
                               gt_labels, hp, device,
                               self.anchor_generator.anchor_scale)

    def _targets(self, hp, cls_scores, img_metas, gt_bboxes, gt_labels):
        sizes = self._level_sizes(cls_scores, self.anchor_generator.num_levels)
        return self.get_targets_batched(sizes, img_metas, gt_bboxes, gt_labels,
                                        hp, cls_scores[0].device)

    def _run_block(self, hp, targets, outs, teacher, feats=None, extra=(),
                   reduce_norm=True, want=None):
        """The fused loss block on ``outs`` = (cls_scores, bbox_preds).
        ``teacher`` = (cls, reg, x[, kd]) maps, detached here; ``extra`` the
        fourth student group (centernesses, or GFLv2's cls_feat).  ``feats`` =
        None for a loss that reads no features: the student's own class maps
        stand in for both feature sets (their term has weight zero)."""
        cls_scores, bbox_preds = outs
        teacher = [ts and [t.detach() for t in ts] for ts in teacher]
        if feats is None:
            feats = teacher[2] = [c.detach() for c in cls_scores]
            hp.feat_channels = feats[0].shape[1]
        table, _ = LB.LDLossBlock.apply(
            hp, targets, tuple(teacher),
            self._norm_reducer() if reduce_norm else None, self.unit_upstream,
            *cls_scores, *bbox_preds, *feats, *extra)
        self.last_targets = targets
        return self._loss_dict(table, self._loss_keys, self._loss_rows, want)

    def _loss(self, outs, gt_bboxes, gt_labels, img_metas, teacher=None,
              extra=(), **hp_over):
        """check -> hp -> targets -> block for the losses that read no
        features.  Without a teacher the student's own detached outputs are
        fed (every distillation weight is zero) and the plain keys returned."""
        self._check_loss_cfg()
        hp = self._hp(**hp_over)
        targets = self._targets(hp, outs[0], img_metas, gt_bboxes, gt_labels)
        if teacher is None:
            return self._run_block(hp, targets, outs, (*outs, None),
                                   extra=extra, want=self._plain_keys)
        return self._run_block(hp, targets, outs, (*teacher[:2], None),
                               extra=extra)

    def forward_train(self, x, img_metas, gt_bboxes, gt_labels=None,
                      gt_bboxes_ignore=None, proposal_cfg=None, **kwargs):
        """base_dense_head.py:20-59."""
        outs = self(x)
        if proposal_cfg is not None:
            raise NotImplementedError('proposal_cfg')
        return self.loss(*outs, gt_bboxes, gt_labels, img_metas,
                         gt_bboxes_ignore=gt_bboxes_ignore)

    def _forward_train_ld(self, x, out_teacher, teacher_x, img_metas,
                          gt_bboxes, gt_labels, gt_bboxes_ignore, proposal_cfg):
        """forward_train of the LD heads (ld_head.py:73-114, ld_gflv2.py:
        74-114, ld_atss.py:252-290, ld_fcos_head.py:219-259, ld_retina.py:
        139-185).  ``teacher_x`` = None for the heads whose loss reads no
        features."""
        outs = self(x)
        if gt_labels is None:
            raise NotImplementedError(f'{type(self).__name__} needs gt_labels')
        if proposal_cfg is not None:
            raise NotImplementedError('proposal_cfg')
        soft = (out_teacher, ) if teacher_x is None else \
            (out_teacher, self._loss_feats(x), teacher_x)
        return self.loss(*outs, gt_bboxes, gt_labels, *soft, img_metas,
                         gt_bboxes_ignore=gt_bboxes_ignore)

    # ---------------------------------------------------------- inference --
    def _get_bboxes(self, cls_scores, bbox_preds, img_metas, cfg, rescale,
                    with_nms, prob, centernesses=None, points=False,
                    strides=None, num_base=1, delta=None, dist=False):
        cfg = self.test_cfg if cfg is None else cfg
        if cfg is None:
            raise ValueError('get_bboxes needs a test_cfg')
        nms = cfg['nms'] if isinstance(cfg, dict) else cfg.nms
        nms_type = nms.get('type', 'nms')
        if nms_type not in ('nms', 'voting_cluster_diounms'):
            raise NotImplementedError(
                f"nms type {nms_type!r}: the reference's multiclass_nms knows "
                "'nms' and 'voting_cluster_diounms' (bbox_nms.py:141-188)")
        get = cfg.get if hasattr(cfg, 'get') else lambda k, d=None: cfg[k]
        if get('min_bbox_size', 0) not in (0, -1):
            raise NotImplementedError('min_bbox_size > 0')
        if centernesses is not None and nms_type != 'nms' and with_nms:
            raise NotImplementedError('score voting with centerness factors')
        if not with_nms:
            nms_type = 'nms'  # the nms config is not consulted
        strides = [s[0] if isinstance(s, (tuple, list)) else s
                   for s in (strides or self.anchor_generator.strides)]
        N = cls_scores[0].shape[0]
        shapes = [img_metas[i]['img_shape'] for i in range(N)]
        sfs = [img_metas[i]['scale_factor'] for i in range(N)] if rescale \
            else None
        return LB.get_bboxes(
            [c.detach() for c in cls_scores], [b.detach() for b in bbox_preds],
            strides, shapes, sfs, nms_pre=get('nms_pre', -1),
            score_thr=get('score_thr'), iou_thr=nms['iou_threshold'],
            max_per_img=get('max_per_img'), num_classes=self.cls_out_channels,
            reg_max=getattr(self, 'reg_max', 16),
            voting=nms_type == 'voting_cluster_diounms',
            prob=prob, centernesses=None if centernesses is None else
            [c.detach() for c in centernesses], points=points,
            num_base=num_base, with_nms=with_nms, dist=dist,
            delta=delta and delta(cls_scores), **(
                dict(anchor_scale=self.anchor_generator.anchor_scale or 8)
                if delta else {}))


@HEADS.register_module()
class GFLHead(_DenseHead):
    """Constructor = AnchorHead.__init__ (anchor_head.py:31-96) +
    GFLHead.__init__ (gfl_head.py:76-100)."""
    _predictors = ('gfl_cls', 'gfl_reg')

    def __init__(self, num_classes, in_channels, stacked_convs=4,
                 conv_cfg=None,
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True),
                 loss_dfl=dict(type='DistributionFocalLoss', loss_weight=0.25),
                 reg_max=16, feat_channels=256,
                 anchor_generator=dict(type='AnchorGenerator', ratios=[1.0],
                                       octave_base_scale=8,
                                       scales_per_octave=1,
                                       strides=[8, 16, 32, 64, 128]),
                 bbox_coder=dict(type='DeltaXYWHBBoxCoder',
                                 target_means=(.0, .0, .0, .0),
                                 target_stds=(1.0, 1.0, 1.0, 1.0)),
                 reg_decoded_bbox=False,
                 loss_cls=dict(type='QualityFocalLoss', use_sigmoid=True,
                               beta=2.0, loss_weight=1.0),
                 loss_bbox=dict(type='GIoULoss', loss_weight=2.0),
                 train_cfg=None, test_cfg=None):
        super().__init__()
        self.reg_max = reg_max
        self._init_anchor_head(num_classes, in_channels, feat_channels,
                               stacked_convs, conv_cfg, norm_cfg,
                               anchor_generator, bbox_coder, reg_decoded_bbox,
                               loss_cls, loss_bbox, train_cfg, test_cfg)
        self.sampling = False  # gfl_head.py:93 overrides AnchorHead's value
        # after the layers, like the reference (state_dict key order)
        self.integral = Integral(self.reg_max)
        self.loss_dfl = build_loss(loss_dfl)

    def _init_layers(self):
        """gfl_head.py:102-133."""
        self._build_towers()
        assert self.num_anchors == 1, 'anchor free version'
        self.gfl_cls = Conv2d(self.feat_channels, self.cls_out_channels, 3,
                              padding=1)
        self.gfl_reg = Conv2d(self.feat_channels, 4 * (self.reg_max + 1), 3,
                              padding=1)
        self._build_scales(self.anchor_generator.strides)

    def forward(self, feats):
        """feats: tuple of per-level (N, C, H, W) -> (cls_scores, bbox_preds)
        lists (gfl_head.py:145-183)."""
        return self._predict(*self._trunk(feats))

    def _predict(self, cls_feat, reg_feat, levels):
        cls3, _ = self.gfl_cls.forward3(cls_feat, levels)
        reg3, _ = self.gfl_reg.forward3(reg_feat, levels)
        reg3 = self._scale(reg3, levels)
        return Y.split_levels(cls3, levels), Y.split_levels(reg3, levels)

    # --------------------------------------------------------------- loss --
    def _hp(self, **over):
        kw = dict(topk=self.assigner.topk,
                  qfl_beta=getattr(self.loss_cls, 'beta', 2.0),
                  lw_dfl=self.loss_dfl.loss_weight)
        kw.update(over)
        return super()._hp(**kw)

    def _check_loss_cfg(self):
        from .losses import QualityFocalLoss
        if not isinstance(self.loss_cls, QualityFocalLoss) or \
                bbox_loss_mode(self.loss_bbox) is None:
            raise NotImplementedError(
                'the fused loss block implements QualityFocalLoss + '
                f'{_BOX_LOSSES} (got {type(self.loss_cls).__name__}, '
                f'{type(self.loss_bbox).__name__})')
        self._check_train_cfg()

    def loss(self, cls_scores, bbox_preds, gt_bboxes, gt_labels, img_metas,
             gt_bboxes_ignore=None):
        """gfl_head.py:269-352 (plain GFL: QFL + GIoU + DFL)."""
        return self._loss((cls_scores, bbox_preds), gt_bboxes, gt_labels,
                          img_metas)

    def get_bboxes(self, cls_scores, bbox_preds, img_metas, cfg=None,
                   rescale=False, with_nms=True):
        """anchor_head.py:497-589 + gfl_head.py:354-451 + multiclass_nms, one
        C-ABI call for the whole batch (ld_get_bboxes).  Returns, per image,
        ``(det_bboxes (k, 5), det_labels (k,))`` like the reference."""
        return self._get_bboxes(cls_scores, bbox_preds, img_metas, cfg,
                                rescale, with_nms, prob=False)


class _FeatureLD:
    """LDHead / LDv2Head (ld_head.py:43-637, ld_gflv2.py:44-644): LD on the
    positives and on the valuable localisation region, KD on the class maps
    and feature imitation, whose loss reads the neck features of student and
    teacher.  The host class gives ``_split_teacher`` and its ``loss``
    signature."""
    _wants_packed_feats = True
    _feat256_ref = None  # where the reference hard-codes 256 channels

    def __init__(self, num_classes, in_channels,
                 loss_ld=dict(type='KnowledgeDistillationKLDivLoss',
                              loss_weight=0.25, T=10),
                 loss_ld_vlr=dict(type='KnowledgeDistillationKLDivLoss',
                                  loss_weight=0.25, T=10),
                 loss_kd=dict(type='KnowledgeDistillationKLDivLoss',
                              loss_weight=10, T=2),
                 loss_im=dict(type='IMLoss', loss_weight=0),
                 imitation_method='gibox', **kwargs):
        super().__init__(num_classes, in_channels, **kwargs)
        assert imitation_method in ['gibox', 'finegrained', 'fitnet',
                                    'decouple']
        self.imitation_method = imitation_method
        self.loss_im = build_loss(loss_im)
        self.loss_ld = build_loss(loss_ld)
        self.loss_ld_vlr = build_loss(loss_ld_vlr)
        self.loss_kd = build_loss(loss_kd)
        self.iou_calculator = build_iou_calculator(dict(type='BboxOverlaps2D'))

    def forward_train(self, x, out_teacher, teacher_x, img_metas, gt_bboxes,
                      gt_labels=None, gt_bboxes_ignore=None, proposal_cfg=None,
                      **kwargs):
        return self._forward_train_ld(x, out_teacher, teacher_x, img_metas,
                                      gt_bboxes, gt_labels, gt_bboxes_ignore,
                                      proposal_cfg)

    def _ld_loss(self, outs, gt_bboxes, gt_labels, soft_teacher, x, teacher_x,
                 img_metas, extra=()):
        """-> dict of 8 lists of per-level scalars (LOSS_KEYS)."""
        self._check_loss_cfg()
        lw_im = float(self.loss_im.loss_weight)
        im_flags = _imitation_flags(self.imitation_method, lw_im)
        if x[0].shape[1] != 256:
            raise ValueError(f'{type(self).__name__} hard-codes 256 feature '
                             f'channels ({self._feat256_ref})')
        hp = self._hp(lw_ld=self.loss_ld.loss_weight, T_ld=self.loss_ld.T,
                      lw_ld_vlr=self.loss_ld_vlr.loss_weight,
                      T_ld_vlr=self.loss_ld_vlr.T,
                      lw_kd=self.loss_kd.loss_weight, T_kd=self.loss_kd.T,
                      lw_im=lw_im)
        hp.flags |= im_flags
        targets = self._targets(hp, outs[0], img_metas, gt_bboxes, gt_labels)
        t_kd, t_reg, *fourth = self._split_teacher(soft_teacher)
        if self.imitation_method == 'gibox' and lw_im != 0.0:
            # ld_head.py:580-611; ld_gflv2.py:619-644 (there the raw teacher
            # cls_feat against the student's probabilities, no sigmoids)
            targets = LB.gi_region(hp, targets,
                                   [c.detach() for c in outs[0]],
                                   [b.detach() for b in outs[1]],
                                   [t.detach() for t in t_kd],
                                   [t.detach() for t in t_reg])
        return self._run_block(hp, targets, outs,
                               (t_kd, t_reg, teacher_x, *fourth), feats=x,
                               extra=extra)


@HEADS.register_module()
class LDHead(_FeatureLD, GFLHead):
    """ld_head.py:43-637."""
    _feat256_ref = 'ld_head.py:153-154'

    def _split_teacher(self, soft_teacher):
        soft_label, soft_target = soft_teacher
        return soft_label, soft_target

    def loss(self, cls_scores, bbox_preds, gt_bboxes, gt_labels, soft_teacher,
             x, teacher_x, img_metas, gt_bboxes_ignore=None):
        """ld_head.py:284-375."""
        return self._ld_loss((cls_scores, bbox_preds), gt_bboxes, gt_labels,
                             soft_teacher, x, teacher_x, img_metas)


class _SideLD:
    """LDATSSHead / LDFCOSHead / LDRetinaHead: LD on the positives weighted by
    the max class score, ``_vlr_k`` x LD on the head's second region and KD on
    the positives' class logits.  Their loss reads no features; the detector
    calls them with output_feature=False:
    forward_train(x, out_teacher, img_metas, ...)."""
    _vlr_k = None

    def __init__(self, num_classes, in_channels,
                 loss_ld=dict(type='LocalizationDistillationLoss',
                              loss_weight=0.25, T=10),
                 loss_kd=None, **kwargs):
        super().__init__(num_classes, in_channels, **kwargs)
        self.loss_ld = build_loss(loss_ld)
        self.loss_kd = build_loss(loss_kd)

    def forward_train(self, x, out_teacher, img_metas, gt_bboxes,
                      gt_labels=None, gt_bboxes_ignore=None, proposal_cfg=None,
                      **kwargs):
        return self._forward_train_ld(x, out_teacher, None, img_metas,
                                      gt_bboxes, gt_labels, gt_bboxes_ignore,
                                      proposal_cfg)

    def _ld_hp(self):
        """The reference's second term is _vlr_k * loss_ld(..., avg_factor=4);
        the block's VLR term is lw_ld_vlr * sum / 16."""
        return dict(lw_ld=self.loss_ld.loss_weight, T_ld=self.loss_ld.T,
                    lw_ld_vlr=self._vlr_k * 4.0 * self.loss_ld.loss_weight,
                    T_ld_vlr=self.loss_ld.T,
                    lw_kd=self.loss_kd.loss_weight, T_kd=self.loss_kd.T)


class _ATSSFamily:
    """What ATSSGFLHead and the plain ATSSHead share (atss_gfl_head.py:52-185,
    atss_head.py:15-143): GFLHead's two towers, ``atss_cls`` / ``atss_reg`` /
    ``atss_centerness`` output convs (state_dict names of the reference),
    FocalLoss + centerness-weighted box loss + centerness BCE.  forward
    returns (cls_scores, bbox_preds, centernesses); the box branch has
    ``_reg_out`` channels."""
    _predictors = ('atss_cls', 'atss_reg', 'atss_centerness')
    _loss_keys, _loss_rows = ATSS_LOSS_KEYS, _ATSS_ROWS
    _plain_keys = ('loss_cls', 'loss_bbox', 'loss_centerness')

    def _init_layers(self):
        """atss_gfl_head.py:90-125, atss_head.py:62-106."""
        self._build_towers()
        assert self.num_anchors == 1, 'one square anchor per position'
        self.atss_cls = Conv2d(self.feat_channels,
                               self.num_anchors * self.cls_out_channels, 3,
                               padding=1)
        self.atss_reg = Conv2d(self.feat_channels,
                               self.num_anchors * self._reg_out, 3, padding=1)
        self.atss_centerness = Conv2d(self.feat_channels, self.num_anchors, 3,
                                      padding=1)
        self._build_scales(self.anchor_generator.strides)

    def forward(self, feats):
        """atss_gfl_head.py:139-183, atss_head.py:108-143."""
        return self._predict(*self._trunk(feats))

    def _predict(self, cls_feat, reg_feat, levels):
        cls3, _ = self.atss_cls.forward3(cls_feat, levels)
        reg3, _ = self.atss_reg.forward3(reg_feat, levels)
        ctr3, _ = self.atss_centerness.forward3(reg_feat, levels)
        reg3 = self._scale(reg3, levels)
        return (Y.split_levels(cls3, levels), Y.split_levels(reg3, levels),
                Y.split_levels(ctr3, levels))

    def _check_loss_cfg(self):
        self._check_focal_cfg('ATSS', centerness=True)
        self._check_train_cfg()

    def _atss_hp(self):
        return dict(lw_dfl=0.0, lw_ctr=self.loss_centerness.loss_weight,
                    focal_alpha=self.loss_cls.alpha, qfl_beta=2.0,
                    flags=L.LD_LOSS_ATSS)

    def loss(self, cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels,
             img_metas, gt_bboxes_ignore=None):
        """atss_gfl_head.py:187-310, atss_head.py:221-296: loss_cls, loss_bbox,
        loss_centerness."""
        return self._loss((cls_scores, bbox_preds), gt_bboxes, gt_labels,
                          img_metas, extra=centernesses)

    def get_bboxes(self, cls_scores, bbox_preds, centernesses, img_metas,
                   cfg=None, rescale=False, with_nms=True):
        """atss_gfl_head.py:420-575, atss_head.py:376-508: GFLHead's pipeline
        with the top-k key max_c score_c * sigmoid(centerness) and the
        centerness as multiclass_nms' score factor (applied after the
        threshold test)."""
        return self._get_bboxes(cls_scores, bbox_preds, img_metas, cfg,
                                rescale, with_nms, prob=False,
                                centernesses=centernesses)


@HEADS.register_module()
class ATSSGFLHead(_ATSSFamily, GFLHead):
    """atss_gfl_head.py:52-185: the ATSS head with a general-distribution box
    branch."""

    def __init__(self, num_classes, in_channels, stacked_convs=4,
                 conv_cfg=None,
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True),
                 loss_centerness=dict(type='CrossEntropyLoss',
                                      use_sigmoid=True, loss_weight=1.0),
                 reg_max=16, **kwargs):
        kwargs.setdefault('loss_cls', dict(type='FocalLoss', use_sigmoid=True,
                                           gamma=2.0, alpha=0.25,
                                           loss_weight=1.0))
        kwargs.setdefault('bbox_coder', dict(
            type='DeltaXYWHBBoxCoder', target_means=(.0, .0, .0, .0),
            target_stds=(1.0, 1.0, 1.0, 1.0)))
        super().__init__(num_classes, in_channels, stacked_convs=stacked_convs,
                         conv_cfg=conv_cfg, norm_cfg=norm_cfg,
                         loss_dfl=dict(type='DistributionFocalLoss',
                                       loss_weight=0.0),
                         reg_max=reg_max, **kwargs)
        self.loss_centerness = build_loss(loss_centerness)

    def _hp(self, **over):
        kw = self._atss_hp()
        kw.update(over)
        return super()._hp(**kw)


@HEADS.register_module()
class LDATSSHead(_SideLD, ATSSGFLHead):
    """ld_atss.py:13-250: localization distillation on the ATSS-GFL head; the
    second region is the valuable localisation region."""
    # loss_ld_neg = 0.15 * loss_ld(..., avg_factor=4) (ld_atss.py:148-159)
    _vlr_k = 0.15

    def loss(self, cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels,
             soft_target, img_metas, gt_bboxes_ignore=None):
        """ld_atss.py:168-250 -> the six keys of ATSS_LOSS_KEYS."""
        return self._loss((cls_scores, bbox_preds), gt_bboxes, gt_labels,
                          img_metas, teacher=soft_target, extra=centernesses,
                          **self._ld_hp())


INF = 1e8


class _FCOSFamily:
    """What FCOSGFLHead and the plain FCOSHead share (fcos_gfl_head.py:52-346,
    fcos_head.py:15-154 over anchor_free_head.py:15-130): the anchor-free
    constructor, parameters ``cls_convs / reg_convs / conv_cls / conv_reg /
    conv_centerness / scales`` as in the reference, points (x, y) * stride +
    stride // 2 with the batched point targets, FocalLoss + centerness-weighted
    box loss + centerness BCE.  forward returns (cls_scores, bbox_preds,
    centernesses); the box branch has ``_reg_out`` channels."""
    _predictors = ('conv_cls', 'conv_reg', 'conv_centerness')
    _loss_keys, _loss_rows = ATSS_LOSS_KEYS, _ATSS_ROWS
    _plain_keys = ('loss_cls', 'loss_bbox', 'loss_centerness')
    # the targets of a captured step come from its StaticTargets
    _static_gt = False
    # ConvModule's bias argument of the tower layers
    _tower_bias = 'auto'

    def _init_fcos_head(self, num_classes, in_channels, feat_channels,
                        stacked_convs, strides, dcn_on_last_conv, conv_bias,
                        regress_ranges, center_sampling, center_sample_radius,
                        norm_on_bbox, centerness_on_reg, loss_cls, loss_bbox,
                        loss_centerness, conv_cfg, norm_cfg, train_cfg,
                        test_cfg):
        """AnchorFreeHead.__init__ (anchor_free_head.py:46-91) + the FCOS
        arguments; the caller runs ``_init_layers()``."""
        self.num_classes = self.cls_out_channels = num_classes
        self.in_channels, self.feat_channels = in_channels, feat_channels
        self.stacked_convs, self.strides = stacked_convs, list(strides)
        self.dcn_on_last_conv, self.conv_bias = dcn_on_last_conv, conv_bias
        self.regress_ranges = regress_ranges
        self.center_sampling = center_sampling
        self.center_sample_radius = center_sample_radius
        self.norm_on_bbox, self.centerness_on_reg = (norm_on_bbox,
                                                     centerness_on_reg)
        self.loss_cls = build_loss(loss_cls)
        self.loss_bbox = build_loss(loss_bbox)
        self.loss_centerness = build_loss(loss_centerness)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.conv_cfg, self.norm_cfg = conv_cfg, norm_cfg
        self.fp16_enabled = False
        self.unit_upstream = False

    def _init_layers(self):
        """fcos_gfl_head.py:134-165, fcos_head.py:93-97."""
        self._build_towers(self._tower_bias)
        self.conv_cls = Conv2d(self.feat_channels, self.cls_out_channels, 3,
                               padding=1)
        self.conv_reg = Conv2d(self.feat_channels, self._reg_out, 3,
                               padding=1)
        self.conv_centerness = Conv2d(self.feat_channels, 1, 3, padding=1)
        self._build_scales(self.strides)

    def forward(self, feats):
        """fcos_gfl_head.py:178-224, fcos_head.py:104-154."""
        return self._predict(*self._trunk(feats))

    def _ctr_feat(self, cls_feat, reg_feat):
        """The tower conv_centerness reads."""
        return reg_feat

    def _predict(self, cls_feat, reg_feat, levels):
        cls3, _ = self.conv_cls.forward3(cls_feat, levels)
        reg3, _ = self.conv_reg.forward3(reg_feat, levels)
        ctr3, _ = self.conv_centerness.forward3(
            self._ctr_feat(cls_feat, reg_feat), levels)
        reg3 = self._scale(reg3, levels)
        return (Y.split_levels(cls3, levels), Y.split_levels(reg3, levels),
                Y.split_levels(ctr3, levels))

    # ---------------------------------------------------------------- loss --
    def _check_loss_cfg(self):
        self._check_focal_cfg('FCOS', centerness=True)

    def _fcos_hp(self):
        return dict(lw_ctr=self.loss_centerness.loss_weight,
                    focal_alpha=self.loss_cls.alpha,
                    flags=L.LD_LOSS_ATSS | L.LD_LOSS_FCOS)

    def _hp(self, **over):
        kw = self._fcos_hp()
        kw.update(over)
        return super()._hp(**kw)

    def get_targets_batched(self, featmap_sizes, gt_bboxes, gt_labels, device,
                            img_metas=None):
        """get_points + get_targets (ld_fcos_head.py:261-414, fcos_head.py:
        468-588) for the whole batch in one launch."""
        return LB.fcos_targets(featmap_sizes, self.strides, gt_bboxes,
                               gt_labels, self.num_classes,
                               self.regress_ranges, self.center_sampling,
                               self.center_sample_radius, device,
                               img_metas=img_metas)

    def _targets(self, hp, cls_scores, img_metas, gt_bboxes, gt_labels):
        sizes = self._level_sizes(cls_scores, len(self.strides))
        return self.get_targets_batched(
            sizes, gt_bboxes, gt_labels, cls_scores[0].device,
            img_metas=img_metas if self._static_gt else None)

    def loss(self, cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels,
             img_metas, gt_bboxes_ignore=None):
        """fcos_gfl_head.py:276-345, fcos_head.py:157-254: loss_cls, loss_bbox,
        loss_centerness."""
        return self._loss((cls_scores, bbox_preds), gt_bboxes, gt_labels,
                          img_metas, extra=centernesses)

    def get_bboxes(self, cls_scores, bbox_preds, centernesses, img_metas,
                   cfg=None, rescale=False, with_nms=True):
        """fcos_gfl_head.py:347-546, fcos_head.py:257-454: as
        ATSSGFLHead.get_bboxes, decoded about the FCOS points (x, y) * stride +
        stride // 2."""
        return self._get_bboxes(cls_scores, bbox_preds, img_metas, cfg,
                                rescale, with_nms, prob=False,
                                centernesses=centernesses, points=True,
                                strides=self.strides)


@HEADS.register_module()
class FCOSGFLHead(_FCOSFamily, _DenseHead):
    """fcos_gfl_head.py:52-346 over anchor_free_head.py:15-130: the anchor-free
    FCOS head with a general-distribution box branch."""

    def __init__(self, num_classes, in_channels, feat_channels=256,
                 stacked_convs=4, strides=(4, 8, 16, 32, 64),
                 dcn_on_last_conv=False, conv_bias='auto',
                 regress_ranges=((-1, 64), (64, 128), (128, 256), (256, 512),
                                 (512, INF)),
                 center_sampling=False, center_sample_radius=1.5,
                 norm_on_bbox=False, centerness_on_reg=False,
                 loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0,
                               alpha=0.25, loss_weight=1.0),
                 loss_bbox=dict(type='IoULoss', loss_weight=1.0),
                 loss_centerness=dict(type='CrossEntropyLoss',
                                      use_sigmoid=True, loss_weight=1.0),
                 reg_max=16, conv_cfg=None,
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True),
                 train_cfg=None, test_cfg=None):
        super().__init__()
        if dcn_on_last_conv:
            raise NotImplementedError('dcn_on_last_conv')
        if norm_on_bbox:
            raise NotImplementedError('norm_on_bbox=True')
        self.reg_max = reg_max
        self._init_fcos_head(num_classes, in_channels, feat_channels,
                             stacked_convs, strides, dcn_on_last_conv,
                             conv_bias, regress_ranges, center_sampling,
                             center_sample_radius, norm_on_bbox,
                             centerness_on_reg, loss_cls, loss_bbox,
                             loss_centerness, conv_cfg, norm_cfg, train_cfg,
                             test_cfg)
        self._init_layers()
        # after the layers, like the reference (state_dict key order)
        self.integral = Integral(reg_max)


@HEADS.register_module()
class LDFCOSHead(_SideLD, FCOSGFLHead):
    """ld_fcos_head.py:13-445: localization distillation on the FCOS-GFL head;
    the second region is the "remain" points (inside a gt box, assigned to
    none), weighted by the student's max class score."""
    # loss_ld_neg = 0.25 * loss_ld(..., avg_factor=4) (ld_fcos_head.py:125-129)
    _vlr_k = 0.25

    def loss(self, cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels,
             out_teacher, img_metas, gt_bboxes_ignore=None):
        """ld_fcos_head.py:138-217 -> the six keys of ATSS_LOSS_KEYS."""
        return self._loss((cls_scores, bbox_preds), gt_bboxes, gt_labels,
                          img_metas, teacher=out_teacher, extra=centernesses,
                          **self._ld_hp())


class _RetinaFamily:
    """What RetinaGFLHead and the plain RetinaHead share (retina_gfl_head.py:
    50-330, retina_head.py:8-114 over anchor_head.py:14-173): ratios x scales
    anchors per cell, conv + ReLU towers, the two predictors named by
    ``_predictors``; forward returns (cls_scores (N, B * C, H, W), bbox_preds
    (N, B * _reg_out, H, W)) lists.

    Loss execution: the B anchors of a cell are B pseudo-images of the fused
    one-anchor-per-cell loss block (an (N, B * C, H, W) map IS the (N * B, C,
    H, W) map of them), targets come from ld_retina_targets."""
    _loss_keys, _loss_rows = RETINA_LOSS_KEYS, _RETINA_ROWS
    _plain_keys = ('loss_cls', 'loss_bbox')

    def _init_layers(self):
        """retina_gfl_head.py:231-264, retina_head.py:60-93 (no per-level
        Scale)."""
        self._build_towers()
        cls_name, reg_name = self._predictors
        setattr(self, cls_name, Conv2d(
            self.feat_channels, self.num_anchors * self.cls_out_channels, 3,
            padding=1))
        setattr(self, reg_name, Conv2d(
            self.feat_channels, self.num_anchors * self._reg_out, 3,
            padding=1))

    def forward(self, feats):
        """retina_gfl_head.py:276-299, retina_head.py:95-114."""
        return self._predict(*self._trunk(feats))

    def _predict(self, cls_feat, reg_feat, levels):
        cls_name, reg_name = self._predictors
        cls3, _ = getattr(self, cls_name).forward3(cls_feat, levels)
        reg3, _ = getattr(self, reg_name).forward3(reg_feat, levels)
        return Y.split_levels(cls3, levels), Y.split_levels(reg3, levels)

    # ---------------------------------------------------------------- loss --
    def _check_assigner(self):
        if type(self.assigner).__name__ != 'MaxIoUAssigner':
            raise NotImplementedError(
                f'{type(self.assigner).__name__}: the Retina targets kernel '
                'implements MaxIoUAssigner')

    def get_targets_batched(self, featmap_sizes, img_metas, gt_bboxes,
                            gt_labels, device, want_gt_inds=False):
        """get_anchors + get_targets (ld_retina.py:364-470) for the whole
        batch: three launches."""
        strides = [s[0] for s in self.anchor_generator.strides]
        if gt_labels is None:
            gt_labels = [b.new_zeros(b.shape[0], dtype=torch.long)
                         for b in gt_bboxes]
        anchors = [self.anchor_generator.grid_anchors_flat(featmap_sizes,
                                                           device)]
        return LB.retina_targets(featmap_sizes, strides, img_metas, gt_bboxes,
                                 gt_labels, anchors, self.num_anchors,
                                 self.assigner, self.num_classes, device,
                                 want_gt_inds=want_gt_inds)

    def _targets(self, hp, cls_scores, img_metas, gt_bboxes, gt_labels):
        sizes = self._level_sizes(cls_scores, self.anchor_generator.num_levels)
        return self.get_targets_batched(sizes, img_metas, gt_bboxes, gt_labels,
                                        cls_scores[0].device)

    def _pseudo(self, maps, channels):
        """(N, B * C, H, W) -> the (N * B, C, H, W) view of the same memory."""
        B = self.num_anchors
        return [t.view(t.shape[0] * B, channels, t.shape[2], t.shape[3])
                for t in maps]

    def _run_block(self, hp, targets, outs, teacher, **kw):
        """The block runs on the pseudo-image views.  num_total_samples is the
        LOCAL count (ld_retina.py:228-229, anchor_head.py:476-477): no
        cross-rank reduction of the normaliser."""
        C_, R4 = self.cls_out_channels, self._reg_out
        outs = self._pseudo(outs[0], C_), self._pseudo(outs[1], R4)
        teacher = (self._pseudo(teacher[0], C_), self._pseudo(teacher[1], R4),
                   None)
        return super()._run_block(hp, targets, outs, teacher,
                                  reduce_norm=False, **kw)

    def loss(self, cls_scores, bbox_preds, gt_bboxes, gt_labels, img_metas,
             gt_bboxes_ignore=None):
        """retina_gfl_head.py:157-229, anchor_head.py:427-495: loss_cls,
        loss_bbox."""
        return self._loss((cls_scores, bbox_preds), gt_bboxes, gt_labels,
                          img_metas)

    def get_bboxes(self, cls_scores, bbox_preds, img_metas, cfg=None,
                   rescale=False, with_nms=True):
        """anchor_head.py:497-727 + retina_gfl_head.py:301-412: sigmoid scores,
        per-level top-nms_pre over all (cell, base anchor) rows, decode,
        multiclass_nms."""
        return self._get_bboxes(cls_scores, bbox_preds, img_metas, cfg,
                                rescale, with_nms, prob=False,
                                num_base=self.num_anchors)


@HEADS.register_module()
class RetinaGFLHead(_RetinaFamily, _DenseHead):
    """retina_gfl_head.py:50-330: the RetinaNet head with a
    general-distribution box branch (``atss_cls`` / ``atss_reg`` predictor
    names as in the reference, Integral * stride decoded about the cell
    centre)."""
    _predictors = ('atss_cls', 'atss_reg')

    def __init__(self, num_classes, in_channels, stacked_convs=4,
                 conv_cfg=None, norm_cfg=None, reg_max=16, feat_channels=256,
                 anchor_generator=dict(type='AnchorGenerator',
                                       octave_base_scale=4,
                                       scales_per_octave=3,
                                       ratios=[0.5, 1.0, 2.0],
                                       strides=[8, 16, 32, 64, 128]),
                 bbox_coder=dict(type='DeltaXYWHBBoxCoder',
                                 target_means=(.0, .0, .0, .0),
                                 target_stds=(1.0, 1.0, 1.0, 1.0)),
                 reg_decoded_bbox=False,
                 loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True,
                               loss_weight=1.0),
                 loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0,
                                loss_weight=1.0),
                 train_cfg=None, test_cfg=None):
        super().__init__()
        self.reg_max = reg_max
        self._init_anchor_head(num_classes, in_channels, feat_channels,
                               stacked_convs, conv_cfg, norm_cfg,
                               anchor_generator, bbox_coder, reg_decoded_bbox,
                               loss_cls, loss_bbox, train_cfg, test_cfg)
        # after the layers, like the reference (state_dict key order)
        self.integral = Integral(self.reg_max)

    def _check_loss_cfg(self):
        if not self.reg_decoded_bbox:
            raise NotImplementedError(
                'the fused RetinaGFL loss block evaluates its box loss on '
                'decoded boxes (reg_decoded_bbox=True)')
        self._check_focal_cfg('RetinaGFL', centerness=False)
        self._check_train_cfg()
        self._check_assigner()

    def _hp(self, **over):
        kw = dict(focal_alpha=self.loss_cls.alpha, flags=L.LD_LOSS_RETINA)
        kw.update(over)
        return super()._hp(**kw)


@HEADS.register_module()
class LDRetinaHead(_SideLD, RetinaGFLHead):
    """ld_retina.py:13-636: localization distillation on the RetinaGFL head,
    LD over the 68 corner logits of every positive anchor; the second region
    is the valuable localisation region of the background anchors."""
    # loss_ld_vlr = 0.03 * loss_ld(..., avg_factor=4) (ld_retina.py:109-110)
    _vlr_k = 0.03

    def loss(self, cls_scores, bbox_preds, gt_bboxes, gt_labels, out_teacher,
             img_metas, gt_bboxes_ignore=None):
        """ld_retina.py:187-254 -> the five keys of RETINA_LOSS_KEYS."""
        return self._loss((cls_scores, bbox_preds), gt_bboxes, gt_labels,
                          img_metas, teacher=out_teacher, **self._ld_hp())


class _Marker(nn.Module):
    """Parameter-free placeholder that keeps nn.Sequential's indices (and with
    them the state_dict keys ``reg_conf.0.*`` / ``reg_conf.2.*``) identical to
    the reference's [Conv2d, ReLU, Conv2d, Sigmoid]; the arithmetic of all four
    stages is the fused quality kernel."""

    def __init__(self, what):
        super().__init__()
        self.what = what

    def extra_repr(self):
        return self.what


@HEADS.register_module()
class GFocalHead(GFLHead):
    """GFLv2 head (gfocal_head.py:14-217): GFLHead's towers + the
    distribution-guided quality estimator ``reg_conf``; cls_out_channels is
    num_classes + 1 because its QFL runs with use_sigmoid=False
    (anchor_head.py:68-71).  forward returns (cls_scores, bbox_preds,
    cls_feats) like the reference."""

    def __init__(self, num_classes, in_channels, stacked_convs=4,
                 conv_cfg=None,
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True),
                 loss_dfl=dict(type='DistributionFocalLoss', loss_weight=0.25),
                 reg_max=16, reg_topk=4, reg_channels=64, add_mean=True,
                 **kwargs):
        if (reg_topk, reg_channels, bool(add_mean), reg_max) != (4, 64, True,
                                                                 16):
            raise NotImplementedError(
                'GFocalHead: the fused quality kernel is compiled for '
                'reg_topk=4, reg_channels=64, add_mean=True, reg_max=16 '
                '(the values of configs/gfl/gflv2_*.py and configs/ldv2)')
        self.reg_topk, self.reg_channels, self.add_mean = (reg_topk,
                                                           reg_channels,
                                                           add_mean)
        self.total_dim = reg_topk + (1 if add_mean else 0)
        super().__init__(num_classes, in_channels, stacked_convs=stacked_convs,
                         conv_cfg=conv_cfg, norm_cfg=norm_cfg,
                         loss_dfl=loss_dfl, reg_max=reg_max, **kwargs)

    def _init_layers(self):
        """gfocal_head.py:102-144."""
        super()._init_layers()
        self.reg_conf = nn.Sequential(
            Conv2d(4 * self.total_dim, self.reg_channels, 1), _Marker('ReLU'),
            Conv2d(self.reg_channels, 1, 1), _Marker('Sigmoid'))

    def init_weights(self):
        """gfocal_head.py:146-158."""
        super().init_weights()
        for m in self.reg_conf:
            if isinstance(m, Conv2d):
                normal_init(m, std=0.01)

    def forward(self, feats):
        """gfocal_head.py:160-217: GFLHead's forward, then the fused quality
        kernel."""
        return self._predict(*self._trunk(feats))

    def _predict(self, cls_feat, reg_feat, levels):
        cls3, _ = self.gfl_cls.forward3(cls_feat, levels)
        reg3, _ = self.gfl_reg.forward3(reg_feat, levels)
        reg3 = self._scale(reg3, levels)
        c0, c2 = self.reg_conf[0], self.reg_conf[2]
        score3, _ = Y.QualityFn.apply(reg3, cls3, c0.weight, c0.bias,
                                      c2.weight, c2.bias)
        return (Y.split_levels(score3, levels), Y.split_levels(reg3, levels),
                Y.split_levels(cls3, levels))

    def _hp(self, **over):
        kw = dict(cls_channels=self.cls_out_channels,
                  flags=L.LD_LOSS_PROB_CLS)
        kw.update(over)
        return super()._hp(**kw)

    def _check_loss_cfg(self):
        super()._check_loss_cfg()
        if getattr(self.loss_cls, 'use_sigmoid', True):
            raise NotImplementedError(
                'GFocalHead multiplies sigmoid(cls_feat) by the quality score '
                'itself: its QualityFocalLoss must have use_sigmoid=False '
                '(configs/gfl/gflv2_*.py)')

    def loss(self, cls_scores, bbox_preds, cls_feat, gt_bboxes, gt_labels,
             img_metas, gt_bboxes_ignore=None):
        """gfocal_head.py:230-352 (plain GFLv2: QFL on probabilities + GIoU +
        DFL); the KD term of the fused block reads cls_feat, so the student's
        own detached cls_feat is its KD teacher and stands in for the
        features."""
        self._check_loss_cfg()
        hp = self._hp()
        targets = self._targets(hp, cls_scores, img_metas, gt_bboxes,
                                gt_labels)
        det = [c.detach() for c in cls_feat]
        hp.feat_channels = det[0].shape[1]
        return self._run_block(hp, targets, (cls_scores, bbox_preds),
                               (det, bbox_preds, det, det), feats=det,
                               extra=cls_feat, want=self._plain_keys)

    def get_bboxes(self, cls_scores, bbox_preds, cls_feat, img_metas, cfg=None,
                   rescale=False, with_nms=True):
        """gfocal_head.py:317-596: GFLHead's pipeline on the head's own
        probabilities (cls_score = sigmoid(cls) * quality, no second sigmoid)
        over all cls_out_channels = num_classes + 1 score channels -- the
        reference's background column is an ordinary class here, label 80
        included.  ``cls_feat`` (the third head output) is unused, as in the
        reference."""
        return self._get_bboxes(cls_scores, bbox_preds, img_metas, cfg,
                                rescale, with_nms, prob=True)


@HEADS.register_module()
class LDv2Head(_FeatureLD, GFocalHead):
    """ld_gflv2.py:44-644: LDHead's distillation terms on a GFocalHead.
    Differences from LDHead that the fused block is told through its hp flags
    (ld_gflv2.py:200,243,326): weight_targets = max_c cls_score with no
    sigmoid, QFL on probabilities over 81 channels, KD on the raw cls_feat of
    student and teacher (``soft_teacher`` = (cls_score, bbox_pred, cls_feat),
    of which the first is ignored)."""
    _feat256_ref = 'ld_gflv2.py:155-156'

    def _split_teacher(self, soft_teacher):
        _, soft_target, soft_label = soft_teacher  # ld_gflv2.py:326
        return soft_label, soft_target, soft_label

    def loss(self, cls_scores, bbox_preds, cls_feat, gt_bboxes, gt_labels,
             soft_teacher, x, teacher_x, img_metas, gt_bboxes_ignore=None):
        """ld_gflv2.py:286-380."""
        return self._ld_loss((cls_scores, bbox_preds), gt_bboxes, gt_labels,
                             soft_teacher, x, teacher_x, img_metas,
                             extra=cls_feat)
