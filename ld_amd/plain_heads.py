"""The plain ATSS, RetinaNet and FCOS heads with mmdet's constructor
arguments, state_dict keys and method signatures (reference:
mmdet/models/dense_heads/atss_head.py:15-508, retina_head.py:8-114,
anchor_head.py:14-727, fcos_head.py:15-608 over anchor_free_head.py): the
baselines the general-distribution and LD heads
of ``heads.py`` are measured against.

They are ``heads._DenseHead`` heads -- towers, packed forward trunk, the ONE
loss-block call, loss dict, forward_train, get_bboxes, aug_test -- and share
``_ATSSFamily`` / ``_RetinaFamily`` with ATSSGFLHead / RetinaGFLHead; what
differs is the box branch, stated once in ``_DeltaBox``: 4 DeltaXYWH deltas per
anchor, taken by the fused loss block with LD_LOSS_DELTA and by get_bboxes with
LD_INFER_DELTA (csrc/loss.hip, csrc/infer.hip).  FCOSHead shares
``_FCOSFamily`` with FCOSGFLHead; its box branch is ``_DistBox``: 4 activated
distances per point, LD_LOSS_DIST / LD_INFER_DIST."""
import torch

from . import layers as Y
from . import lib as L
from .heads import (INF, _BOX_LOSSES, _ATSSFamily, _DenseHead, _FCOSFamily,
                    _RetinaFamily)
from .losses import bbox_loss_mode
from .registry import HEADS, build_loss


class _DeltaBox:
    """The box branch of the plain heads: 4 DeltaXYWH deltas per anchor
    (``bbox_coder``) instead of a distribution.  The fused loss block takes
    them with LD_LOSS_DELTA -- its positives launch decodes about the anchor,
    evaluates the box loss and differentiates through the decode --, and
    get_bboxes with LD_INFER_DELTA.  No Integral, no teacher terms."""
    _reg_out = 4
    # the anchors the kernels decode about: the implicit square of the
    # single-anchor generators, or the generator's explicit list
    _explicit_anchors = False

    def _box_term(self):
        return dict(box_term='decoded')

    def _delta(self, cls_scores):
        """(ld_delta_t, explicit anchors or None) for these level maps."""
        if type(self.bbox_coder).__name__ != 'DeltaXYWHBBoxCoder':
            raise NotImplementedError(
                f'{type(self).__name__}: bbox_coder '
                f'{type(self.bbox_coder).__name__} (DeltaXYWHBBoxCoder)')
        anchors = None
        if self._explicit_anchors:
            sizes = self._level_sizes(cls_scores,
                                      self.anchor_generator.num_levels)
            anchors = self.anchor_generator.grid_anchors_flat(
                sizes, cls_scores[0].device)
        return (self.bbox_coder.delta_t(
            num_base=self.num_anchors if self._explicit_anchors else 0,
            **self._box_term()), anchors)

    def _targets(self, hp, cls_scores, img_metas, gt_bboxes, gt_labels):
        targets = super()._targets(hp, cls_scores, img_metas, gt_bboxes,
                                   gt_labels)
        targets['delta'] = self._delta(cls_scores)
        return targets

    def _get_bboxes(self, *args, **kwargs):
        return super()._get_bboxes(*args, delta=self._delta, **kwargs)


@HEADS.register_module()
class ATSSHead(_DeltaBox, _ATSSFamily, _DenseHead):
    """atss_head.py:15-143 over anchor_head.py:14-173: the plain ATSS head,
    ``atss_reg`` predicts the 4 deltas of the one square anchor of a cell.
    Loss (atss_head.py:145-296): FocalLoss, the box loss on the decoded
    prediction against the encoded-then-decoded GT weighted by the centerness
    target, centerness BCE."""

    def __init__(self, num_classes, in_channels, stacked_convs=4,
                 conv_cfg=None,
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True),
                 loss_centerness=dict(type='CrossEntropyLoss',
                                      use_sigmoid=True, loss_weight=1.0),
                 feat_channels=256,
                 anchor_generator=dict(type='AnchorGenerator',
                                       scales=[8, 16, 32],
                                       ratios=[0.5, 1.0, 2.0],
                                       strides=[4, 8, 16, 32, 64]),
                 bbox_coder=dict(type='DeltaXYWHBBoxCoder', clip_border=True,
                                 target_means=(.0, .0, .0, .0),
                                 target_stds=(1.0, 1.0, 1.0, 1.0)),
                 reg_decoded_bbox=False,
                 loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True,
                               loss_weight=1.0),
                 loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0,
                                loss_weight=1.0),
                 train_cfg=None, test_cfg=None):
        super().__init__()
        self._init_anchor_head(num_classes, in_channels, feat_channels,
                               stacked_convs, conv_cfg, norm_cfg,
                               anchor_generator, bbox_coder, reg_decoded_bbox,
                               loss_cls, loss_bbox, train_cfg, test_cfg)
        self.sampling = False  # atss_head.py:58
        self.loss_centerness = build_loss(loss_centerness)

    def _hp(self, **over):
        kw = self._atss_hp()
        kw.update(topk=self.assigner.topk,
                  flags=L.LD_LOSS_ATSS | L.LD_LOSS_DELTA)
        kw.update(over)
        return super()._hp(**kw)


@HEADS.register_module()
class RetinaHead(_DeltaBox, _RetinaFamily, _DenseHead):
    """retina_head.py:8-114 over anchor_head.py:14-173: the plain RetinaNet
    head, ``retina_cls`` / ``retina_reg`` with 4 deltas per anchor.  Loss
    (anchor_head.py:376-495): FocalLoss with label_weights; L1Loss /
    SmoothL1Loss on pred - bbox2delta(anchor, gt), or with
    reg_decoded_bbox=True a box loss on the decoded prediction; both divided by
    the local num_total_pos."""
    _predictors = ('retina_cls', 'retina_reg')
    _explicit_anchors = True

    def __init__(self, num_classes, in_channels, stacked_convs=4,
                 conv_cfg=None, norm_cfg=None,
                 anchor_generator=dict(type='AnchorGenerator',
                                       octave_base_scale=4,
                                       scales_per_octave=3,
                                       ratios=[0.5, 1.0, 2.0],
                                       strides=[8, 16, 32, 64, 128]),
                 feat_channels=256,
                 bbox_coder=dict(type='DeltaXYWHBBoxCoder', clip_border=True,
                                 target_means=(.0, .0, .0, .0),
                                 target_stds=(1.0, 1.0, 1.0, 1.0)),
                 reg_decoded_bbox=False,
                 loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True,
                               loss_weight=1.0),
                 loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0,
                                loss_weight=1.0),
                 train_cfg=None, test_cfg=None):
        super().__init__()
        self._init_anchor_head(num_classes, in_channels, feat_channels,
                               stacked_convs, conv_cfg, norm_cfg,
                               anchor_generator, bbox_coder, reg_decoded_bbox,
                               loss_cls, loss_bbox, train_cfg, test_cfg)

    def _box_term(self):
        from .losses import L1Loss, SmoothL1Loss
        if self.reg_decoded_bbox:
            return dict(box_term='decoded')
        if isinstance(self.loss_bbox, SmoothL1Loss):
            return dict(box_term='smooth_l1', beta=self.loss_bbox.beta)
        if isinstance(self.loss_bbox, L1Loss):
            return dict(box_term='l1')
        raise NotImplementedError(
            f'RetinaHead: loss_bbox {type(self.loss_bbox).__name__} on the '
            'deltas (reg_decoded_bbox=False takes L1Loss or SmoothL1Loss)')

    def _check_loss_cfg(self):
        from .losses import FocalLoss
        if self.sampling or not isinstance(self.loss_cls, FocalLoss):
            raise NotImplementedError(
                f'RetinaHead: a sampling loss_cls '
                f'({type(self.loss_cls).__name__}) needs a sampler; the fused '
                'loss block implements FocalLoss on every anchor')
        if self.loss_cls.gamma != 2.0:
            raise NotImplementedError('FocalLoss gamma != 2')
        if self.reg_decoded_bbox and bbox_loss_mode(self.loss_bbox) is None:
            raise NotImplementedError(
                f'RetinaHead: reg_decoded_bbox=True takes {_BOX_LOSSES} (got '
                f'{type(self.loss_bbox).__name__})')
        self._box_term()
        self._check_train_cfg()
        self._check_assigner()

    def _hp(self, **over):
        kw = dict(focal_alpha=self.loss_cls.alpha,
                  flags=L.LD_LOSS_RETINA | L.LD_LOSS_DELTA)
        kw.update(over)
        return super()._hp(**kw)


class _DistBox:
    """The box branch of the plain FCOS head: 4 distances (l, t, r, b) per
    point, ``exp(scale_l * x)`` or, with ``norm_on_bbox``, ``relu(scale_l *
    x)`` in stride units while training and times the stride in eval mode
    (fcos_head.py:145-153) -- Scale and activation in one launch
    (layers.scale_act_levels), so ``forward`` returns the activated maps.  The
    fused loss block takes them with LD_LOSS_DIST, get_bboxes with
    LD_INFER_DIST.  No Integral, no teacher terms."""
    _reg_out = 4

    def _scale(self, reg3, levels):
        mode = 'exp' if not self.norm_on_bbox else \
            'relu' if self.training else 'relu_stride'
        return Y.scale_act_levels(
            reg3, torch.stack([s.scale for s in self.scales]), levels, mode,
            self.strides)

    def _get_bboxes(self, *args, **kwargs):
        return super()._get_bboxes(*args, dist=True, **kwargs)


@HEADS.register_module()
class FCOSHead(_DistBox, _FCOSFamily, _DenseHead):
    """fcos_head.py:15-154 over anchor_free_head.py:15-130: the plain FCOS
    head.  Loss (fcos_head.py:157-254): FocalLoss / max(num_pos, 1), the box
    loss on distance2bbox(point, pred) against distance2bbox(point, target)
    weighted by the centerness target / max(sum of the targets, 1e-6),
    centerness BCE / max(num_pos, 1).  ``conv_centerness`` reads the class
    tower unless ``centerness_on_reg``."""
    _static_gt = True

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
                 conv_cfg=None,
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True),
                 train_cfg=None, test_cfg=None):
        super().__init__()
        if dcn_on_last_conv:
            raise NotImplementedError('FCOSHead: dcn_on_last_conv')
        if loss_cls.get('type') != 'FocalLoss' or \
                loss_cls.get('gamma', 2.0) != 2.0:
            raise NotImplementedError(
                f'FCOSHead: loss_cls {loss_cls.get("type")} (gamma '
                f'{loss_cls.get("gamma", 2.0)}); the fused loss block '
                'implements FocalLoss with gamma 2')
        self._init_fcos_head(num_classes, in_channels, feat_channels,
                             stacked_convs, strides, dcn_on_last_conv,
                             conv_bias, regress_ranges, center_sampling,
                             center_sample_radius, norm_on_bbox,
                             centerness_on_reg, loss_cls, loss_bbox,
                             loss_centerness, conv_cfg, norm_cfg, train_cfg,
                             test_cfg)
        self._init_layers()

    @property
    def _tower_bias(self):
        return self.conv_bias

    def _ctr_feat(self, cls_feat, reg_feat):
        return reg_feat if self.centerness_on_reg else cls_feat

    def _fcos_hp(self):
        kw = super()._fcos_hp()
        kw['flags'] |= L.LD_LOSS_DIST | \
            (L.LD_LOSS_DIST_NORM if self.norm_on_bbox else 0)
        return kw
