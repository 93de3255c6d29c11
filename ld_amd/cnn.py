"""Building blocks with mmcv.cnn's names and state_dict keys (ConvModule,
Scale, build_conv_layer, build_norm_layer, init helpers), implemented over the
HIP layer functions in ld_amd.layers.  Parameter shapes and key names match
mmdet/mmcv so released checkpoints map 1:1 (SURVEY.md section 5 "checkpoint").

Modules take and return ordinary (N, C, H, W) tensors; the level-concatenated
fast path of the head lives in ld_amd.heads.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import layers as Y


# ------------------------------------------------------------------ inits --
def constant_init(module, val, bias=0):
    if getattr(module, 'weight', None) is not None:
        nn.init.constant_(module.weight, val)
    if getattr(module, 'bias', None) is not None:
        nn.init.constant_(module.bias, bias)


def normal_init(module, mean=0, std=1, bias=0):
    if getattr(module, 'weight', None) is not None:
        nn.init.normal_(module.weight, mean, std)
    if getattr(module, 'bias', None) is not None:
        nn.init.constant_(module.bias, bias)


def xavier_init(module, gain=1, bias=0, distribution='normal'):
    assert distribution in ['uniform', 'normal']
    if getattr(module, 'weight', None) is not None:
        if distribution == 'uniform':
            nn.init.xavier_uniform_(module.weight, gain=gain)
        else:
            nn.init.xavier_normal_(module.weight, gain=gain)
    if getattr(module, 'bias', None) is not None:
        nn.init.constant_(module.bias, bias)


def kaiming_init(module, a=0, mode='fan_out', nonlinearity='relu', bias=0,
                 distribution='normal'):
    assert distribution in ['uniform', 'normal']
    if getattr(module, 'weight', None) is not None:
        if distribution == 'uniform':
            nn.init.kaiming_uniform_(module.weight, a=a, mode=mode,
                                     nonlinearity=nonlinearity)
        else:
            nn.init.kaiming_normal_(module.weight, a=a, mode=mode,
                                    nonlinearity=nonlinearity)
    if getattr(module, 'bias', None) is not None:
        nn.init.constant_(module.bias, bias)


def bias_init_with_prob(prior_prob):
    return float(-np.log((1 - prior_prob) / prior_prob))


# ---------------------------------------------------------------- layers ---
def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


class Conv2d(nn.Module):
    """nn.Conv2d's parameters and keys; forward = MFMA implicit GEMM."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1,
                 padding=0, dilation=1, groups=1, bias=True):
        super().__init__()
        k, s, p, d = (_pair(kernel_size), _pair(stride), _pair(padding),
                      _pair(dilation))
        if k[0] != k[1] or s[0] != s[1] or p[0] != p[1]:
            raise NotImplementedError('only square kernels/strides/pads')
        if d != (1, 1) or groups != 1:
            raise NotImplementedError(
                'dilated / grouped convs are not on the LD hot path')
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = k, s, p
        self.weight = nn.Parameter(
            torch.empty(out_channels, in_channels, k[0], k[1]))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            fan_in = self.in_channels * self.kernel_size[0] * self.kernel_size[1]
            bound = 1 / math.sqrt(fan_in)
            nn.init.uniform_(self.bias, -bound, bound)

    def forward3(self, x3, levels):
        """(N, C, P) level-concatenated in/out."""
        return Y.conv2d(x3, self.weight, self.bias, self.stride[0],
                        self.padding[0], levels)

    def forward(self, x):
        n, c, h, w = x.shape
        y3, lv = self.forward3(x.reshape(n, c, h * w), ((h, w), ))
        return y3.view(n, self.out_channels, lv[0][0], lv[0][1])

    def extra_repr(self):
        return (f'{self.in_channels}, {self.out_channels}, '
                f'kernel_size={self.kernel_size}, stride={self.stride}, '
                f'padding={self.padding}, bias={self.bias is not None}')


class GroupedConv2d(nn.Module):
    """nn.Conv2d(..., groups=G > 1)'s parameters and keys: ``weight`` (Cout,
    Cin / G, k, k) -- the 3x3 conv2 of every ResNeXt Bottleneck
    (resnext.py:49-61, groups = 32 / 64).

    Frozen or under ``torch.no_grad()`` (the X-101 teacher of BASELINE config
    5): ld_gconv_forward with the following eval-mode BN and ReLU folded into
    its epilogue (``forward3_fused``, the hook resnet._conv_bn takes for
    forward-only convs).

    Trainable (``forward3`` / ``forward3_bn`` with autograd on and an input or
    weight that needs a gradient; configs/gfl/gfl_x101_*): layers.gconv2d
    (GroupedConvFn: ld_gconv_dgrad / ld_gconv_wgrad) followed by the eval-mode
    BN as its own autograd node.  fp32 only, and the input must exist in fp32."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1,
                 padding=0, dilation=1, groups=1, bias=False):
        super().__init__()
        k, s, p, d = (_pair(kernel_size), _pair(stride), _pair(padding),
                      _pair(dilation))
        if k[0] != k[1] or s[0] != s[1] or p[0] != p[1]:
            raise NotImplementedError('only square kernels/strides/pads')
        if d != (1, 1) or bias:
            raise NotImplementedError('grouped conv: no dilation, no bias '
                                      '(resnext.py:49-61)')
        if in_channels % groups or out_channels % groups or \
                out_channels // groups not in (4, 8, 16, 32) or \
                k[0] not in (1, 3):
            raise NotImplementedError(
                f'grouped conv {in_channels}->{out_channels} / {groups} k{k[0]}: '
                'built for 4 / 8 / 16 / 32 output channels per group, k 1 or 3')
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = k, s, p
        self.groups = groups
        self.weight = nn.Parameter(
            torch.empty(out_channels, in_channels // groups, k[0], k[1]))
        self.bias = None
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))

    def needs_grad(self, x3):
        return torch.is_grad_enabled() and (
            (isinstance(x3, torch.Tensor) and x3.requires_grad) or
            self.weight.requires_grad)

    def forward3_bn(self, x3, levels, bn=None, residual=None, relu=False):
        """The trainable path: relu?(BN_eval(gconv(x)) + residual), or the plain
        grouped conv with ``bn`` None."""
        y3, out_levels = Y.gconv2d(x3, self.weight, self.groups,
                                   self.stride[0], self.padding[0], levels)
        if bn is None:
            if residual is not None or relu:
                raise NotImplementedError(
                    'grouped conv epilogue without a norm layer')
            return y3, out_levels
        return bn.forward3(y3, residual, relu), out_levels

    def forward3_fused(self, x3, levels, scale=None, shift=None, residual=None,
                       relu=False):
        if self.needs_grad(x3):
            raise NotImplementedError(
                'GroupedConv2d.forward3_fused (the folded-epilogue hook) is '
                'inference-only: the trainable entry points are forward3 / '
                'forward3_bn (resnet._conv_bn takes the latter)')
        if residual is not None:
            raise NotImplementedError('grouped conv with a fused residual')
        return Y.gconv_forward(x3, self.weight, self.groups, self.stride[0],
                               self.padding[0], levels, scale, shift, relu)

    def forward3(self, x3, levels):
        if self.needs_grad(x3):
            return self.forward3_bn(x3, levels)
        return self.forward3_fused(x3, levels)

    def forward(self, x):
        n, c, h, w = x.shape
        y3, lv = self.forward3(x.reshape(n, c, h * w), ((h, w), ))
        return y3.view(n, self.out_channels, lv[0][0], lv[0][1])

    def extra_repr(self):
        return (f'{self.in_channels}, {self.out_channels}, '
                f'kernel_size={self.kernel_size}, stride={self.stride}, '
                f'padding={self.padding}, groups={self.groups}, bias=False')


class _DeformConvPack(nn.Module):
    """What DeformConv2dPack (DCNv1) and ModulatedDeformConv2dPack (DCNv2)
    share: the parameters, the cached (Cout, Cin*k*k, 1, 1) weight views and
    the three paths (frozen, trainable plain / conv + eval-BN pair, trainable
    grouped as conv + BN pair).  A subclass names itself (``_NAME``, used in
    every refusal), says how many ``conv_offset`` channels a tap takes
    (``_TAP_CHANNELS``), checks its own constructor arguments
    (``_check_args``) and supplies the sampling (``_sample`` without autograd,
    ``_sample_fn`` differentiable)."""

    _NAME = 'DCN'
    _TAP_CHANNELS = 2
    _NOT_SQUARE = 'only square kernels/strides/pads'

    def __init__(self, in_channels, out_channels, kernel_size, stride=1,
                 padding=0, dilation=1, groups=1, deform_groups=1, bias=False,
                 **kwargs):
        super().__init__()
        k, s, p, d = (_pair(kernel_size), _pair(stride), _pair(padding),
                      _pair(dilation))
        if k[0] != k[1] or s[0] != s[1] or p[0] != p[1] or d[0] != d[1]:
            raise NotImplementedError(self._NOT_SQUARE)
        self._check_args(deform_groups, bias, groups)
        if groups != 1 and (in_channels % groups or out_channels % groups or
                            out_channels // groups not in (4, 8, 16, 32)):
            raise NotImplementedError(
                f'grouped {self._NAME} {in_channels}->{out_channels} / '
                f'{groups}')
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding, self.dilation = k, s, p, d
        self.groups, self.deform_groups = groups, deform_groups
        self.weight = nn.Parameter(
            torch.empty(out_channels, in_channels // groups, k[0], k[1]))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.conv_offset = Conv2d(
            in_channels, deform_groups * self._TAP_CHANNELS * k[0] * k[1],
            k[0], stride=s[0], padding=p[0], bias=True)
        if d != (1, 1):
            raise NotImplementedError(f'dilated {self._NAME}')
        self.reset_parameters()
        self._w2d = None
        self._w2d_train = None

    def reset_parameters(self):
        # mmcv: uniform(-stdv, stdv), stdv = 1/sqrt(Cin*k*k); offsets start at 0
        n = self.in_channels * self.kernel_size[0] * self.kernel_size[1]
        stdv = 1.0 / math.sqrt(n)
        nn.init.uniform_(self.weight, -stdv, stdv)
        if self.bias is not None:
            nn.init.zeros_(self.bias)
        nn.init.zeros_(self.conv_offset.weight)
        nn.init.zeros_(self.conv_offset.bias)

    def _weight_2d(self):
        """(Cout, Cin*k*k, 1, 1) view of the weight, kept alive so the GEMM
        weight image cached on it survives between calls."""
        w, v = self.weight, self._w2d
        if v is None or v.data_ptr() != w.data_ptr() or v.device != w.device \
                or v._version != w._version:
            v = w.detach().view(self.out_channels, -1, 1, 1)
            v._ld_static = getattr(w, '_ld_static', False) or \
                not w.requires_grad
            self._w2d = v
        return v

    def _weight_2d_train(self):
        """The (Cout, Cin*k*k, 1, 1) weight of the differentiable 1x1 conv.  With
        a gradient arena (train.GradArena gave the parameter ``_ld_grad``) a
        persistent leaf view that carries the matching view of the arena slice
        and forwards the ready callback to the parameter: the wgrad kernel then
        accumulates straight into the arena, and the GEMM images cached on the
        view are refreshed with every other trainable weight.  Without an
        arena an autograd view, whose gradient flows back to ``weight.grad``."""
        w = self.weight
        if not w.requires_grad:
            return self._weight_2d()
        sink = getattr(w, '_ld_grad', None) if Y.DIRECT_GRADS[0] else None
        if sink is None:
            v = w.view(self.out_channels, -1, 1, 1)
            v._ld_static = True  # a fresh tensor per call: nothing to refresh
            return v
        v = self._w2d_train
        if v is None or v.data_ptr() != w.data_ptr() or \
                v.device != w.device or \
                v._ld_grad.data_ptr() != sink.data_ptr():
            v = w.detach().view(self.out_channels, -1, 1, 1).requires_grad_(True)
            v._ld_grad = sink.view(v.shape)
            v._ld_pending = 0
            self._w2d_train = v
        v._ld_ready = lambda _v, w=w: w._ld_ready(w)
        return v

    def needs_grad(self, x3):
        return torch.is_grad_enabled() and (
            (isinstance(x3, torch.Tensor) and x3.requires_grad) or
            any(p.requires_grad for p in self.parameters()))

    def forward3_bn(self, x3, levels, bn=None, residual=None, relu=False):
        """The trainable path: relu?(BN_eval(dcn(x)) + residual), or the plain
        deformable conv with ``bn`` None.  Every piece is an autograd node."""
        name = self._NAME
        if self.groups != 1 and bn is None:
            raise NotImplementedError(
                f'grouped {name} trains as the conv + BN pair of a ResNeXt '
                'Bottleneck only (forward3_bn with its norm layer)')
        if self.groups != 1 and Y.get_precision() == 'bf16':
            raise NotImplementedError(
                f'trainable grouped {name} is fp32 only (bf16 mode is not '
                'built)')
        if self.deform_groups != 1 or self.dilation != (1, 1):
            raise NotImplementedError(
                f'trainable {name}: deform_groups = 1 and no dilation are '
                'built')
        if self.bias is not None and bn is not None:
            raise NotImplementedError(
                f'{name} with a bias followed by a folded norm layer (bn)')
        Y._fp32_readable(x3, f'trainable {name} input')
        if len(levels) != 1:
            raise NotImplementedError(
                f'{name} on level-concatenated tensors')
        if self.groups == 1 and bn is None and (residual is not None or relu):
            raise NotImplementedError(f'{name} epilogue without a norm layer')
        (h, w), = levels
        k, s, p = self.kernel_size[0], self.stride[0], self.padding[0]
        co = self.conv_offset
        off3, out_levels = Y.conv2d(x3, co.weight, co.bias, s, p, levels)
        col = self._sample_fn(x3, off3, h, w, k, s, p)
        w2 = self._weight_2d_train()
        if self.groups != 1:
            # grouped DCN (resnext.py:62-74): rows [g * cg * k * k, (g + 1) * cg
            # * k * k) of the column tensor feed group g -- the differentiable
            # grouped 1x1 conv over Cin * k * k channels, then the BN node
            y3, _ = Y.gconv2d(col, w2, self.groups, 1, 0, out_levels)
            return bn.forward3(y3, residual, relu), out_levels
        if bn is None:
            return Y.conv2d(col, w2, self.bias, 1, 0, out_levels)
        return Y.conv_bn_act(col, w2, bn.weight, bn.bias, bn.running_mean,
                             bn.running_var, bn.eps, 1, 0, out_levels, residual,
                             relu)

    def forward3_fused(self, x3, levels, scale=None, shift=None, residual=None,
                       relu=False):
        """offset conv -> deformable im2col -> 1x1 GEMM with the fused epilogue
        (BN affine / residual / ReLU); inference only when an epilogue is
        given (the trainable conv + BN pair is ``forward3_bn``)."""
        if self.needs_grad(x3):
            if scale is not None or shift is not None or \
                    residual is not None or relu:
                raise NotImplementedError(
                    f'{type(self).__name__}.forward3_fused with a folded '
                    'epilogue is inference-only: the trainable conv + BN pair '
                    'is forward3_bn (resnet._conv_bn takes it)')
            return self.forward3_bn(x3, levels)
        if len(levels) != 1:
            raise NotImplementedError(
                f'{self._NAME} on level-concatenated tensors')
        if self.bias is not None and (scale is not None or shift is not None):
            raise NotImplementedError(
                f'{self._NAME} with a bias and a folded norm layer (scale / '
                'shift)')
        if self.groups != 1 and residual is not None:
            raise NotImplementedError(
                f'grouped {self._NAME} with a fused residual')
        (h, w), = levels
        N, cin, P = x3.shape
        k, s, p = self.kernel_size[0], self.stride[0], self.padding[0]
        off3, out_levels = Y.conv_forward_raw(
            x3, self.conv_offset.weight, s, p, levels,
            bias=self.conv_offset.bias)
        (ho, wo), = out_levels
        col = self._sample(x3, off3, h, w, k, s, p)
        if self.groups != 1:
            # grouped DCN (ResNeXt-DCN, resnext.py:62-74): rows [g * cg * k * k,
            # (g + 1) * cg * k * k) of the column tensor feed group g -- a grouped
            # 1x1 conv over Cin * k * k channels
            y3, _ = Y.gconv_forward(col, self._weight_2d(), self.groups, 1, 0,
                                    ((ho, wo), ), scale, shift, relu)
            return y3, out_levels
        y3, _ = Y.conv_forward_raw(col, self._weight_2d(), 1, 0,
                                   ((ho, wo), ), bias=self.bias, scale=scale,
                                   shift=shift, residual=residual, relu=relu)
        return y3, out_levels

    def forward3(self, x3, levels):
        return self.forward3_fused(x3, levels)

    def forward(self, x):
        if torch.is_grad_enabled() and (x.requires_grad or
                                        self.weight.requires_grad):
            raise NotImplementedError(
                f'{type(self).__name__}.forward (4-D) is inference-only: call '
                'it under torch.no_grad(); the trainable entry points are '
                'forward3 / forward3_bn on (N, C, H*W) tensors')
        n, c, h, w = x.shape
        y3, lv = self.forward3(x.reshape(n, c, h * w), ((h, w), ))
        return y3.view(n, self.out_channels, lv[0][0], lv[0][1])


class DeformConv2dPack(_DeformConvPack):
    """mmcv.ops.DeformConv2dPack (conv type 'DCN'): deformable convolution v1
    whose offsets come from its own ``conv_offset`` 3x3 conv (zero-initialised,
    with bias).  Parameter names / shapes as mmcv's: ``weight`` (Cout, Cin, k,
    k), no bias, ``conv_offset.weight`` (2*k*k*deform_groups, Cin, k, k),
    ``conv_offset.bias``.  deform_groups = 1, no dilation.

    Frozen or under ``torch.no_grad()`` (the R101-DCN teacher of config 4,
    resnet.py:171-194): offset conv -> ld_deform_im2col -> 1x1 GEMM with the
    fused epilogue, three launches, no autograd (``groups`` > 1: the grouped
    GEMM of the X-101 teacher).

    Trainable (``forward3`` / ``forward3_fused`` / ``forward3_bn`` with
    autograd on and anything upstream or inside that needs a gradient;
    configs/gfl/gfl_r101_fpn_dconv_c3-c5_mstrain_2x_coco.py): the offset conv is
    a layers.ConvFn, the sampling a layers.DeformIm2colFn (offset gradient +
    sorted, atomic-free data gradient, csrc/dcn.hip) and the product with
    ``weight.view(Cout, Cin*k*k, 1, 1)`` the differentiable 1x1 conv
    (layers.conv2d, or layers.conv_bn_act with the following eval-mode BN), so
    the GEMM's dgrad / wgrad and the BN backward are the existing kernels.
    ``groups`` > 1 (configs/imv2/gflv2_x101_fpn_2x_coco.py): the product is
    layers.gconv2d over the Cin*k*k column channels followed by the BN node,
    fp32 only and only as that conv + BN pair.  The input must exist in fp32
    (not C8-only).  The 4-D
    convenience ``forward`` stays inference-only."""

    def _check_args(self, deform_groups, bias, groups):
        if deform_groups != 1 or bias:
            raise NotImplementedError(
                'DCN: deform_groups = 1 and no bias (the configs/gfl/*dconv* '
                'and configs/imv2/gflv2_x101* settings) are built')

    def _sample(self, x3, off3, h, w, k, s, p):
        return Y.deform_im2col(x3, off3, h, w, k, s, p, 1)

    def _sample_fn(self, x3, off3, h, w, k, s, p):
        return Y.deform_im2col_fn(x3, off3, h, w, k, s, p)


class ModulatedDeformConv2dPack(_DeformConvPack):
    """mmcv.ops.ModulatedDeformConv2dPack (conv type 'DCNv2'): deformable
    convolution v2, DeformConv2dPack with a modulation mask.  ``conv_offset``
    has 3*k*k channels: [0, 2*k*k) the offsets, (dy, dx) interleaved per tap as
    in v1, [2*k*k, 3*k*k) the mask logits (mmcv: ``o1, o2, mask = chunk(out,
    3, 1); offset = cat(o1, o2); mask = sigmoid(mask)``); the sample of tap t
    is sigmoid(logit_t) times v1's bilinear sum, so the zero-initialised layer
    is 0.5 x the plain convolution.  Parity with mmcv itself is UNPINNED (the
    op is not in the reference checkout; tests/_mdcn_ref64.py restates it).

    Parameter names / shapes as mmcv's: ``weight`` (Cout, Cin/groups, k, k),
    an optional ``bias`` (Cout) (mmcv's class default is bias=True; ResNet and
    ConvModule pass False), ``conv_offset.weight`` (3*k*k, Cin, k, k),
    ``conv_offset.bias``.  A checkpoint from before mmcv's module version 2
    carries ``<name>_offset.weight / .bias``; they load into ``conv_offset``.

    The three paths are DeformConv2dPack's with the sampling replaced by
    ld_mdeform_im2col / layers.ModulatedDeformIm2colFn (csrc/dcn.hip): frozen or
    ``no_grad`` in three launches (``groups`` > 1 through gconv_forward),
    trainable plain or as conv + eval-BN pair, trainable grouped as conv + BN
    pair in fp32.  ``bias`` is added by the 1x1 GEMM on the paths without a
    folded norm; together with ``bn`` / ``scale`` / ``shift``, or with
    ``groups`` > 1, it is refused by name.  deform_groups = 1, no dilation."""

    _NAME = 'DCNv2'
    _TAP_CHANNELS = 3
    _NOT_SQUARE = 'DCNv2: only square kernels/strides/pads'
    _version = 2

    def __init__(self, in_channels, out_channels, kernel_size, stride=1,
                 padding=0, dilation=1, groups=1, deform_groups=1, bias=True,
                 **kwargs):
        super().__init__(in_channels, out_channels, kernel_size, stride,
                         padding, dilation, groups, deform_groups, bias,
                         **kwargs)

    def _check_args(self, deform_groups, bias, groups):
        if deform_groups != 1:
            raise NotImplementedError(
                f'DCNv2: deform_groups = {deform_groups} is not built '
                '(deform_groups = 1 is)')
        if bias and groups != 1:
            raise NotImplementedError(
                'grouped DCNv2 with a bias (the grouped GEMM has no bias '
                'operand; ResNeXt passes bias=False)')

    def _sample(self, x3, om3, h, w, k, s, p):
        return Y.mdeform_im2col(x3, om3, h, w, k, s, p, 1)

    def _sample_fn(self, x3, om3, h, w, k, s, p):
        return Y.mdeform_im2col_fn(x3, om3, h, w, k, s, p)

    @staticmethod
    def rename_legacy_keys(state_dict, prefix, version):
        """mmcv's version-2 rename, in place: a checkpoint without a module
        version, or with one below 2, carries the offset conv as ``<prefix
        minus its trailing dot>_offset.weight / .bias``."""
        if version is None or version < 2:
            for leaf in ('weight', 'bias'):
                old = prefix[:-1] + '_offset.' + leaf
                new = prefix + 'conv_offset.' + leaf
                if new not in state_dict and old in state_dict:
                    state_dict[new] = state_dict.pop(old)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata,
                              strict, missing_keys, unexpected_keys,
                              error_msgs):
        # nn.Module.load_state_dict hands a nested module only the keys under
        # its own prefix, so this serves a layer loaded on its own (as mmcv's
        # loader, which passes the whole dict, serves every depth);
        # checkpoint.load_state_dict applies the same rename at every depth
        self.rename_legacy_keys(state_dict, prefix,
                                local_metadata.get('version', None))
        super()._load_from_state_dict(state_dict, prefix, local_metadata,
                                      strict, missing_keys, unexpected_keys,
                                      error_msgs)


def train_bn_refusals(conv, bn):
    """What a conv followed by a training-mode BatchNorm2d refuses, asked
    before the conv launches.  After a DeformConv2dPack it is refused by name:
    the trainable DCN runs conv + BN as one node with the folded eval
    coefficients (``forward3_bn``), which batch statistics cannot take."""
    if not (isinstance(bn, BatchNorm2d) and bn.training):
        return
    if isinstance(conv, _DeformConvPack):
        raise NotImplementedError(
            'BatchNorm2d in training mode (batch statistics) after a '
            f'{type(conv).__name__} is not implemented: keep the norm layers '
            f'of {conv._NAME} blocks in eval mode (norm_eval=True)')
    Y.bn_train_check(bn.momentum)


class BatchNorm2d(nn.Module):
    """BatchNorm2d.  Eval mode: its running statistics (the LD configs run
    every BN with norm_eval=True, resnet.py:639-648), affine trainable.
    Training mode (norm_eval=False): the batch's own statistics, and the
    running statistics / num_batches_tracked updated on the device as
    torch.nn.BatchNorm2d does (layers.bn_train_act; fp32 mode only)."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1):
        super().__init__()
        self.num_features, self.eps, self.momentum = num_features, eps, momentum
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer('running_mean', torch.zeros(num_features))
        self.register_buffer('running_var', torch.ones(num_features))
        self.register_buffer('num_batches_tracked',
                             torch.tensor(0, dtype=torch.long))

    def forward3(self, x3, residual=None, relu=False):
        if self.training:
            # a replayed step rewrites the buffers without passing here: the
            # mode switch after it (``train``) drops the eval coefficients
            self._ld_trained = True
            return Y.bn_train_act(x3, self.weight, self.bias,
                                  self.running_mean, self.running_var,
                                  self.num_batches_tracked, self.eps,
                                  self.momentum, residual, relu)
        return Y.bn_act(x3, self.weight, self.bias, self.running_mean,
                        self.running_var, self.eps, residual, relu)

    def train(self, mode=True):
        if getattr(self, '_ld_trained', False):
            Y.bn_stats_changed(self.weight)
        return super().train(mode)

    def forward(self, x):
        n, c, h, w = x.shape
        return self.forward3(x.reshape(n, c, h * w)).view(n, c, h, w)


class GroupNorm(nn.Module):

    def __init__(self, num_groups, num_channels, eps=1e-5):
        super().__init__()
        self.num_groups, self.num_channels, self.eps = (num_groups,
                                                        num_channels, eps)
        self.weight = nn.Parameter(torch.ones(num_channels))
        self.bias = nn.Parameter(torch.zeros(num_channels))

    def forward3(self, x3, levels, relu=False):
        return Y.gn_act(x3, self.weight, self.bias, self.num_groups, self.eps,
                        levels, relu)

    def forward(self, x):
        n, c, h, w = x.shape
        return self.forward3(x.reshape(n, c, h * w), ((h, w), )).view(
            n, c, h, w)


class ReLU(nn.Module):
    """Marker module (mmcv ConvModule.activate); the ReLU itself is fused
    into the preceding norm / conv epilogue kernel."""

    def __init__(self, inplace=True):
        super().__init__()
        self.inplace = inplace


def build_conv_layer(cfg, *args, **kwargs):
    if cfg is None:
        cfg = dict(type='Conv2d')
    layer_type = cfg['type'] if isinstance(cfg, dict) else cfg
    if layer_type in ('Conv2d', 'Conv'):
        if kwargs.get('groups', 1) != 1:
            return GroupedConv2d(*args, **kwargs)
        return Conv2d(*args, **kwargs)
    if layer_type == 'DCN':
        kw = {k: v for k, v in cfg.items() if k != 'type'}
        kw.update(kwargs)
        return DeformConv2dPack(*args, **kw)
    if layer_type == 'DCNv2':
        kw = {k: v for k, v in cfg.items() if k != 'type'}
        kw.update(kwargs)
        return ModulatedDeformConv2dPack(*args, **kw)
    raise NotImplementedError(
        f'conv layer type {layer_type} is not implemented on the MI355X path '
        "(built: 'Conv2d' / 'Conv', 'DCN', 'DCNv2')")


def build_norm_layer(cfg, num_features, postfix=''):
    """-> (name, layer); mmcv: 'BN' -> bn{postfix}, 'GN' -> gn{postfix}."""
    cfg_ = dict(cfg)
    layer_type = cfg_.pop('type')
    requires_grad = cfg_.pop('requires_grad', True)
    cfg_.setdefault('eps', 1e-5)
    if layer_type == 'BN':
        layer, abbr = BatchNorm2d(num_features, **cfg_), 'bn'
    elif layer_type == 'GN':
        assert 'num_groups' in cfg_
        layer, abbr = GroupNorm(num_channels=num_features, **cfg_), 'gn'
    else:
        raise NotImplementedError(f'norm type {layer_type}')
    for p in layer.parameters():
        p.requires_grad = requires_grad
    return abbr + str(postfix), layer


class Scale(nn.Module):
    """mmcv.cnn.Scale: a learnable scalar."""

    def __init__(self, scale=1.0):
        super().__init__()
        self.scale = nn.Parameter(torch.tensor(scale, dtype=torch.float))

    def forward(self, x):
        n, c, h, w = x.shape
        return Y.scale_levels(x.reshape(n, c, h * w), self.scale.reshape(1),
                              ((h, w), )).view(n, c, h, w)


class ConvModule(nn.Module):
    """conv -> norm -> activation, mmcv semantics: bias='auto' means bias iff
    there is no norm; the norm layer is registered as ``gn`` / ``bn``."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1,
                 padding=0, dilation=1, groups=1, bias='auto', conv_cfg=None,
                 norm_cfg=None, act_cfg=dict(type='ReLU'), inplace=True,
                 with_spectral_norm=False, padding_mode='zeros',
                 order=('conv', 'norm', 'act')):
        super().__init__()
        assert order == ('conv', 'norm', 'act') and padding_mode == 'zeros'
        assert not with_spectral_norm
        self.with_norm = norm_cfg is not None
        self.with_activation = act_cfg is not None
        if bias == 'auto':
            bias = not self.with_norm
        self.with_bias = bias
        self.conv = build_conv_layer(conv_cfg, in_channels, out_channels,
                                     kernel_size, stride=stride,
                                     padding=padding, dilation=dilation,
                                     groups=groups, bias=bias)
        self.in_channels, self.out_channels = in_channels, out_channels
        if self.with_norm:
            self.norm_name, norm = build_norm_layer(norm_cfg, out_channels)
            self.add_module(self.norm_name, norm)
        if self.with_activation:
            if act_cfg['type'] != 'ReLU':
                raise NotImplementedError(act_cfg['type'])
            self.activate = ReLU(inplace=inplace)
        self.init_weights()

    @property
    def norm(self):
        return getattr(self, self.norm_name)

    def init_weights(self):
        kaiming_init(self.conv, a=0, nonlinearity='relu')
        if self.with_norm:
            constant_init(self.norm, 1, bias=0)

    def forward3(self, x3, levels, activate=True, norm=True, c8_out=False):
        """``c8_out``: the caller's next layer is another conv of this kind -- a
        frozen conv + GN layer in bf16 mode may then return its output as a
        layers.C8Act (no fp32 copy)."""
        act = activate and self.with_activation
        if act and not (norm and self.with_norm):
            # conv (+bias) -> ReLU (RetinaGFLHead's towers, norm_cfg=None)
            c = self.conv
            if type(c) is Conv2d and not (torch.is_grad_enabled() and (
                    x3.requires_grad or c.weight.requires_grad or
                    (c.bias is not None and c.bias.requires_grad))):
                return Y.conv_forward_raw(x3, c.weight, c.stride[0],
                                          c.padding[0], levels, bias=c.bias,
                                          relu=True, emit_c8=True)
            y3, lv = c.forward3(x3, levels)
            return Y.relu(y3), lv
        if norm and self.with_norm and type(self.conv) is Conv2d and \
                self.conv.bias is None and type(self.norm) is GroupNorm:
            # trainable tower layer: one autograd node in bf16 mode (the pair
            # of launches otherwise) -- layers.conv_gn_act
            c, n = self.conv, self.norm
            return Y.conv_gn_act(x3, c.weight, n.weight, n.bias, n.num_groups,
                                 n.eps, c.stride[0], c.padding[0], levels,
                                 relu=act, c8_only=c8_out)
        if norm and self.with_norm:
            train_bn_refusals(self.conv, self.norm)
        y3, lv = self.conv.forward3(x3, levels)
        if norm and self.with_norm:
            n = self.norm
            if isinstance(n, GroupNorm):
                y3 = n.forward3(y3, lv, relu=act)
            else:
                y3 = n.forward3(y3, None, relu=act)
        return y3, lv

    def forward(self, x, activate=True, norm=True):
        n, c, h, w = x.shape
        y3, lv = self.forward3(x.reshape(n, c, h * w), ((h, w), ), activate,
                               norm)
        return y3.view(n, self.out_channels, lv[0][0], lv[0][1])
