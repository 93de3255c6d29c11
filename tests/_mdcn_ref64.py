"""TEST INFRASTRUCTURE ONLY -- modulated deformable convolution (DCNv2) restated
for autograd in any floating dtype, on top of tests/_dcn_ref64.py (float64 is
the truth; float32 on the CPU gives the error a correct fp32 evaluation makes).

mmcv.ops.ModulatedDeformConv2dPack, deform_groups = 1 (Zhu et al. 2019): the
conv_offset output ``om`` (N, 3*k*k, Ho, Wo) holds the offsets in channels
[0, 2*k*k), (dy, dx) interleaved per tap as in v1, and the mask logits in
channels [2*k*k, 3*k*k), one per tap (mmcv: ``o1, o2, mask = chunk(om, 3, 1);
offset = cat(o1, o2); mask = sigmoid(mask)``).  The sample of tap t is
sigmoid(logit_t) times v1's bilinear sum.  Parity with mmcv itself is
unpinned, as for v1.
"""
import torch
import torch.nn.functional as F

import _dcn_ref64 as R


def modulated_im2col(x, om, k, stride, pad):
    """x (N, C, H, W), om (N, 3*k*k, Ho, Wo) -> col (N, C*k*k, Ho*Wo), channel
    = ci*k*k + tap (the layout of ld_mdeform_im2col)."""
    N, C = x.shape[:2]
    kk = k * k
    Ho, Wo = om.shape[2:]
    col = R.deform_im2col(x, om[:, :2 * kk], k, stride, pad)
    mask = torch.sigmoid(om[:, 2 * kk:]).reshape(N, 1, kk, Ho * Wo)
    return (col.view(N, C, kk, Ho * Wo) * mask).reshape(N, C * kk, Ho * Wo)


def mdcn_pack_forward(x, weight, bias, off_w, off_b, stride=1, pad=1):
    """ModulatedDeformConv2dPack: om from the layer's own conv; -> (y, om).
    ``weight`` (Cout, Cin, k, k); ``bias`` (Cout) or None."""
    k = weight.shape[2]
    om = F.conv2d(x, off_w, off_b, stride=stride, padding=pad)
    col = modulated_im2col(x, om, k, stride, pad)
    y = torch.matmul(weight.reshape(weight.shape[0], -1), col)
    if bias is not None:
        y = y + bias.view(1, -1, 1)
    return y.view(x.shape[0], weight.shape[0], om.shape[2], om.shape[3]), om


def mdcn_pack_forward_grouped(x, weight, off_w, off_b, groups, stride=1,
                              pad=1):
    """The grouped layer: rows [g*cg*k*k, (g+1)*cg*k*k) of the column tensor
    feed output-channel group g.  ``weight`` (Cout, Cin/groups, k, k)."""
    k = weight.shape[2]
    N = x.shape[0]
    cout = weight.shape[0]
    om = F.conv2d(x, off_w, off_b, stride=stride, padding=pad)
    col = modulated_im2col(x, om, k, stride, pad)
    colg = col.view(N, groups, -1, col.shape[2])
    wg = weight.reshape(groups, cout // groups, -1)
    y = torch.einsum('gok,ngkp->ngop', wg, colg)
    return y.reshape(N, cout, om.shape[2], om.shape[3]), om
