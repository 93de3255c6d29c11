"""TEST INFRASTRUCTURE ONLY -- grouped convolution for autograd in float64 (the
truth the device gradients are held to) and float32 on the CPU (the error a
correct fp32 evaluation makes): torch.nn.functional.conv2d(..., groups=G), the
op the reference's ResNeXt runs (mmdet/models/backbones/resnext.py:49-61), and
the grouped DCN as tests/_dcn_ref64.py's sampling followed by the grouped 1x1;
``resnext_forward`` restates ResNeXtBottleneck (resnext.py:11-85, style
'pytorch': the stride sits on the grouped conv2) and the backbone built from
it (resnet.py:622-637) functionally over a state dict, in the dtype of its
tensors."""
import torch
import torch.nn.functional as F

import _dcn_ref64 as D


def gconv_grads(x, w, dy, groups, stride, pad, dtype):
    """-> (y, dx, dw) of conv2d(x, w, groups) under the output gradient dy."""
    a = x.detach().clone().to(dtype).requires_grad_(True)
    b = w.detach().clone().to(dtype).requires_grad_(True)
    y = F.conv2d(a, b, None, stride, pad, 1, groups)
    y.backward(dy.to(dtype))
    return y.detach(), a.grad, b.grad


def bn_eval(y, gamma, beta, mean, var, eps):
    s = gamma / torch.sqrt(var + eps)
    return y * s.view(1, -1, 1, 1) + (beta - mean * s).view(1, -1, 1, 1)


def gconv_bn_grads(x, w, bn, residual, relu, dy, groups, stride, dtype):
    """relu?(BN_eval(gconv(x)) + residual); bn = (gamma, beta, mean, var, eps).
    -> (y, dx, dw, dgamma, dbeta)."""
    a = x.detach().clone().to(dtype).requires_grad_(True)
    b = w.detach().clone().to(dtype).requires_grad_(True)
    ga, be = (t.detach().clone().to(dtype).requires_grad_(True) for t in bn[:2])
    y = F.conv2d(a, b, None, stride, w.shape[2] // 2, 1, groups)
    y = bn_eval(y, ga, be, bn[2].to(dtype), bn[3].to(dtype), bn[4])
    if residual is not None:
        y = y + residual.to(dtype)
    if relu:
        y = torch.relu(y)
    y.backward(dy.to(dtype))
    return y.detach(), a.grad, b.grad, ga.grad, be.grad


def gdcn_bn_grads(x, w, off_w, off_b, bn, dy, groups, stride, dtype):
    """Grouped DeformConv2dPack + eval BN: offsets from the layer's own conv,
    _dcn_ref64's sampling, then the grouped 1x1 over Cin*9 column channels.
    -> (y, dx, dw, d off_w, d off_b, dgamma, dbeta)."""
    ts = [t.detach().clone().to(dtype).requires_grad_(True)
          for t in (x, w, off_w, off_b, bn[0], bn[1])]
    a, b, ow, ob, ga, be = ts
    N, _, H, W = x.shape
    offset = F.conv2d(a, ow, ob, stride=stride, padding=1)
    col = D.deform_im2col(a, offset, 3, stride, 1)
    ho, wo = offset.shape[2:]
    y = F.conv2d(col.view(N, -1, ho, wo), b.reshape(b.shape[0], -1, 1, 1), None,
                 1, 0, 1, groups)
    y = bn_eval(y, ga, be, bn[2].to(dtype), bn[3].to(dtype), bn[4])
    y.backward(dy.to(dtype))
    return (y.detach(), ) + tuple(t.grad for t in ts)


def resnext_forward(sd, x, groups=32, blocks=(3, 4, 6, 3)):
    """The four stage outputs of ResNeXt (norm_eval, eps 1e-5) for the state
    dict ``sd`` (mmdet's key names) -- differentiable in every entry of ``sd``
    that requires a gradient."""

    def bn(y, p):
        return bn_eval(y, sd[p + '.weight'], sd[p + '.bias'],
                       sd[p + '.running_mean'], sd[p + '.running_var'], 1e-5)

    y = torch.relu(bn(F.conv2d(x, sd['conv1.weight'], None, 2, 3), 'bn1'))
    y = F.max_pool2d(y, 3, 2, 1)
    outs = []
    for i, nb in enumerate(blocks):
        for b in range(nb):
            p = f'layer{i + 1}.{b}'
            s = 2 if (b == 0 and i > 0) else 1
            idt = y
            if p + '.downsample.0.weight' in sd:
                idt = bn(F.conv2d(y, sd[p + '.downsample.0.weight'], None, s),
                         p + '.downsample.1')
            o = torch.relu(bn(F.conv2d(y, sd[p + '.conv1.weight']), p + '.bn1'))
            o = torch.relu(bn(F.conv2d(o, sd[p + '.conv2.weight'], None, s, 1, 1,
                                       groups), p + '.bn2'))
            o = bn(F.conv2d(o, sd[p + '.conv3.weight']), p + '.bn3')
            y = torch.relu(o + idt)
        outs.append(y)
    return outs


def block_diagonal(w, groups):
    """The dense (Cout, Cin, k, k) weight of a grouped (Cout, Cin/G, k, k) one:
    the grouped weight embedded in zeros.  -> (dense, mask of the blocks)."""
    cout, cin_g, kh, kw = w.shape
    cg = cout // groups
    dense = w.new_zeros((cout, cin_g * groups, kh, kw))
    mask = torch.zeros_like(dense)
    for g in range(groups):
        dense[g * cg:(g + 1) * cg, g * cin_g:(g + 1) * cin_g] = \
            w[g * cg:(g + 1) * cg]
        mask[g * cg:(g + 1) * cg, g * cin_g:(g + 1) * cin_g] = 1
    return dense, mask
