"""TEST INFRASTRUCTURE ONLY -- deformable convolution v1 restated for autograd in
any floating dtype (float64 is the truth the device gradients are held to;
float32 on the CPU gives the error a correct fp32 evaluation makes).

oracle/dcn_oracle.py hard-codes float32 and is forward-only; this restatement
follows the same published algorithm (Dai et al. 2017, eq. 2-4) and the same
conventions as ld_amd/csrc/dcn.hip: (dy, dx) interleaved per tap, value 0
unless -1 < h < H and -1 < w < W, neighbours outside the map contribute 0, and
floor picks the cell -- it is constant under differentiation, so at an integer
coordinate the offset gradient is the forward difference into cell floor + 1.
Dense torch ops: one index_select-style gather per bilinear corner over the
flattened map; everything is differentiable in x, the offsets and the weights.
"""
import torch
import torch.nn.functional as F


def sample_coords(offset, H, W, k, stride, pad):
    """offset (N, 2*k*k, Ho, Wo) -> sampling rows / columns (N, k*k, Ho, Wo)."""
    N, _, Ho, Wo = offset.shape
    dt, dev = offset.dtype, offset.device
    taps = torch.arange(k * k, device=dev)
    base_y = (torch.arange(Ho, device=dev) * stride - pad).view(1, 1, Ho, 1) + \
        (taps // k).view(1, -1, 1, 1)
    base_x = (torch.arange(Wo, device=dev) * stride - pad).view(1, 1, 1, Wo) + \
        (taps % k).view(1, -1, 1, 1)
    return base_y.to(dt) + offset[:, 0::2], base_x.to(dt) + offset[:, 1::2]


def deform_im2col(x, offset, k, stride, pad):
    """x (N, C, H, W), offset (N, 2*k*k, Ho, Wo) -> col (N, C*k*k, Ho*Wo), channel
    = ci*k*k + tap (the layout of ld_deform_im2col)."""
    N, C, H, W = x.shape
    Ho, Wo = offset.shape[2:]
    py, px = sample_coords(offset, H, W, k, stride, pad)
    inside = (py > -1) & (px > -1) & (py < H) & (px < W)
    y0, x0 = torch.floor(py).detach(), torch.floor(px).detach()
    ly, lx = py - y0, px - x0
    flat = x.reshape(N, C, H * W)
    T = k * k * Ho * Wo
    col = x.new_zeros((N, C, T))
    for cy, cx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        yy, xx = y0 + cy, x0 + cx
        ok = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        wy = ly if cy else 1 - ly
        wx = lx if cx else 1 - lx
        wgt = torch.where(ok, wy * wx, torch.zeros_like(wy))
        idx = torch.where(ok, yy * W + xx, torch.zeros_like(yy)).long()
        idx = idx.reshape(N, 1, T).expand(N, C, T)
        col = col + torch.gather(flat, 2, idx) * wgt.reshape(N, 1, T)
    return col.view(N, C * k * k, Ho * Wo)


def deform_conv2d(x, offset, weight, stride=1, pad=1):
    """y (N, Cout, Ho, Wo) = weight.view(Cout, Cin*k*k) @ col."""
    k = weight.shape[2]
    col = deform_im2col(x, offset, k, stride, pad)
    y = torch.matmul(weight.reshape(weight.shape[0], -1), col)
    return y.view(x.shape[0], weight.shape[0], offset.shape[2], offset.shape[3])


def dcn_pack_forward(x, weight, off_w, off_b, stride=1, pad=1):
    """DeformConv2dPack: offsets from the layer's own conv; -> (y, offset)."""
    offset = F.conv2d(x, off_w, off_b, stride=stride, padding=pad)
    return deform_conv2d(x, offset, weight, stride, pad), offset


def grid_offsets(shape, gen, lo=-4.0, hi=4.0, step=1.0 / 64):
    """Offsets on a ``step`` grid in [lo, hi]: sampling coordinates are then exact
    in float32 and float64 alike, so no floor can flip between the two."""
    n = int(round((hi - lo) / step))
    return torch.randint(0, n + 1, shape, generator=gen).double() * step + lo
