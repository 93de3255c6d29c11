"""The float64 restatement of DCNv1 the device gradients are checked against
(tests/_dcn_ref64.py): it agrees with the forward-only float32 oracle
(oracle/dcn_oracle.py) and its autograd gradients pass torch's numerical
gradcheck away from the integer coordinates, where the bilinear surface has its
kinks."""
import pytest
import torch

import _dcn_ref64 as R

CASES = [(2, 5, 7, 11, 1), (1, 5, 9, 10, 2), (1, 3, 4, 5, 1)]


def _case(N, C, H, W, stride, seed, cout=4):
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    off = R.grid_offsets((N, 18, Ho, Wo), g)
    w = torch.randn(cout, C, 3, 3, generator=g, dtype=torch.float64) / (9 * C)**0.5
    return x, off, w


@pytest.mark.parametrize('N,C,H,W,stride', CASES)
def test_ref64_matches_fp32_oracle(N, C, H, W, stride):
    """Forward, evaluated in float32 and in float64, against the float32 oracle:
    within fp32 rounding of a sum of Cin*9 products (the coordinates are exact in
    both formats, so the same cells are sampled)."""
    import dcn_oracle as D
    x, off, w = _case(N, C, H, W, stride, seed=H * 100 + W)
    # force the special regions: integer coordinates, the (-1, 0) border band
    off[:, :, 0, 0] = 0.0
    off[:, 0, 0, 1], off[:, 1, 0, 1] = -0.5, -0.25
    ref = D.deform_conv2d(x.float(), off.float(), w.float(), stride, 1)
    col_ref = D.deform_sample(x.float(), off.float(), 3, stride, 1)
    col32 = R.deform_im2col(x.float(), off.float(), 3, stride, 1)
    col64 = R.deform_im2col(x, off, 3, stride, 1)
    assert col32.dtype == torch.float32 and col64.dtype == torch.float64
    col_ref = col_ref.reshape(col32.shape)
    # one sample = four products: a few ulp of the largest term
    tol = 4 * 2.0**-23 * float(x.abs().max())
    assert float((col32 - col_ref).abs().max()) <= tol
    assert float((col64 - col_ref.double()).abs().max()) <= tol
    y32 = R.deform_conv2d(x.float(), off.float(), w.float(), stride, 1)
    y64 = R.deform_conv2d(x, off, w, stride, 1)
    # sum of Cin*9 terms: n * eps * sum|terms| bounds any summation order
    bound = (9 * C + 4) * 2.0**-23 * float(
        torch.matmul(w.abs().reshape(w.shape[0], -1), col64.abs()).max())
    assert float((y32 - ref).abs().max()) <= bound
    assert float((y64 - ref.double()).abs().max()) <= bound
    # the Pack form: offsets from the layer's own conv
    ow = torch.randn(18, C, 3, 3, dtype=torch.float64,
                     generator=torch.Generator().manual_seed(3)) * 0.3
    ob = torch.linspace(-1, 1, 18, dtype=torch.float64)
    yp, offp = R.dcn_pack_forward(x, w, ow, ob, stride, 1)
    yr, offr = D.dcn_pack_forward(x.float(), w.float(), ow.float(), ob.float(),
                                  stride, 1)
    assert float((offp - offr.double()).abs().max()) < 1e-4
    assert yp.shape == yr.shape


@pytest.mark.parametrize('N,C,H,W,stride', CASES[1:])
def test_ref64_gradcheck_away_from_integers(N, C, H, W, stride):
    """torch.autograd.gradcheck of x, offset and weight.  Coordinates are kept
    >= 1/8 away from every integer (and so from -1, H, W as well): the
    numerical derivative's step of 1e-6 then never crosses a kink."""
    x, off, w = _case(N, C, H, W, stride, seed=7 * H + W)
    frac = off - torch.floor(off)
    off = torch.floor(off) + frac.clamp(0.125, 0.875)
    py, px = R.sample_coords(off, H, W, 3, stride, 1)
    for c in (py, px):
        assert float((c - torch.round(c)).abs().min()) >= 0.125 - 1e-12
    # the regions that matter are present: border band and outside the map
    assert bool(((py > -1) & (py < 0)).any()) and bool((py < -1).any())
    assert bool(((px > W - 1) & (px < W)).any()) and bool((px > W).any())
    x.requires_grad_(True)
    off.requires_grad_(True)
    w.requires_grad_(True)
    assert torch.autograd.gradcheck(
        lambda a, b, c: R.deform_conv2d(a, b, c, stride, 1), (x, off, w),
        eps=1e-6, atol=1e-7, rtol=1e-5)
