"""torch float64 restatements (CPU) of what landscape.hip computes, for the
landscape tests: the reference's ``abs(t - s).mean(1).sum()`` per level
(AP_landscape/apis/test.py:114-177) with the fp32 element differences it sums
and every sum in float64, and Pearson r of the channel maps of a level
(apis/test.py:106-111: audtorch's pearsonr is cov / (std_x * std_y) =
Sxy / sqrt(Sxx * Syy))."""
import numpy as np
import torch


def segments(levels):
    off, out = 0, []
    for h, w in levels:
        out.append((off, off + h * w))
        off += h * w
    return out


def pack(feats):
    """per-level (N, C, H, W) -> (N, C, P), levels."""
    levels = tuple((int(f.shape[2]), int(f.shape[3])) for f in feats)
    return torch.cat([f.detach().cpu().flatten(2) for f in feats], 2), levels


def abs_err(t3, s3, levels):
    """-> (N, L) float64: per image and level sum_p mean_c |t - s|, |t - s| in
    fp32."""
    d = (t3.float().cpu() - s3.float().cpu()).abs().double()
    return torch.stack([d[:, :, a:b].mean(1).sum(1)
                        for a, b in segments(levels)], 1)


def abs_err_reference_fp32(t3, s3, levels):
    """The reference's literal expression per image and level, fp32 on torch
    CPU tensors: permute(0, 2, 3, 1).reshape(-1, C), abs(t - s).mean(1).sum().
    -> (N, L) float32."""
    N, C, _ = t3.shape
    out = torch.zeros(N, len(levels))
    for l, (a, b) in enumerate(segments(levels)):
        for n in range(N):
            pt = t3[n:n + 1, :, a:b].permute(0, 2, 1).reshape(-1, C)
            ps = s3[n:n + 1, :, a:b].permute(0, 2, 1).reshape(-1, C)
            out[n, l] = torch.abs(pt - ps).mean(1).sum()
    return out


def pearson_rows(t3, s3, levels):
    """-> (N, L, C) float64: r of every (n, c) row of every level segment, NaN
    for a degenerate row (fewer than 2 positions, or constant in t or s)."""
    t, s = t3.double().cpu(), s3.double().cpu()
    out = []
    for a, b in segments(levels):
        x, y = t[:, :, a:b], s[:, :, a:b]
        dx, dy = x - x.mean(2, keepdim=True), y - y.mean(2, keepdim=True)
        sxy, sxx, syy = (dx * dy).sum(2), (dx * dx).sum(2), (dy * dy).sum(2)
        r = sxy / torch.sqrt(sxx * syy)
        bad = (sxx == 0) | (syy == 0) | torch.tensor(b - a < 2)
        out.append(torch.where(bad, torch.full_like(r, float('nan')), r))
    return torch.stack(out, 1)


def pearson(t3, s3, levels):
    """-> (r_sum (N, L) float64 over the valid rows, valid (N, L), degenerate
    (N, L)) as ld_levels_pearson reports them."""
    r = pearson_rows(t3, s3, levels)
    bad = torch.isnan(r)
    return (torch.where(bad, torch.zeros_like(r), r).sum(2),
            (~bad).sum(2), bad.sum(2))


def discrepancy(adds):
    """``adds``: per batch (xs, xt, outs_s, outs_t) as per-level lists.  -> the
    dict TeacherStudentDiscrepancy.compute returns."""
    fams = ('feature', 'cls', 'bbox')
    tot = {f: [] for f in fams}
    lev = {f: [] for f in fams}
    per_img, degen = [], []
    for xs, xt, outs_s, outs_t in adds:
        for f, s, t in (('feature', xs, xt), ('cls', outs_s[0], outs_t[0]),
                        ('bbox', outs_s[1], outs_t[1])):
            s3, levels = pack(s)
            t3, _ = pack(t)
            pos = np.array([h * w for h, w in levels], dtype=np.float64)
            e = abs_err(t3, s3, levels).numpy()
            tot[f].append(e.sum(1) / pos.sum())
            lev[f].append(e / pos[None])
            if f == 'feature':
                r, valid, bad = pearson(t3, s3, levels)
                r, valid = r.numpy(), valid.numpy()
                with np.errstate(invalid='ignore', divide='ignore'):
                    per_img.append(np.where(valid > 0, r / valid, np.nan))
                degen.append(bad.numpy())
    out = {}
    for f in fams:
        out[f'{f}_error'] = float(np.concatenate(tot[f]).mean())
        out[f'{f}_error_levels'] = np.concatenate(lev[f]).mean(0)
    per_img = np.concatenate(per_img)
    has = (~np.isnan(per_img)).sum(0)
    with np.errstate(invalid='ignore', divide='ignore'):
        out['pearson'] = np.where(has > 0, np.nansum(per_img, 0) / has, np.nan)
    out['degenerate_rows'] = np.concatenate(degen).sum(0)
    out['num_images'] = int(per_img.shape[0])
    return out
