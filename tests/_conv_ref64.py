"""Sampled float64 reference of the level-concatenated convolutions, with a
per-element error bar (host arithmetic; the operands may live on the device).

Layout: activations are (N, C, P) with the levels' (H, W) images concatenated
along P, as ld_amd.layers holds them; every level is convolved on its own with
the same k x k weight, stride and zero padding.

For each sampled output element the helpers return
  ref = sum_i t_i   (float64; t_i the exact products of the operands the kernel
                     consumed: fp32 operands, or in bf16 mode the RNE-rounded
                     ones -- forward rounds x and w, dgrad dy and w, wgrad dy
                     and x),
  S   = sum_i |t_i|,
  K   = the number of terms.
The product of two fp32 (or bf16) values is exact in float64 and the float64
sum of <= 2^20 of them is off by far less than 2^-24 S, so ref is the exact
result for the purpose of the bar

  |got - ref| <= BAR * u * S,   u = 2^-24, BAR = 16   (fixed, not per layer).

Any fp32 summation order stays within (K - 1) u S in the worst case, and near
sqrt(K) u S or below when the products have zero mean.  A dropped term of
average size, S / K, exceeds 16 u S whenever K < 2^24 / 16 ~ 10^6 -- every
layer here.  The inputs of the checks must therefore make the products zero
mean: w and dy from randn, x from randn or |randn|.  Then the kernel's own
rounding stays near sqrt(K) u S/K-sized steps, far inside the bar, while a
missing or misplaced term still breaks it.  With all-positive products the
worst-case (K - 1) u S growth of an fp32 sum would come close to the bar at
large K and the check would lose its sharpness.

Sampling is deterministic where kernels break (level borders and boundaries,
tile edges of P, channel tile edges) plus seeded random points, and a caller
gathers only the sampled patches (torch indexing, on the operands' device); no
full-size float64 convolution runs on the host.
"""
import numpy as np
import torch

U = 2.0 ** -24
BAR = 16.0
CHANNELS = (0, 1, 31, 32, 63, 64, 127, 128, 255, 256)


def bf16_rne(t):
    """t rounded to bf16 (round to nearest even), as fp32."""
    return t.to(torch.bfloat16).to(torch.float32)


def bf16_rtz(t):
    """t rounded to bf16 toward zero (truncated): the wrong rounding."""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


class Geom:
    """One conv geometry over level-concatenated positions."""

    def __init__(self, N, Cin, Cout, k, stride, pad, levels):
        self.N, self.Cin, self.Cout = int(N), int(Cin), int(Cout)
        self.k, self.stride, self.pad = int(k), int(stride), int(pad)
        self.levels = tuple((int(h), int(w)) for h, w in levels)
        self.out_levels, self.off_in, self.off_out = [], [], []
        pin = pout = 0
        for h, w in self.levels:
            ho = (h + 2 * pad - k) // stride + 1
            wo = (w + 2 * pad - k) // stride + 1
            self.out_levels.append((ho, wo))
            self.off_in.append(pin)
            self.off_out.append(pout)
            pin += h * w
            pout += ho * wo
        self.Pin, self.Pout = pin, pout
        self.T = k * k
        self._src = self._dst = None

    def __repr__(self):
        lv = 'x'.join(f'{h}:{w}' for h, w in self.levels)
        return (f'N{self.N} {self.Cin}>{self.Cout} k{self.k} s{self.stride} '
                f'p{self.pad} [{lv}]')

    def src(self):
        """(Pout, T) int64: input position each tap of each output position
        reads, -1 for a padding tap."""
        if self._src is None:
            parts = []
            kk = torch.arange(self.k)
            for (h, w), (ho, wo), oi in zip(self.levels, self.out_levels,
                                            self.off_in):
                hi = (torch.arange(ho)[:, None] * self.stride - self.pad +
                      kk[None, :])  # (ho, k)
                wi = (torch.arange(wo)[:, None] * self.stride - self.pad +
                      kk[None, :])  # (wo, k)
                H = hi[:, None, :, None].expand(ho, wo, self.k, self.k)
                W = wi[None, :, None, :].expand(ho, wo, self.k, self.k)
                ok = (H >= 0) & (H < h) & (W >= 0) & (W < w)
                pos = torch.where(ok, oi + H * w + W, torch.full_like(H, -1))
                parts.append(pos.reshape(ho * wo, self.T))
            self._src = torch.cat(parts, 0)
        return self._src

    def dst(self):
        """(Pin, T) int64: output position whose tap t reads input position q
        (at most one per tap), -1 if none -- the data gradient's gather."""
        if self._dst is None:
            s = self.src()
            d = torch.full((self.Pin, self.T), -1, dtype=torch.int64)
            p = torch.arange(self.Pout)[:, None].expand_as(s)
            t = torch.arange(self.T)[None, :].expand_as(s)
            ok = s >= 0
            d[s[ok], t[ok]] = p[ok]
            self._dst = d
        return self._dst


# ---------------------------------------------------------------- sampling --
def _level_positions(levels, offs):
    """First / last rows and columns of every level (corners and a middle
    point of each border) and both sides of each level boundary."""
    out = set()
    for (h, w), off in zip(levels, offs):
        rows = sorted({0, h - 1})
        cols = sorted({0, w - 1})
        for r in rows:
            for c in sorted({0, w // 2, w - 1, min(1, w - 1)}):
                out.add(off + r * w + c)
        for c in cols:
            for r in sorted({h // 2, min(1, h - 1), max(h - 2, 0)}):
                out.add(off + r * w + c)
        out.add(off)
        if off > 0:
            out.add(off - 1)
    return out


def sample_positions(levels, offs, P, rng, n_random=24):
    pos = _level_positions(levels, offs)
    pos.update({P - 1, P - 2})
    for m in (32, 64, 128, 256):
        mult = list(range(m, P, m))
        if not mult:
            continue
        pick = mult[:2] + mult[-2:]
        # multiples next to each level boundary, and a few seeded ones
        for off in offs[1:]:
            pick.append(off // m * m)
        pick += [int(v) for v in rng.choice(mult, min(4, len(mult)),
                                            replace=False)]
        for b in pick:
            for d in (-1, 0, 1):
                if 0 < b + d < P:
                    pos.add(b + d)
    pos.update(int(v) for v in rng.integers(0, P, n_random))
    return sorted(v for v in pos if 0 <= v < P)


def sample_channels(C):
    return sorted({c for c in CHANNELS if c < C} | {C - 1})


def sample_elements(N, C, levels, offs, P, seed, n_random=48):
    """(n, c, p) triples: every sampled position with a channel from the edge
    set (cycled), every edge channel at the first / last / a random position,
    and seeded random triples."""
    rng = np.random.default_rng(seed)
    pos = sample_positions(levels, offs, P, rng)
    ch = sample_channels(C)
    out = set()
    for i, p in enumerate(pos):
        out.add((i % N, ch[(i * 7) % len(ch)], p))
    for j, c in enumerate(ch):
        for p in (0, P - 1, int(rng.integers(0, P))):
            out.add(((j + p) % N, c, p))
    for _ in range(n_random):
        out.add((int(rng.integers(0, N)), int(rng.integers(0, C)),
                 int(rng.integers(0, P))))
    a = np.array(sorted(out), dtype=np.int64)
    return a[:, 0], a[:, 1], a[:, 2]


def sample_weights(g, seed, max_count=None):
    """(co, ci, tap) weight-gradient samples: every tap, the first and last
    co / ci, 128-row tile edges, seeded random."""
    rng = np.random.default_rng(seed)
    cos = sorted({c for c in CHANNELS + (g.Cout - 1, ) if c < g.Cout} |
                 {e for m in range(128, g.Cout + 1, 128)
                  for e in (m - 1, m) if e < g.Cout})
    cis = sorted({c for c in CHANNELS + (g.Cin - 1, ) if c < g.Cin} |
                 {e for m in range(128, g.Cin + 1, 128)
                  for e in (m - 1, m) if e < g.Cin})
    out = set()
    for t in range(g.T):  # every tap, at the extreme channel pairs
        out.add((0, 0, t))
        out.add((g.Cout - 1, g.Cin - 1, t))
        out.add((cos[t % len(cos)], cis[(t * 3) % len(cis)], t))
    for i, co in enumerate(cos):
        out.add((co, cis[i % len(cis)], i % g.T))
    for i, ci in enumerate(cis):
        out.add((cos[(i * 5) % len(cos)], ci, (i + 1) % g.T))
    for _ in range(16):
        out.add((int(rng.integers(0, g.Cout)), int(rng.integers(0, g.Cin)),
                 int(rng.integers(0, g.T))))
    a = sorted(out)
    if max_count is not None and len(a) > max_count:
        keep = set(rng.choice(len(a), max_count, replace=False).tolist())
        # the deterministic corner samples always stay
        keep.update(i for i, s in enumerate(a)
                    if s[:2] in ((0, 0), (g.Cout - 1, g.Cin - 1)))
        a = [a[i] for i in sorted(keep)]
    a = np.array(a, dtype=np.int64)
    return a[:, 0], a[:, 1], a[:, 2]


# ------------------------------------------------------------- reductions --
def _sum(terms):
    """terms: float64 (S, K) array; invalid terms are exact zeros."""
    return terms.sum(1), np.abs(terms).sum(1)


def _host(t):
    return t.detach().to('cpu', torch.float32).double().numpy()


def _idx(a, device):
    return torch.as_tensor(np.asarray(a), dtype=torch.int64, device=device)


def forward(g, x, w, n, co, p, bf16=False):
    """Sampled y[n, co, p] of y = conv(x, w).  x: (N, Cin, Pin), w: (Cout, Cin,
    k, k), any device.  Returns (ref, S, K) float64 / int arrays."""
    dev = x.device
    if bf16:
        x, w = bf16_rne(x), bf16_rne(w)
    src = g.src().to(dev)[_idx(p, dev)]  # (S, T)
    ok = src >= 0
    n_, co_ = _idx(n, dev), _idx(co, dev)
    xs = x[n_[:, None, None], torch.arange(g.Cin, device=dev)[None, :, None],
           src.clamp(min=0)[:, None, :]]  # (S, Cin, T)
    xs = xs * ok[:, None, :]
    ws = w.reshape(g.Cout, g.Cin, g.T)[co_]  # (S, Cin, T)
    terms = _host(xs).reshape(len(n), -1) * _host(ws).reshape(len(n), -1)
    ref, S = _sum(terms)
    K = _host(ok.sum(1)).astype(np.int64) * g.Cin
    return ref, S, K


def dgrad(g, dy, w, n, ci, q, bf16=False):
    """Sampled dx[n, ci, q] of dx = conv_transpose(dy, w) (the input gradient of
    y = conv(x, w)).  dy: (N, Cout, Pout)."""
    dev = dy.device
    if bf16:
        dy, w = bf16_rne(dy), bf16_rne(w)
    dst = g.dst().to(dev)[_idx(q, dev)]  # (S, T)
    ok = dst >= 0
    n_, ci_ = _idx(n, dev), _idx(ci, dev)
    ds = dy[n_[:, None, None], torch.arange(g.Cout, device=dev)[None, :, None],
            dst.clamp(min=0)[:, None, :]]  # (S, Cout, T)
    ds = ds * ok[:, None, :]
    ws = w.reshape(g.Cout, g.Cin, g.T)[:, ci_, :].permute(1, 0, 2)  # (S,Cout,T)
    terms = _host(ds).reshape(len(n), -1) * _host(ws).reshape(len(n), -1)
    ref, S = _sum(terms)
    K = _host(ok.sum(1)).astype(np.int64) * g.Cout
    return ref, S, K


def wgrad(g, x, dy, co, ci, t, bf16=False):
    """Sampled dw[co, ci, tap] of the weight gradient.  Sums over every image
    and output position the tap reaches."""
    dev = x.device
    if bf16:
        x, dy = bf16_rne(x), bf16_rne(dy)
    src = g.src().to(dev)  # (Pout, T)
    refs, Ss, Ks = [], [], []
    # a few samples per gather: each is (N, Pout) wide
    step = max(1, int(2 ** 22 // max(1, g.N * g.Pout)))
    for s0 in range(0, len(co), step):
        c_o = _idx(co[s0:s0 + step], dev)
        c_i = _idx(ci[s0:s0 + step], dev)
        tt = _idx(t[s0:s0 + step], dev)
        pos = src[:, tt].t()  # (s, Pout)
        ok = pos >= 0
        ds = dy[:, c_o, :].permute(1, 0, 2)  # (s, N, Pout)
        xs = x[torch.arange(g.N, device=dev)[None, :, None], c_i[:, None, None],
               pos.clamp(min=0)[:, None, :]]  # (s, N, Pout)
        xs = xs * ok[:, None, :]
        terms = _host(ds).reshape(len(c_o), -1) * _host(xs).reshape(len(c_o), -1)
        r, S = _sum(terms)
        refs.append(r)
        Ss.append(S)
        Ks.append(_host(ok.sum(1)).astype(np.int64) * g.N)
    return np.concatenate(refs), np.concatenate(Ss), np.concatenate(Ks)


# ------------------------------------------------------------------- bars --
def bound(S):
    return BAR * U * S


def epilogue(ref, S, scale=None, shift=None, res=None, relu=False, c8=False):
    """The fused epilogue y = relu(scale * acc + shift + res) applied to the
    sampled sums (scale / shift / res already gathered per sample, float64;
    shift includes the bias).  Returns (ref_y, bar)."""
    sc = np.ones_like(ref) if scale is None else scale
    sh = np.zeros_like(ref) if shift is None else shift
    rs = np.zeros_like(ref) if res is None else res
    v = sc * ref + sh + rs
    bar = np.abs(sc) * bound(S) + 4 * U * (np.abs(sc * ref) + np.abs(sh) +
                                           np.abs(rs))
    if relu:
        v = np.maximum(v, 0.0)
    if c8:
        bar = bar + 2.0 ** -8 * (np.abs(v) + bar)
    return v, bar


def check(got, ref, S, bar=None, what='', detail=None):
    """Assert |got - ref| <= bar (default 16 u S) on every sample.  Returns the
    largest |got - ref| / (u S) (0 where S == 0)."""
    got = np.asarray(got, dtype=np.float64)
    if bar is None:
        bar = bound(S)
    err = np.abs(got - ref)
    bad = ~(err <= bar)
    ratio = np.where(S > 0, err / np.maximum(U * S, 1e-300), 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        where = '' if detail is None else f' at {detail(i)}'
        raise AssertionError(
            f'{what}: {int(bad.sum())}/{bad.size} sampled elements outside the '
            f'bar; first{where}: got {got[i]:.9g} ref {ref[i]:.9g} |err| '
            f'{err[i]:.3g} > bar {bar[i]:.3g} (S {S[i]:.3g}, err/(uS) '
            f'{ratio[i]:.1f}); worst err/(uS) {worst:.1f}')
    return worst
