// Deformable convolution v1 for gfx950, forward and backward of the sampling: the
// conv2 of the R101-DCN Bottlenecks in stages c3-c5 (BASELINE.json config 4 as a
// frozen teacher; mmdet/models/backbones/resnet.py:171-194 with
// dcn=dict(type='DCN', deform_groups=1) from
// configs/gfl/gfl_r101_fpn_dconv_c3-c5_mstrain_2x_coco.py, which trains them).
//
// The arithmetic lives in mmcv-full (mmcv.ops.DeformConv2dPack, pinned
// 1.2.4-1.3; absent from the reference checkout), so it is restated from the
// published algorithm (Dai et al. 2017, "Deformable Convolutional Networks";
// mmcv/ops/csrc/deform_conv_cuda_kernel.cuh deformable_im2col / col2im /
// col2im_coord):
//   offset = conv3x3(x) with 2*KH*KW channels, (dy, dx) interleaved per tap
//   y[co][p] = sum_{ci,k} W[co][ci][k] * bilinear(x[ci], p*stride - pad + k*dil + offset_k(p))
//   bilinear: zero outside (-1, H) x (-1, W); neighbours outside the map are 0;
//   floorf picks the cell, also for the derivative (at an integer coordinate the
//   offset gradient is the forward difference into cell hl + 1).
// Parity status: UNPINNED against mmcv itself (no golden vectors exist for it in
// the reference); checked against independent torch-CPU restatements
// (oracle/dcn_oracle.py for the forward, tests/_dcn_ref64.py in float64 with
// autograd for the gradients).
//
// MI355X mapping, forward: the sampled patches are written once as a column
// tensor col (N, Cin*KH*KW, Pout) -- channel = ci*KH*KW + k, exactly the order
// of weight.view(Cout, Cin*KH*KW) -- and the product with the weights is the
// existing MFMA implicit GEMM as a 1x1 convolution over Cin*KH*KW channels
// (BN/ReLU folded into its epilogue; its dgrad / wgrad give d_col and d_weight).
// Thread = (n, tap, position): the sampling location and the four bilinear
// weights are computed once and reused over the channel loop; consecutive lanes
// are consecutive positions, so both the gathers (neighbouring cells) and the
// column stores are coalesced.  HBM-bound: Cin*KH*KW*4 B per output position.
//
// Backward of the sampling (fp32, no float atomics anywhere):
//   * offset gradient (deform_offset_grad_kernel): the same thread mapping and
//     channel loop as the forward; reads d_col coalesced, x through the same four
//     gathers, and keeps the two sums in registers.  One writer per element.
//   * data gradient: a scatter whose destinations depend on the offsets.  It is
//     computed as a gather so that it is bitwise reproducible: every (n, tap,
//     position, corner) ENTRY is keyed by the cell it touches (invalid corners by
//     a sentinel past the last cell), the entries are sorted by cell with a
//     stable radix sort over the cell bits only (entries are generated in id
//     order, so ties keep id order), and the sorted list is cut into fixed
//     64-entry chunks, one wave each.  A lane owns one entry: for every channel
//     it loads weight * d_col and the wave runs a segmented scan (fixed tree)
//     over the lanes of one cell.  A cell whose entries lie inside one chunk is
//     stored directly; a cell that crosses chunk boundaries leaves one partial
//     sum per chunk, which a second kernel adds in chunk order (one wave per
//     cell, lanes = channels, so the loop is wave-uniform).  The index (keys,
//     sort, segment starts) is shared by all Cin channels and built once per
//     call.  All buffers come from the caller's workspace; every launch, the
//     sort's included, goes to the stream argument.
//
// Modulated deformable convolution, DCNv2 (mmcv.ops.ModulatedDeformConv2dPack,
// conv type 'DCNv2', deform_groups = 1; Zhu et al. 2019, "Deformable ConvNets
// v2: More Deformable, Better Results"; mmcv/ops/csrc
// modulated_deform_conv_cuda_kernel.cuh).  mmcv is not in the reference
// checkout either, so the semantics are restated here:
//   om = conv_offset(x), 3*KH*KW channels (zero-initialised conv, with bias)
//   mmcv: o1, o2, mask = chunk(om, 3, 1); offset = cat(o1, o2); mask = sigmoid(mask)
//   => channels [0, 2*KH*KW) of om are the offsets, (dy, dx) interleaved per tap
//      exactly as in v1; channels [2*KH*KW, 3*KH*KW) are the mask logits, one
//      per tap
//   col[n][ci*KH*KW + t][p] = m_t(p) * (w1*x1 + w2*x2 + w3*x3 + w4*x4),
//      m = sigmoidf_(logit) (ld_math.h); the four terms, the window, the floor
//      and the zero corners are v1's, in v1's order; the mask multiplies the
//      finished sum (so om = 0 gives exactly 0.5 x v1's column tensor)
//   d_logit_t(p) = m (1 - m) * sum_ci d_col * (four-term sum)   (0 outside)
//   d_offset = v1's expression times m;  d_x = v1's scatter, corner weights times m
// Parity status: UNPINNED against mmcv; checked against tests/_mdcn_ref64.py
// (float64, autograd) built on tests/_dcn_ref64.py.
// The kernels read the offset and logit planes straight from om (no offset /
// mask tensor is materialised) and share Corners / deform_corners with v1.  The
// data gradient stores corner weight * m into the v1 workspace (same layout:
// ld_deform_col2im_workspace_bytes and ld_deform_col2im_sum serve it unchanged),
// so it stays atomic-free and bit-reproducible.  HBM-bound like v1, one more
// plane read per tap.  Measured once on an MI355X against the v1 calls of the
// same shape (R101 c3-c5 conv2 at 2 x 800 x 1344, HIP events, alternating in one
// process; tools/bench_mdcn.py -> profiles/mdcn_latency.json): im2col 0.72-0.96 x,
// offset + mask gradient 1.00-1.03 x, index + sum 1.00-1.01 x the v1 call; at
// 16 % of the HBM rate or less these calls are paced by launch and latency.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include "ld_launch.h"
#include "ld_math.h"

#include "../../include/ld_hip.h"

namespace {

__global__ __launch_bounds__(256) void deform_im2col_kernel(
    const float* __restrict__ x, const float* __restrict__ offset, int Cin, int Hin,
    int Win, int Hout, int Wout, int KH, int KW, int stride, int pad, int dil,
    float* __restrict__ col) {
  const int Pout = Hout * Wout, Pin = Hin * Win, ntaps = KH * KW;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y, n = blockIdx.z;
  if (p >= Pout) return;
  const int ho = p / Wout, wo = p - ho * Wout;
  const int kh = k / KW, kw = k - kh * KW;
  const float* off = offset + (size_t)n * 2 * ntaps * Pout;
  const float h = (float)(ho * stride - pad + kh * dil) + off[(size_t)(2 * k) * Pout + p];
  const float w = (float)(wo * stride - pad + kw * dil) + off[(size_t)(2 * k + 1) * Pout + p];
  float w1 = 0.0f, w2 = 0.0f, w3 = 0.0f, w4 = 0.0f;
  int o1 = 0, o2 = 0, o3 = 0, o4 = 0;
  if (h > -1.0f && w > -1.0f && h < (float)Hin && w < (float)Win) {
    const int hl = (int)floorf(h), wl = (int)floorf(w);
    const int hh_ = hl + 1, wh = wl + 1;
    const float lh = h - (float)hl, lw = w - (float)wl;
    const float uh = 1.0f - lh, uw = 1.0f - lw;
    const bool t = hl >= 0, b = hh_ <= Hin - 1, l = wl >= 0, r = wh <= Win - 1;
    if (t && l) { w1 = uh * uw; o1 = hl * Win + wl; }
    if (t && r) { w2 = uh * lw; o2 = hl * Win + wh; }
    if (b && l) { w3 = lh * uw; o3 = hh_ * Win + wl; }
    if (b && r) { w4 = lh * lw; o4 = hh_ * Win + wh; }
  }
  const float* xn = x + (size_t)n * Cin * Pin;
  float* cn = col + ((size_t)n * Cin * ntaps + k) * Pout + p;
  const size_t cstep = (size_t)ntaps * Pout;
#pragma unroll 4
  for (int ci = 0; ci < Cin; ++ci) {
    const float* xc = xn + (size_t)ci * Pin;
    // same order of the four terms as deformable_im2col_bilinear
    const float v = w1 * xc[o1] + w2 * xc[o2] + w3 * xc[o3] + w4 * xc[o4];
    cn[(size_t)ci * cstep] = v;
  }
}

// The four bilinear corners of one (tap, position): weights, offsets into the
// map (0 where the corner is outside: a safe address, weight 0) and validity.
struct Corners {
  float w[4];
  int o[4];
  bool ok[4];
  float lh, lw;
};

__device__ __forceinline__ Corners deform_corners(const float* __restrict__ off, int Pout,
                                                  int p, int k, int Hin, int Win, int Wout,
                                                  int KW, int stride, int pad, int dil) {
  const int ho = p / Wout, wo = p - ho * Wout;
  const int kh = k / KW, kw = k - kh * KW;
  const float h = (float)(ho * stride - pad + kh * dil) + off[(size_t)(2 * k) * Pout + p];
  const float w = (float)(wo * stride - pad + kw * dil) + off[(size_t)(2 * k + 1) * Pout + p];
  Corners c;
#pragma unroll
  for (int i = 0; i < 4; ++i) { c.w[i] = 0.0f; c.o[i] = 0; c.ok[i] = false; }
  c.lh = c.lw = 0.0f;
  if (h > -1.0f && w > -1.0f && h < (float)Hin && w < (float)Win) {
    const int hl = (int)floorf(h), wl = (int)floorf(w);
    const int hh_ = hl + 1, wh = wl + 1;
    c.lh = h - (float)hl;
    c.lw = w - (float)wl;
    const float uh = 1.0f - c.lh, uw = 1.0f - c.lw;
    const bool t = hl >= 0, b = hh_ <= Hin - 1, l = wl >= 0, r = wh <= Win - 1;
    if (t && l) { c.ok[0] = true; c.w[0] = uh * uw; c.o[0] = hl * Win + wl; }
    if (t && r) { c.ok[1] = true; c.w[1] = uh * c.lw; c.o[1] = hl * Win + wh; }
    if (b && l) { c.ok[2] = true; c.w[2] = c.lh * uw; c.o[2] = hh_ * Win + wl; }
    if (b && r) { c.ok[3] = true; c.w[3] = c.lh * c.lw; c.o[3] = hh_ * Win + wh; }
  }
  return c;
}

// d_offset[n][2k + {0,1}][p] = sum_ci d_col[n][ci*KK + k][p] * d/d{h,w} of the
// forward's four-term expression (hl, wl held fixed).  Thread = (n, tap, position).
__global__ __launch_bounds__(256) void deform_offset_grad_kernel(
    const float* __restrict__ x, const float* __restrict__ offset,
    const float* __restrict__ dcol, int Cin, int Hin, int Win, int Hout, int Wout, int KH,
    int KW, int stride, int pad, int dil, float* __restrict__ doff) {
  const int Pout = Hout * Wout, Pin = Hin * Win, ntaps = KH * KW;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y, n = blockIdx.z;
  if (p >= Pout) return;
  const Corners c = deform_corners(offset + (size_t)n * 2 * ntaps * Pout, Pout, p, k, Hin,
                                   Win, Wout, KW, stride, pad, dil);
  const float uh = 1.0f - c.lh, uw = 1.0f - c.lw;
  // d/dh: -uw x1 - lw x2 + uw x3 + lw x4;  d/dw: -uh x1 + uh x2 - lh x3 + lh x4
  const float h1 = c.ok[0] ? -uw : 0.0f, h2 = c.ok[1] ? -c.lw : 0.0f;
  const float h3 = c.ok[2] ? uw : 0.0f, h4 = c.ok[3] ? c.lw : 0.0f;
  const float v1 = c.ok[0] ? -uh : 0.0f, v2 = c.ok[1] ? uh : 0.0f;
  const float v3 = c.ok[2] ? -c.lh : 0.0f, v4 = c.ok[3] ? c.lh : 0.0f;
  const float* xn = x + (size_t)n * Cin * Pin;
  const float* gn = dcol + ((size_t)n * Cin * ntaps + k) * Pout + p;
  const size_t cstep = (size_t)ntaps * Pout;
  float ah = 0.0f, aw = 0.0f;
#pragma unroll 4
  for (int ci = 0; ci < Cin; ++ci) {
    const float* xc = xn + (size_t)ci * Pin;
    const float g = gn[(size_t)ci * cstep];
    const float x1 = xc[c.o[0]], x2 = xc[c.o[1]], x3 = xc[c.o[2]], x4 = xc[c.o[3]];
    ah += g * (h1 * x1 + h2 * x2 + h3 * x3 + h4 * x4);
    aw += g * (v1 * x1 + v2 * x2 + v3 * x3 + v4 * x4);
  }
  float* dn = doff + (size_t)n * 2 * ntaps * Pout;
  dn[(size_t)(2 * k) * Pout + p] = ah;
  dn[(size_t)(2 * k + 1) * Pout + p] = aw;
}

// ---- data gradient: index ------------------------------------------------------
// Entry e = ((n*KK + k)*Pout + p)*4 + corner.  key = n*Pin + cell of the corner,
// or NC = N*Pin (sorts last) where the corner is outside the map.
__global__ __launch_bounds__(256) void deform_entries_kernel(
    const float* __restrict__ offset, int Hin, int Win, int Hout, int Wout, int KH, int KW,
    int stride, int pad, int dil, unsigned NC, unsigned* __restrict__ keys,
    unsigned* __restrict__ vals, float* __restrict__ wq) {
  const int Pout = Hout * Wout, Pin = Hin * Win, ntaps = KH * KW;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y, n = blockIdx.z;
  if (p >= Pout) return;
  const Corners c = deform_corners(offset + (size_t)n * 2 * ntaps * Pout, Pout, p, k, Hin,
                                   Win, Wout, KW, stride, pad, dil);
  const unsigned e = (unsigned)(((size_t)n * ntaps + k) * Pout + p) * 4u;
  uint4 kk, vv;
  const unsigned base = (unsigned)n * (unsigned)Pin;
  kk.x = c.ok[0] ? base + (unsigned)c.o[0] : NC;
  kk.y = c.ok[1] ? base + (unsigned)c.o[1] : NC;
  kk.z = c.ok[2] ? base + (unsigned)c.o[2] : NC;
  kk.w = c.ok[3] ? base + (unsigned)c.o[3] : NC;
  vv.x = e; vv.y = e + 1; vv.z = e + 2; vv.w = e + 3;
  *reinterpret_cast<uint4*>(keys + e) = kk;
  *reinterpret_cast<uint4*>(vals + e) = vv;
  *reinterpret_cast<float4*>(wq + e) = make_float4(c.w[0], c.w[1], c.w[2], c.w[3]);
}

// start[c] = first sorted entry whose key is >= c, for c in [0, NC]; start[NC] =
// the number of valid entries.  One bounded binary search per cell.
__global__ __launch_bounds__(256) void deform_segments_kernel(
    const unsigned* __restrict__ skeys, unsigned E, unsigned NC,
    unsigned* __restrict__ start) {
  const unsigned c = blockIdx.x * 256u + threadIdx.x;
  if (c > NC) return;
  unsigned lo = 0, hi = E;
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo) >> 1);
    if (skeys[mid] < c) lo = mid + 1; else hi = mid;
  }
  start[c] = lo;
}

// ---- data gradient: sum --------------------------------------------------------
// One wave per 64-entry chunk of the sorted list, blockIdx.y = a block of `cb`
// channels.  Lane = entry; per channel a segmented inclusive scan over the lanes
// of one cell (fixed tree: the order of the additions depends on the index alone).
__global__ __launch_bounds__(256) void deform_col2im_chunks_kernel(
    const unsigned* __restrict__ skeys, const unsigned* __restrict__ svals,
    const float* __restrict__ wq, const unsigned* __restrict__ start,
    const float* __restrict__ dcol, unsigned NC, int Cin, int Pin, int Pout, int ntaps,
    int cb, float* __restrict__ partial, float* __restrict__ dx) {
  const int lane = threadIdx.x & 63;
  const unsigned g = blockIdx.x * 4u + (threadIdx.x >> 6);
  const unsigned nvalid = start[NC];
  if ((size_t)g * 64 >= nvalid) return;  // wave-uniform
  const unsigned idx = g * 64u + (unsigned)lane;
  const bool valid = idx < nvalid;
  const unsigned cell = valid ? skeys[idx] : 0xffffffffu;
  const unsigned e = valid ? svals[idx] : 0u;
  const float w = valid ? wq[e] : 0.0f;
  const unsigned q = e >> 2;
  const unsigned pp = q % (unsigned)Pout, nk = q / (unsigned)Pout;
  const unsigned k = nk % (unsigned)ntaps, n = nk / (unsigned)ntaps;
  const size_t cstep = (size_t)ntaps * Pout;
  const float* src = dcol + ((size_t)n * Cin * ntaps + k) * Pout + pp;
  // segment structure of the chunk
  const unsigned prev = __shfl_up(cell, 1);
  const bool head = lane == 0 || prev != cell;
  const unsigned long long hb = __ballot(head);
  const unsigned long long upto = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
  const int hl = 63 - __clzll((long long)(hb & upto));  // lane 0 is always a head
  const int d = lane - hl;
  const bool tail = lane == 63 || ((hb >> (lane + 1)) & 1ull);
  const bool from_prev = hl == 0 && g > 0 && skeys[g * 64u - 1u] == cell;
  const bool to_next = lane == 63 && idx + 1 < nvalid && skeys[idx + 1] == cell;
  const bool store = valid && tail;
  float* dst = dx;
  size_t dstep = 0;
  if (store) {
    if (!from_prev && !to_next) {  // the whole cell lies in this chunk
      const unsigned cn = cell / (unsigned)Pin, cc = cell - cn * (unsigned)Pin;
      dst = dx + (size_t)cn * Cin * Pin + cc;
      dstep = (size_t)Pin;
    } else {  // slot 0: the segment of lane 0, slot 1: another one that runs on
      dst = partial + ((size_t)g * 2 + (hl == 0 ? 0 : 1)) * Cin;
      dstep = 1;
    }
  }
  const int c0 = blockIdx.y * cb;
  const int c1 = min(c0 + cb, Cin);
#pragma unroll 4
  for (int ci = c0; ci < c1; ++ci) {
    float v = w * src[(size_t)ci * cstep];
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const float t = __shfl_up(v, s);
      if (s <= d) v += t;
    }
    if (store) dst[(size_t)ci * dstep] = v;
  }
}

// Cells whose entries cross chunk boundaries: add their per-chunk partial sums in
// chunk order.  One wave per cell, lane = channel (the loop is wave-uniform).
__global__ __launch_bounds__(256) void deform_col2im_fixup_kernel(
    const unsigned* __restrict__ start, const float* __restrict__ partial, unsigned NC,
    int Cin, int Pin, float* __restrict__ dx) {
  const unsigned c = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (c >= NC) return;
  const unsigned s = start[c], t = start[c + 1];
  if (t <= s) return;
  const unsigned g0 = s >> 6, g1 = (t - 1) >> 6;
  if (g0 == g1) return;  // stored by the chunk kernel
  const int ci = blockIdx.y * 64 + (threadIdx.x & 63);
  if (ci >= Cin) return;
  float acc = partial[((size_t)g0 * 2 + ((s & 63u) ? 1 : 0)) * Cin + ci];
  for (unsigned g = g0 + 1; g <= g1; ++g) acc += partial[(size_t)g * 2 * Cin + ci];
  const unsigned cn = c / (unsigned)Pin, cc = c - cn * (unsigned)Pin;
  dx[((size_t)cn * Cin + ci) * Pin + cc] = acc;
}

// Workspace of the data gradient: [keys | sorted keys | entry ids | sorted ids |
// corner weights | segment starts | per-chunk partials | radix-sort scratch].
struct Col2imWs {
  size_t keys, skeys, vals, svals, wq, start, partial, sort, total, sort_bytes;
  unsigned E, NC;
  int Hout, Wout, end_bit;
};

inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }

// 0 = ok.  `with_sort`: also size the radix-sort scratch (asks hipcub; needs a device).
int col2im_layout(int N, int Cin, int Hin, int Win, int KH, int KW, int stride, int pad,
                  int dilation, bool with_sort, Col2imWs* L) {
  if (N < 1 || Cin < 1 || Hin < 1 || Win < 1 || KH < 1 || KW < 1 || stride < 1 ||
      dilation < 1 || pad < 0)
    return LD_EINVAL;
  const long long Hout = ((long long)Hin + 2 * pad - (long long)dilation * (KH - 1) - 1) / stride + 1;
  const long long Wout = ((long long)Win + 2 * pad - (long long)dilation * (KW - 1) - 1) / stride + 1;
  if (Hout < 1 || Wout < 1) return LD_EINVAL;
  const long long E = (long long)N * KH * KW * Hout * Wout * 4;
  const long long NC = (long long)N * Hin * Win;
  const long long ncol = (long long)N * Cin * KH * KW * Hout * Wout;
  if (E >= (1ll << 31) || NC >= (1ll << 31) - 1 || ncol >= (1ll << 40) ||
      (long long)N * Cin * Hin * Win >= (1ll << 40))
    return LD_EINVAL;
  L->E = (unsigned)E;
  L->NC = (unsigned)NC;
  L->Hout = (int)Hout;
  L->Wout = (int)Wout;
  int bits = 1;
  while (bits < 32 && (NC >> bits) != 0) ++bits;  // keys are <= NC
  L->end_bit = bits;
  const size_t nchunks = ((size_t)E + 63) / 64;
  size_t off = 0;
  L->keys = off; off += up256((size_t)E * 4);
  L->skeys = off; off += up256((size_t)E * 4);
  L->vals = off; off += up256((size_t)E * 4);
  L->svals = off; off += up256((size_t)E * 4);
  L->wq = off; off += up256((size_t)E * 4);
  L->start = off; off += up256(((size_t)NC + 1) * 4);
  L->partial = off; off += up256(nchunks * 2 * (size_t)Cin * 4);
  L->sort = off;
  L->sort_bytes = 0;
  if (with_sort) {
    size_t bytes = 0;
    const hipError_t rc = hipcub::DeviceRadixSort::SortPairs(
        nullptr, bytes, (const unsigned*)nullptr, (unsigned*)nullptr,
        (const unsigned*)nullptr, (unsigned*)nullptr, (unsigned)E, 0, bits,
        (hipStream_t) nullptr);
    if (rc != hipSuccess) return (int)rc;
    L->sort_bytes = up256(bytes ? bytes : 1);
  }
  L->total = off + L->sort_bytes;
  return 0;
}

// ---- DCNv2: the same three pieces with the modulation mask --------------------
// om (N, 3*KK, Pout): planes [0, 2*KK) the offsets as v1's, planes [2*KK, 3*KK)
// the mask logits.  deform_corners only needs the image's first offset plane, so
// it takes om's image base as it is.
__device__ __forceinline__ float mdeform_mask(const float* __restrict__ omn, int Pout, int p,
                                              int k, int ntaps) {
  return ld::sigmoidf_(omn[(size_t)(2 * ntaps + k) * Pout + p]);
}

// The four-term expression c1 x1 + c2 x2 + c3 x3 + c4 x4 with the rounding the v1
// kernels have as compiled (-ffp-contract=fast: c2 x2 rounded, then terms 1, 3, 4
// by fused multiply-add), spelled out so that the bits depend neither on how a
// channel loop is unrolled nor on which terms a vectoriser pairs: with a mask of
// exactly 0.5 every DCNv2 result is then exactly half of v1's.
__device__ __forceinline__ float four_terms(float c1, float x1, float c2, float x2, float c3,
                                            float x3, float c4, float x4) {
  return fmaf(c4, x4, fmaf(c3, x3, fmaf(c1, x1, c2 * x2)));
}

// Thread = (n, tap, position) as deform_im2col_kernel; col = m * (four-term sum).
__global__ __launch_bounds__(256) void mdeform_im2col_kernel(
    const float* __restrict__ x, const float* __restrict__ om, int Cin, int Hin, int Win,
    int Hout, int Wout, int KH, int KW, int stride, int pad, int dil,
    float* __restrict__ col) {
  const int Pout = Hout * Wout, Pin = Hin * Win, ntaps = KH * KW;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y, n = blockIdx.z;
  if (p >= Pout) return;
  const float* omn = om + (size_t)n * 3 * ntaps * Pout;
  const Corners c = deform_corners(omn, Pout, p, k, Hin, Win, Wout, KW, stride, pad, dil);
  const float m = mdeform_mask(omn, Pout, p, k, ntaps);
  const float w1 = c.w[0], w2 = c.w[1], w3 = c.w[2], w4 = c.w[3];
  const int o1 = c.o[0], o2 = c.o[1], o3 = c.o[2], o4 = c.o[3];
  const float* xn = x + (size_t)n * Cin * Pin;
  float* cn = col + ((size_t)n * Cin * ntaps + k) * Pout + p;
  const size_t cstep = (size_t)ntaps * Pout;
#pragma unroll 4
  for (int ci = 0; ci < Cin; ++ci) {
    const float* xc = xn + (size_t)ci * Pin;
    // v1's expression, then the mask on the finished sum
    const float v = four_terms(w1, xc[o1], w2, xc[o2], w3, xc[o3], w4, xc[o4]);
    cn[(size_t)ci * cstep] = m * v;
  }
}

// d_om: planes 2k, 2k + 1 = m * v1's two offset sums; plane 2*KK + k = m (1 - m) *
// sum_ci d_col * (four-term sum).  The three sums stay in registers over the
// channel loop; the mask factors are applied at the store.  Thread = (n, tap,
// position) writes its three elements: one writer each, every element written.
__global__ __launch_bounds__(256) void mdeform_offset_mask_grad_kernel(
    const float* __restrict__ x, const float* __restrict__ om,
    const float* __restrict__ dcol, int Cin, int Hin, int Win, int Hout, int Wout, int KH,
    int KW, int stride, int pad, int dil, float* __restrict__ dom) {
  const int Pout = Hout * Wout, Pin = Hin * Win, ntaps = KH * KW;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y, n = blockIdx.z;
  if (p >= Pout) return;
  const float* omn = om + (size_t)n * 3 * ntaps * Pout;
  const Corners c = deform_corners(omn, Pout, p, k, Hin, Win, Wout, KW, stride, pad, dil);
  const float m = mdeform_mask(omn, Pout, p, k, ntaps);
  const float uh = 1.0f - c.lh, uw = 1.0f - c.lw;
  const float h1 = c.ok[0] ? -uw : 0.0f, h2 = c.ok[1] ? -c.lw : 0.0f;
  const float h3 = c.ok[2] ? uw : 0.0f, h4 = c.ok[3] ? c.lw : 0.0f;
  const float v1 = c.ok[0] ? -uh : 0.0f, v2 = c.ok[1] ? uh : 0.0f;
  const float v3 = c.ok[2] ? -c.lh : 0.0f, v4 = c.ok[3] ? c.lh : 0.0f;
  const float* xn = x + (size_t)n * Cin * Pin;
  const float* gn = dcol + ((size_t)n * Cin * ntaps + k) * Pout + p;
  const size_t cstep = (size_t)ntaps * Pout;
  float ah = 0.0f, aw = 0.0f, am = 0.0f;
#pragma unroll 4
  for (int ci = 0; ci < Cin; ++ci) {
    const float* xc = xn + (size_t)ci * Pin;
    const float g = gn[(size_t)ci * cstep];
    const float x1 = xc[c.o[0]], x2 = xc[c.o[1]], x3 = xc[c.o[2]], x4 = xc[c.o[3]];
    ah = fmaf(g, four_terms(h1, x1, h2, x2, h3, x3, h4, x4), ah);
    aw = fmaf(g, four_terms(v1, x1, v2, x2, v3, x3, v4, x4), aw);
    am = fmaf(g, four_terms(c.w[0], x1, c.w[1], x2, c.w[2], x3, c.w[3], x4), am);
  }
  float* dn = dom + (size_t)n * 3 * ntaps * Pout;
  dn[(size_t)(2 * k) * Pout + p] = m * ah;
  dn[(size_t)(2 * k + 1) * Pout + p] = m * aw;
  dn[(size_t)(2 * ntaps + k) * Pout + p] = m * (1.0f - m) * am;
}

// deform_entries_kernel with the corner weights stored as weight * m: keys, entry
// ids and the workspace layout are v1's, so the sort, the segments and
// ld_deform_col2im_sum run on it unchanged.
__global__ __launch_bounds__(256) void mdeform_entries_kernel(
    const float* __restrict__ om, int Hin, int Win, int Hout, int Wout, int KH, int KW,
    int stride, int pad, int dil, unsigned NC, unsigned* __restrict__ keys,
    unsigned* __restrict__ vals, float* __restrict__ wq) {
  const int Pout = Hout * Wout, Pin = Hin * Win, ntaps = KH * KW;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y, n = blockIdx.z;
  if (p >= Pout) return;
  const float* omn = om + (size_t)n * 3 * ntaps * Pout;
  const Corners c = deform_corners(omn, Pout, p, k, Hin, Win, Wout, KW, stride, pad, dil);
  const float m = mdeform_mask(omn, Pout, p, k, ntaps);
  const unsigned e = (unsigned)(((size_t)n * ntaps + k) * Pout + p) * 4u;
  uint4 kk, vv;
  const unsigned base = (unsigned)n * (unsigned)Pin;
  kk.x = c.ok[0] ? base + (unsigned)c.o[0] : NC;
  kk.y = c.ok[1] ? base + (unsigned)c.o[1] : NC;
  kk.z = c.ok[2] ? base + (unsigned)c.o[2] : NC;
  kk.w = c.ok[3] ? base + (unsigned)c.o[3] : NC;
  vv.x = e; vv.y = e + 1; vv.z = e + 2; vv.w = e + 3;
  *reinterpret_cast<uint4*>(keys + e) = kk;
  *reinterpret_cast<uint4*>(vals + e) = vv;
  *reinterpret_cast<float4*>(wq + e) =
      make_float4(c.w[0] * m, c.w[1] * m, c.w[2] * m, c.w[3] * m);
}

}  // namespace

extern "C" int ld_deform_im2col(const float* x, const float* offset, int N, int Cin,
                                int Hin, int Win, int KH, int KW, int stride, int pad,
                                int dilation, float* col, ld_stream_t stream) {
  if (!x || !offset || !col || N < 1 || Cin < 1 || Hin < 1 || Win < 1 || KH < 1 ||
      KW < 1 || stride < 1 || dilation < 1 || pad < 0)
    return LD_EINVAL;
  const int Hout = (Hin + 2 * pad - dilation * (KH - 1) - 1) / stride + 1;
  const int Wout = (Win + 2 * pad - dilation * (KW - 1) - 1) / stride + 1;
  if (Hout < 1 || Wout < 1) return LD_EINVAL;
  const int Pout = Hout * Wout;
  LD_LAUNCH(deform_im2col_kernel, dim3((Pout + 255) / 256, KH * KW, N),
                     dim3(256), 0, (hipStream_t)stream, x, offset, Cin, Hin, Win, Hout,
                     Wout, KH, KW, stride, pad, dilation, col);
  return (int)hipGetLastError();
}

extern "C" int ld_deform_offset_grad(const float* x, const float* offset,
                                     const float* d_col, int N, int Cin, int Hin, int Win,
                                     int KH, int KW, int stride, int pad, int dilation,
                                     float* d_offset, ld_stream_t stream) {
  Col2imWs L;
  if (!x || !offset || !d_col || !d_offset ||
      col2im_layout(N, Cin, Hin, Win, KH, KW, stride, pad, dilation, false, &L) != 0)
    return LD_EINVAL;
  const int Pout = L.Hout * L.Wout;
  LD_LAUNCH(deform_offset_grad_kernel, dim3((Pout + 255) / 256, KH * KW, N), dim3(256), 0,
            (hipStream_t)stream, x, offset, d_col, Cin, Hin, Win, L.Hout, L.Wout, KH, KW,
            stride, pad, dilation, d_offset);
  return (int)hipGetLastError();
}

extern "C" size_t ld_deform_col2im_workspace_bytes(int N, int Cin, int Hin, int Win, int KH,
                                                   int KW, int stride, int pad,
                                                   int dilation) {
  Col2imWs L;
  if (col2im_layout(N, Cin, Hin, Win, KH, KW, stride, pad, dilation, true, &L) != 0)
    return 0;
  return L.total;
}

extern "C" int ld_deform_col2im_index(const float* offset, int N, int Cin, int Hin, int Win,
                                      int KH, int KW, int stride, int pad, int dilation,
                                      void* workspace, size_t workspace_bytes,
                                      ld_stream_t stream) {
  Col2imWs L;
  if (!offset || !workspace) return LD_EINVAL;
  const int rc = col2im_layout(N, Cin, Hin, Win, KH, KW, stride, pad, dilation, true, &L);
  if (rc != 0) return rc > 0 ? rc : LD_EINVAL;
  if (workspace_bytes < L.total) return LD_ENOSPACE;
  char* ws = (char*)workspace;
  unsigned* keys = (unsigned*)(ws + L.keys);
  unsigned* skeys = (unsigned*)(ws + L.skeys);
  unsigned* vals = (unsigned*)(ws + L.vals);
  unsigned* svals = (unsigned*)(ws + L.svals);
  const int Pout = L.Hout * L.Wout;
  hipStream_t st = (hipStream_t)stream;
  LD_LAUNCH(deform_entries_kernel, dim3((Pout + 255) / 256, KH * KW, N), dim3(256), 0, st,
            offset, Hin, Win, L.Hout, L.Wout, KH, KW, stride, pad, dilation, L.NC, keys, vals,
            (float*)(ws + L.wq));
  size_t bytes = L.sort_bytes;
  // stable: entries of one cell stay in entry-id order
  const hipError_t e = hipcub::DeviceRadixSort::SortPairs(
      (void*)(ws + L.sort), bytes, (const unsigned*)keys, skeys, (const unsigned*)vals, svals,
      L.E, 0, L.end_bit, st);
  if (e != hipSuccess) return (int)e;
  LD_LAUNCH(deform_segments_kernel, dim3(L.NC / 256 + 1), dim3(256), 0, st,
            (const unsigned*)skeys, L.E, L.NC, (unsigned*)(ws + L.start));
  return (int)hipGetLastError();
}

extern "C" int ld_deform_col2im_sum(const float* d_col, int N, int Cin, int Hin, int Win,
                                    int KH, int KW, int stride, int pad, int dilation,
                                    void* workspace, size_t workspace_bytes, float* d_x,
                                    ld_stream_t stream) {
  Col2imWs L;
  if (!d_col || !workspace || !d_x ||
      col2im_layout(N, Cin, Hin, Win, KH, KW, stride, pad, dilation, false, &L) != 0)
    return LD_EINVAL;
  if (workspace_bytes < L.total) return LD_ENOSPACE;  // without the sort scratch
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const int Pin = Hin * Win, Pout = L.Hout * L.Wout;
  const hipError_t e = ldrec::memset_async(d_x, 0, (size_t)N * Cin * Pin * 4, st);
  if (e != hipSuccess) return (int)e;
  const unsigned nchunks = (L.E + 63u) / 64u;
  const int cb = 32;
  LD_LAUNCH(deform_col2im_chunks_kernel, dim3((nchunks + 3) / 4, (Cin + cb - 1) / cb),
            dim3(256), 0, st, (const unsigned*)(ws + L.skeys), (const unsigned*)(ws + L.svals),
            (const float*)(ws + L.wq), (const unsigned*)(ws + L.start), d_col, L.NC, Cin, Pin,
            Pout, KH * KW, cb, (float*)(ws + L.partial), d_x);
  LD_LAUNCH(deform_col2im_fixup_kernel, dim3((L.NC + 3) / 4, (Cin + 63) / 64), dim3(256), 0,
            st, (const unsigned*)(ws + L.start), (const float*)(ws + L.partial), L.NC, Cin,
            Pin, d_x);
  return (int)hipGetLastError();
}

// ---- DCNv2 entry points ----------------------------------------------------------
extern "C" int ld_mdeform_im2col(const float* x, const float* om, int N, int Cin, int Hin,
                                 int Win, int KH, int KW, int stride, int pad, int dilation,
                                 float* col, ld_stream_t stream) {
  Col2imWs L;
  if (!x || !om || !col ||
      col2im_layout(N, Cin, Hin, Win, KH, KW, stride, pad, dilation, false, &L) != 0)
    return LD_EINVAL;
  const int Pout = L.Hout * L.Wout;
  LD_LAUNCH(mdeform_im2col_kernel, dim3((Pout + 255) / 256, KH * KW, N), dim3(256), 0,
            (hipStream_t)stream, x, om, Cin, Hin, Win, L.Hout, L.Wout, KH, KW, stride, pad,
            dilation, col);
  return (int)hipGetLastError();
}

extern "C" int ld_mdeform_offset_mask_grad(const float* x, const float* om,
                                           const float* d_col, int N, int Cin, int Hin,
                                           int Win, int KH, int KW, int stride, int pad,
                                           int dilation, float* d_om, ld_stream_t stream) {
  Col2imWs L;
  if (!x || !om || !d_col || !d_om ||
      col2im_layout(N, Cin, Hin, Win, KH, KW, stride, pad, dilation, false, &L) != 0)
    return LD_EINVAL;
  const int Pout = L.Hout * L.Wout;
  LD_LAUNCH(mdeform_offset_mask_grad_kernel, dim3((Pout + 255) / 256, KH * KW, N),
            dim3(256), 0, (hipStream_t)stream, x, om, d_col, Cin, Hin, Win, L.Hout, L.Wout,
            KH, KW, stride, pad, dilation, d_om);
  return (int)hipGetLastError();
}

// The workspace is ld_deform_col2im_workspace_bytes'; ld_deform_col2im_sum reads it.
extern "C" int ld_mdeform_col2im_index(const float* om, int N, int Cin, int Hin, int Win,
                                       int KH, int KW, int stride, int pad, int dilation,
                                       void* workspace, size_t workspace_bytes,
                                       ld_stream_t stream) {
  Col2imWs L;
  if (!om || !workspace) return LD_EINVAL;
  const int rc = col2im_layout(N, Cin, Hin, Win, KH, KW, stride, pad, dilation, true, &L);
  if (rc != 0) return rc > 0 ? rc : LD_EINVAL;
  if (workspace_bytes < L.total) return LD_ENOSPACE;
  char* ws = (char*)workspace;
  unsigned* keys = (unsigned*)(ws + L.keys);
  unsigned* skeys = (unsigned*)(ws + L.skeys);
  unsigned* vals = (unsigned*)(ws + L.vals);
  unsigned* svals = (unsigned*)(ws + L.svals);
  const int Pout = L.Hout * L.Wout;
  hipStream_t st = (hipStream_t)stream;
  LD_LAUNCH(mdeform_entries_kernel, dim3((Pout + 255) / 256, KH * KW, N), dim3(256), 0, st,
            om, Hin, Win, L.Hout, L.Wout, KH, KW, stride, pad, dilation, L.NC, keys, vals,
            (float*)(ws + L.wq));
  size_t bytes = L.sort_bytes;
  // stable: entries of one cell stay in entry-id order
  const hipError_t e = hipcub::DeviceRadixSort::SortPairs(
      (void*)(ws + L.sort), bytes, (const unsigned*)keys, skeys, (const unsigned*)vals, svals,
      L.E, 0, L.end_bit, st);
  if (e != hipSuccess) return (int)e;
  LD_LAUNCH(deform_segments_kernel, dim3(L.NC / 256 + 1), dim3(256), 0, st,
            (const unsigned*)skeys, L.E, L.NC, (unsigned*)(ws + L.start));
  return (int)hipGetLastError();
}
