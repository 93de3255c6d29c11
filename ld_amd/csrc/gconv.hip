// Grouped convolution (forward, data gradient, weight gradient) for gfx950 --
// the 3x3 conv2 of ResNeXt's
// Bottleneck (mmdet/models/backbones/resnext.py:49-61: groups = 32, width =
// floor(planes * base_width / 64) * groups, i.e. 4 / 8 / 16 / 32 channels per
// group in the four stages of ResNeXt-101 32x4d), the frozen X-101 teacher of
// BASELINE config 5.  With K = 1 it is also the grouped GEMM behind a grouped
// deformable conv (columns of ld_deform_im2col: Cin*9 rows, groups of cg*9).
//
// Roofline: a grouped conv does cg * 9 * 2 flop per 8 bytes it must move (one
// fp32 in, one out per channel and position) = 9 ... 72 flop/B for cg = 4 ... 32,
// every layer of the net is 1.24 GFLOP on 17-138 MB of activations: HBM- /
// L1-bound work, NOT an MFMA GEMM (a 32-wide MFMA tile would be 8x ... 1x
// block-diagonal zeros).  So: VALU FMAs with the weights as SCALAR operands.
//   thread = one output position of one group: acc[CG] in registers;
//   the 64 lanes of a wavefront read 64 consecutive positions of each input
//     channel and tap (coalesced; the 9 taps of a channel re-hit the same
//     lines in L1);
//   the group's weights sit in the image [g][ci][tap][co]: for a (ci, tap) the
//     CG out-channel weights are CG consecutive dwords at a wave-uniform
//     address -> s_load_dwordx4/x8/x16 + v_fma with an SGPR operand, no LDS.
// Epilogue as the dense convs': y = relu(scale[c] * acc + shift[c]).
//
// Data gradient (gconv_dgrad_kernel): the same design turned round, as a GATHER:
//   thread = one INPUT position of one group and one chunk of CIC <= 32 of the
//     group's input channels: acc[CIC] in registers (cin_g reaches 288 behind a
//     grouped DCN, so the chunk index is a grid dimension);
//   for every out channel and tap it reads the one dy that this tap maps to the
//     position (stride 2: the taps of the wrong parity contribute nothing, a bit
//     test, no division) and FMAs it with CIC wave-uniform weights from the
//     image [g][chunk][co][tap][CIC] (zero-padded past cin_g);
//   no scatter, no atomics: bitwise reproducible.  dx = addend + acc optional.
//   Stride 1 moves the bytes and does the flops of the forward of that shape.
//
// Weight gradient (gconv_wgrad_kernel + gconv_wgrad_reduce_kernel): dw is small
// (Cout * cin_g * KK) and the reduction over N * Pout long: one pass over x and
// dy, bound by L1 / HBM.
//   the positions of an image are cut into slabs of GW_SLAB;
//   wave = (slab, group, one input channel ci, a chunk of COC <= 8 out channels):
//     lanes run over the slab's positions, acc[COC][KK] per lane (per position
//     KK x loads + COC dy loads feed COC * KK FMAs; the 4 waves of a block take 4
//     neighbouring ci and share the dy lines in L1);
//   at the end of the slab a butterfly over the 64 lanes (fixed order) and one
//     partial per (slab, element) into the caller's workspace, laid out as dw;
//   the second launch sums the slabs in slab order and stores or accumulates.
//   No float atomics anywhere: two runs are bit-identical.
#include <hip/hip_runtime.h>

#include "ld_launch.h"

#include "../../include/ld_hip.h"

namespace {

// w (Cout, cin_g, KK) -> image (G, cin_g, KK, CG), CG = Cout / G
__global__ __launch_bounds__(256) void gconv_weight_image_kernel(
    const float* __restrict__ w, float* __restrict__ img, int G, int CG, int cin_g,
    int KK) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int total = G * CG * cin_g * KK;
  if (i >= total) return;
  // i indexes the image: ((g * cin_g + ci) * KK + t) * CG + co
  const int co = i % CG;
  int r = i / CG;
  const int t = r % KK;
  r /= KK;
  const int ci = r % cin_g, g = r / cin_g;
  img[i] = w[((size_t)(g * CG + co) * cin_g + ci) * KK + t];
}

template <int CG, int K>
__global__ __launch_bounds__(256) void gconv_forward_kernel(
    const float* __restrict__ x, const float* __restrict__ wimg, float* __restrict__ y,
    int Cin, int Cout, int cin_g, int stride, int pad, int Hin, int Win, int Hout,
    int Wout, const float* __restrict__ scale, const float* __restrict__ shift,
    int relu) {
  constexpr int KK = K * K;
  const int g = blockIdx.y, n = blockIdx.z;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int Pout = Hout * Wout, Pin = Hin * Win;
  const bool live = p < Pout;
  const int ho = live ? p / Wout : 0, wo = live ? p - (p / Wout) * Wout : 0;
  int off[KK];
  bool ok[KK];
#pragma unroll
  for (int kh = 0; kh < K; ++kh)
#pragma unroll
    for (int kw = 0; kw < K; ++kw) {
      const int hi = ho * stride - pad + kh, wi = wo * stride - pad + kw;
      ok[kh * K + kw] = live && hi >= 0 && hi < Hin && wi >= 0 && wi < Win;
      off[kh * K + kw] = hi * Win + wi;
    }
  float acc[CG];
#pragma unroll
  for (int c = 0; c < CG; ++c) acc[c] = 0.0f;
  const float* xg = x + ((size_t)n * Cin + (size_t)g * cin_g) * Pin;
  const float* wg = wimg + (size_t)g * cin_g * KK * CG;  // wave-uniform
  for (int ci = 0; ci < cin_g; ++ci) {
    const float* xc = xg + (size_t)ci * Pin;
    float xv[KK];
#pragma unroll
    for (int t = 0; t < KK; ++t) xv[t] = ok[t] ? xc[off[t]] : 0.0f;
#pragma unroll
    for (int t = 0; t < KK; ++t) {
      const float* wr = wg + ((size_t)ci * KK + t) * CG;
#pragma unroll
      for (int c = 0; c < CG; ++c) acc[c] = fmaf(wr[c], xv[t], acc[c]);
    }
  }
  if (!live) return;
  float* yg = y + ((size_t)n * Cout + (size_t)g * CG) * Pout + p;
#pragma unroll
  for (int c = 0; c < CG; ++c) {
    float v = acc[c];
    if (scale) v = v * scale[g * CG + c] + shift[g * CG + c];
    if (relu) v = fmaxf(v, 0.0f);
    yg[(size_t)c * Pout] = v;
  }
}

template <int K>
int launch_gconv(int CG, dim3 grid, hipStream_t st, const float* x, const float* wimg,
                 float* y, int Cin, int Cout, int cin_g, int stride, int pad, int Hin,
                 int Win, int Hout, int Wout, const float* scale, const float* shift,
                 int relu) {
#define LD_GC(C)                                                                      \
  LD_LAUNCH((gconv_forward_kernel<C, K>), grid, dim3(256), 0, st, x, wimg, y, \
                     Cin, Cout, cin_g, stride, pad, Hin, Win, Hout, Wout, scale, shift, \
                     relu)
  switch (CG) {
    case 4: LD_GC(4); break;
    case 8: LD_GC(8); break;
    case 16: LD_GC(16); break;
    case 32: LD_GC(32); break;
    default: return LD_EUNSUPPORTED;
  }
#undef LD_GC
  return (int)hipGetLastError();
}

// w (Cout, cin_g, KK) -> image (G, nchunk, CG, KK, CIC) of the data gradient:
// channel ch * CIC + c of a group, zero where that is past cin_g
__global__ __launch_bounds__(256) void gconv_weight_image_bwd_kernel(
    const float* __restrict__ w, float* __restrict__ img, int G, int CG, int cin_g,
    int KK, int CIC, int nchunk) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int total = G * nchunk * CG * KK * CIC;
  if (i >= total) return;
  const int c = i % CIC;
  int r = i / CIC;
  const int t = r % KK;
  r /= KK;
  const int co = r % CG;
  r /= CG;
  const int ch = r % nchunk, g = r / nchunk;
  const int ci = ch * CIC + c;
  img[i] = ci < cin_g ? w[((size_t)(g * CG + co) * cin_g + ci) * KK + t] : 0.0f;
}

// channels per accumulator chunk of the data gradient
__host__ __device__ inline int gconv_cic(int cin_g) {
  return cin_g > 16 ? 32 : cin_g > 8 ? 16 : cin_g > 4 ? 8 : 4;
}

template <int CIC, int K>
__global__ __launch_bounds__(256) void gconv_dgrad_kernel(
    const float* __restrict__ dy, const float* __restrict__ wimg,
    const float* __restrict__ addend, float* __restrict__ dx, int Cin, int Cout, int CG,
    int cin_g, int nchunk, int stride, int pad, int Hin, int Win, int Hout, int Wout) {
  constexpr int KK = K * K;
  const int g = blockIdx.y / nchunk, ch = blockIdx.y - g * nchunk, n = blockIdx.z;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int Pout = Hout * Wout, Pin = Hin * Win;
  const bool live = p < Pin;
  const int hi = live ? p / Win : 0, wi = live ? p - (p / Win) * Win : 0;
  int off[KK];
  bool ok[KK];
#pragma unroll
  for (int kh = 0; kh < K; ++kh)
#pragma unroll
    for (int kw = 0; kw < K; ++kw) {
      // ho * stride - pad + kh = hi; stride 2: only the taps of the right parity
      const int th = hi + pad - kh, tw = wi + pad - kw;
      const bool par = stride == 1 || (((th | tw) & 1) == 0);
      const int ho = stride == 1 ? th : th >> 1, wo = stride == 1 ? tw : tw >> 1;
      ok[kh * K + kw] =
          live && par && th >= 0 && tw >= 0 && ho < Hout && wo < Wout;
      off[kh * K + kw] = ho * Wout + wo;
    }
  float acc[CIC];
#pragma unroll
  for (int c = 0; c < CIC; ++c) acc[c] = 0.0f;
  const float* dyg = dy + ((size_t)n * Cout + (size_t)g * CG) * Pout;
  const float* wg =
      wimg + ((size_t)g * nchunk + ch) * CG * KK * CIC;  // wave-uniform
  for (int co = 0; co < CG; ++co) {
    const float* dc = dyg + (size_t)co * Pout;
    float dv[KK];
#pragma unroll
    for (int t = 0; t < KK; ++t) dv[t] = ok[t] ? dc[off[t]] : 0.0f;
#pragma unroll
    for (int t = 0; t < KK; ++t) {
      const float* wr = wg + ((size_t)co * KK + t) * CIC;
#pragma unroll
      for (int c = 0; c < CIC; ++c) acc[c] = fmaf(wr[c], dv[t], acc[c]);
    }
  }
  if (!live) return;
  const int ci0 = ch * CIC;
  const size_t base = ((size_t)n * Cin + (size_t)g * cin_g + ci0) * Pin + p;
#pragma unroll
  for (int c = 0; c < CIC; ++c) {
    if (ci0 + c >= cin_g) break;
    const size_t o = base + (size_t)c * Pin;
    dx[o] = addend ? addend[o] + acc[c] : acc[c];
  }
}

constexpr int GW_SLAB = 4096;  // positions of one image per weight-gradient slab

template <int COC, int K>
__global__ __launch_bounds__(256) void gconv_wgrad_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ part,
    int Cin, int Cout, int CG, int cin_g, int stride, int pad, int Hin, int Win, int Hout,
    int Wout, int slabs_img) {
  constexpr int KK = K * K;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slab = blockIdx.x, n = slab / slabs_img, sl = slab - n * slabs_img;
  // blockIdx.y = (g * quads + q) * cochunks + cc
  const int cochunks = CG / COC, quads = (cin_g + 3) / 4;
  int r = blockIdx.y;
  const int cc = r % cochunks;
  r /= cochunks;
  const int q = r % quads, g = r / quads;
  const int ci = q * 4 + wave;
  if (ci >= cin_g) return;  // wave-uniform; no barrier below
  const int Pout = Hout * Wout, Pin = Hin * Win;
  const int p_end = min(Pout, (sl + 1) * GW_SLAB);
  const float* xc = x + ((size_t)n * Cin + (size_t)g * cin_g + ci) * Pin;
  const float* dyc = dy + ((size_t)n * Cout + (size_t)g * CG + cc * COC) * Pout;
  float acc[COC][KK];
#pragma unroll
  for (int c = 0; c < COC; ++c)
#pragma unroll
    for (int t = 0; t < KK; ++t) acc[c][t] = 0.0f;
  for (int p = sl * GW_SLAB + lane; p < p_end; p += 64) {
    const int ho = p / Wout, wo = p - ho * Wout;
    float xv[KK];
#pragma unroll
    for (int kh = 0; kh < K; ++kh)
#pragma unroll
      for (int kw = 0; kw < K; ++kw) {
        const int hi = ho * stride - pad + kh, wi = wo * stride - pad + kw;
        const bool ok = hi >= 0 && hi < Hin && wi >= 0 && wi < Win;
        xv[kh * K + kw] = ok ? xc[hi * Win + wi] : 0.0f;
      }
#pragma unroll
    for (int c = 0; c < COC; ++c) {
      const float d = dyc[(size_t)c * Pout + p];
#pragma unroll
      for (int t = 0; t < KK; ++t) acc[c][t] = fmaf(d, xv[t], acc[c][t]);
    }
  }
  // butterfly over the 64 lanes (every lane ends with the total, fixed order),
  // then lane e keeps element e
  float mine = 0.0f;
#pragma unroll
  for (int c = 0; c < COC; ++c)
#pragma unroll
    for (int t = 0; t < KK; ++t) {
      float v = acc[c][t];
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
      if (lane == (c * KK + t) % 64) mine = v;
      if ((c * KK + t) % 64 == 63 || (c == COC - 1 && t == KK - 1)) {
        // flush up to 64 collected elements: element e = base + lane
        const int e = (c * KK + t) / 64 * 64 + lane;
        if (e <= c * KK + t) {
          const int co = e / KK, tt = e - co * KK;
          part[(size_t)slab * Cout * cin_g * KK +
               ((size_t)(g * CG + cc * COC + co) * cin_g + ci) * KK + tt] = mine;
        }
      }
    }
}

__global__ __launch_bounds__(256) void gconv_wgrad_reduce_kernel(
    const float* __restrict__ part, int nslabs, int total, float* __restrict__ dw,
    int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float s = 0.0f;
  for (int k = 0; k < nslabs; ++k) s += part[(size_t)k * total + i];  // slab order
  dw[i] = accumulate ? dw[i] + s : s;
}

inline bool gconv_geometry(int N, int Cin, int Cout, int groups, int K, int stride,
                           int pad, int Hin, int Win, int* Hout, int* Wout) {
  if (N < 1 || groups < 1 || Cin < 1 || Cout < 1 || Cin % groups || Cout % groups ||
      K < 1 || stride < 1 || pad < 0 || Hin < 1 || Win < 1)
    return false;
  *Hout = (Hin + 2 * pad - K) / stride + 1;
  *Wout = (Win + 2 * pad - K) / stride + 1;
  return Hin + 2 * pad >= K && Win + 2 * pad >= K && *Hout >= 1 && *Wout >= 1;
}

inline bool gconv_bwd_supported(int CG, int K, int stride) {
  return (K == 1 || K == 3) && (stride == 1 || stride == 2) &&
         (CG == 4 || CG == 8 || CG == 16 || CG == 32);
}

}  // namespace

extern "C" size_t ld_gconv_weight_image_floats(int Cout, int Cin, int groups, int K) {
  if (groups < 1 || Cout % groups || Cin % groups) return 0;
  return (size_t)Cout * (Cin / groups) * K * K;
}

extern "C" int ld_gconv_weight_transform(const float* w, int Cout, int Cin, int groups,
                                         int K, float* image, ld_stream_t stream) {
  if (!w || !image || groups < 1 || Cout % groups || Cin % groups || K < 1)
    return LD_EINVAL;
  const int total = Cout * (Cin / groups) * K * K;
  LD_LAUNCH(gconv_weight_image_kernel, dim3((total + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, w, image, groups, Cout / groups, Cin / groups,
                     K * K);
  return (int)hipGetLastError();
}

extern "C" int ld_gconv_forward(const float* x, const float* wimage, float* y, int N,
                                int Cin, int Cout, int groups, int K, int stride, int pad,
                                int Hin, int Win, const float* scale, const float* shift,
                                int relu, ld_stream_t stream) {
  if (!x || !wimage || !y || N < 1 || groups < 1 || Cin % groups || Cout % groups ||
      stride < 1 || pad < 0 || Hin < 1 || Win < 1 || (scale == nullptr) != (shift == nullptr))
    return LD_EINVAL;
  if (K != 1 && K != 3) return LD_EUNSUPPORTED;
  const int Hout = (Hin + 2 * pad - K) / stride + 1, Wout = (Win + 2 * pad - K) / stride + 1;
  if (Hout < 1 || Wout < 1) return LD_EINVAL;
  const int CG = Cout / groups, cin_g = Cin / groups;
  const dim3 grid((Hout * Wout + 255) / 256, groups, N);
  hipStream_t st = (hipStream_t)stream;
  if (K == 3)
    return launch_gconv<3>(CG, grid, st, x, wimage, y, Cin, Cout, cin_g, stride, pad, Hin,
                           Win, Hout, Wout, scale, shift, relu);
  return launch_gconv<1>(CG, grid, st, x, wimage, y, Cin, Cout, cin_g, stride, pad, Hin,
                         Win, Hout, Wout, scale, shift, relu);
}

extern "C" size_t ld_gconv_weight_image_bwd_floats(int Cout, int Cin, int groups, int K) {
  if (groups < 1 || Cout < 1 || Cin < 1 || Cout % groups || Cin % groups || K < 1)
    return 0;
  const int cin_g = Cin / groups, CIC = gconv_cic(cin_g);
  return (size_t)Cout * ((cin_g + CIC - 1) / CIC) * CIC * K * K;
}

extern "C" int ld_gconv_weight_transform_bwd(const float* w, int Cout, int Cin,
                                             int groups, int K, float* image,
                                             ld_stream_t stream) {
  if (!w || !image || groups < 1 || Cout < 1 || Cin < 1 || Cout % groups ||
      Cin % groups || K < 1)
    return LD_EINVAL;
  const int cin_g = Cin / groups, CIC = gconv_cic(cin_g);
  const int nchunk = (cin_g + CIC - 1) / CIC;
  const long long total = (long long)Cout * nchunk * CIC * K * K;
  if (total > 0x7fffffffLL) return LD_EUNSUPPORTED;
  LD_LAUNCH(gconv_weight_image_bwd_kernel, dim3(((int)total + 255) / 256), dim3(256), 0,
            (hipStream_t)stream, w, image, groups, Cout / groups, cin_g, K * K, CIC,
            nchunk);
  return (int)hipGetLastError();
}

extern "C" int ld_gconv_dgrad(const float* dy, const float* wimage_bwd,
                              const float* addend, float* dx, int N, int Cin, int Cout,
                              int groups, int K, int stride, int pad, int Hin, int Win,
                              ld_stream_t stream) {
  int Hout, Wout;
  if (!dy || !wimage_bwd || !dx ||
      !gconv_geometry(N, Cin, Cout, groups, K, stride, pad, Hin, Win, &Hout, &Wout))
    return LD_EINVAL;
  const int CG = Cout / groups, cin_g = Cin / groups;
  if (!gconv_bwd_supported(CG, K, stride)) return LD_EUNSUPPORTED;
  const int CIC = gconv_cic(cin_g), nchunk = (cin_g + CIC - 1) / CIC;
  if ((long long)groups * nchunk > 65535 || N > 65535) return LD_EUNSUPPORTED;
  const dim3 grid((Hin * Win + 255) / 256, groups * nchunk, N);
  hipStream_t st = (hipStream_t)stream;
#define LD_GD(C, KS)                                                                   \
  LD_LAUNCH((gconv_dgrad_kernel<C, KS>), grid, dim3(256), 0, st, dy, wimage_bwd, addend, \
            dx, Cin, Cout, CG, cin_g, nchunk, stride, pad, Hin, Win, Hout, Wout)
  if (K == 3) {
    switch (CIC) {
      case 4: LD_GD(4, 3); break;
      case 8: LD_GD(8, 3); break;
      case 16: LD_GD(16, 3); break;
      default: LD_GD(32, 3); break;
    }
  } else {
    switch (CIC) {
      case 4: LD_GD(4, 1); break;
      case 8: LD_GD(8, 1); break;
      case 16: LD_GD(16, 1); break;
      default: LD_GD(32, 1); break;
    }
  }
#undef LD_GD
  return (int)hipGetLastError();
}

extern "C" int ld_gconv_wgrad_slabs(int N, int K, int stride, int pad, int Hin, int Win) {
  int Hout, Wout;
  if (!gconv_geometry(N, 1, 1, 1, K, stride, pad, Hin, Win, &Hout, &Wout)) return 0;
  return N * ((Hout * Wout + GW_SLAB - 1) / GW_SLAB);
}

extern "C" size_t ld_gconv_wgrad_workspace_floats(int N, int Cin, int Cout, int groups,
                                                  int K, int stride, int pad, int Hin,
                                                  int Win) {
  int Hout, Wout;
  if (!gconv_geometry(N, Cin, Cout, groups, K, stride, pad, Hin, Win, &Hout, &Wout))
    return 0;
  return (size_t)ld_gconv_wgrad_slabs(N, K, stride, pad, Hin, Win) * Cout *
         (Cin / groups) * K * K;
}

extern "C" int ld_gconv_wgrad(const float* x, const float* dy, float* dw, int accumulate,
                              float* workspace, size_t workspace_floats, int N, int Cin,
                              int Cout, int groups, int K, int stride, int pad, int Hin,
                              int Win, ld_stream_t stream) {
  int Hout, Wout;
  if (!x || !dy || !dw || !workspace ||
      !gconv_geometry(N, Cin, Cout, groups, K, stride, pad, Hin, Win, &Hout, &Wout))
    return LD_EINVAL;
  const int CG = Cout / groups, cin_g = Cin / groups;
  if (!gconv_bwd_supported(CG, K, stride)) return LD_EUNSUPPORTED;
  const int slabs_img = (Hout * Wout + GW_SLAB - 1) / GW_SLAB, nslabs = N * slabs_img;
  const long long total = (long long)Cout * cin_g * K * K;
  if (total > 0x7fffffffLL) return LD_EUNSUPPORTED;
  if (workspace_floats < (size_t)nslabs * (size_t)total) return LD_EINVAL;
  const int COC = CG < 8 ? 4 : 8;
  const long long gy = (long long)groups * ((cin_g + 3) / 4) * (CG / COC);
  if (gy > 65535) return LD_EUNSUPPORTED;
  const dim3 grid(nslabs, (unsigned)gy, 1);
  hipStream_t st = (hipStream_t)stream;
#define LD_GW(C, KS)                                                                  \
  LD_LAUNCH((gconv_wgrad_kernel<C, KS>), grid, dim3(256), 0, st, x, dy, workspace, Cin, \
            Cout, CG, cin_g, stride, pad, Hin, Win, Hout, Wout, slabs_img)
  if (K == 3) {
    if (COC == 4) LD_GW(4, 3); else LD_GW(8, 3);
  } else {
    if (COC == 4) LD_GW(4, 1); else LD_GW(8, 1);
  }
#undef LD_GW
  LD_LAUNCH(gconv_wgrad_reduce_kernel, dim3(((int)total + 255) / 256), dim3(256), 0, st,
            (const float*)workspace, nslabs, (int)total, dw, accumulate);
  return (int)hipGetLastError();
}
