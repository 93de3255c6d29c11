// Res2Net block glue (mmdet/models/backbones/res2net.py:108-162): everything
// between the GEMMs of a Bottle2neck, pure HBM traffic.
//
//   ld_res2_gather   y = u[:, slice*w : (slice+1)*w] (+ addend): the contiguous
//                    (N, w, P) operand of conv i, the hierarchical add fused.
//                    Backward reuses it: d sp_i = d cat[:, slice i] (+ d x_{i+1}).
//   ld_res2_concat   y = cat(a, b, c, tail) with tail = slice `tslice` of a
//                    (N, Ct, .) tensor, copied, average-pooled 3x3 / stride /
//                    pad 1 (divisor 9), or run through that pool's backward.
//                    Backward reuses it: d u = cat(d x_0, d x_1, d x_2, tail').
//   ld_avgpool_ceil_forward / _backward   AvgPool2d(k, k, ceil_mode=True,
//                    count_include_pad=False) of the avg_down shortcut.
//
// Arithmetic contract (the tests pin it bit for bit against the CPU operators
// of the framework): a pool is a row-major fp32 sum starting from 0 followed by
// ONE IEEE division (never a reciprocal multiply; -ffp-contract=off); a pool
// backward sums dy / divisor addends in ascending (oh, ow) order starting from
// 0.  All four are gathers: no atomics, two runs are bit-identical.
//
// Alignment: slice i of an image starts i*w*P floats into it; with w = 26 and
// odd P that is not a multiple of 16 bytes.  The 16-byte path is taken only when
// every base address and every per-image / per-slice stride it will form is a
// multiple of 16 bytes; anything else takes the scalar kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ld_launch.h"

#include "../../include/ld_hip.h"

#define LD_STREAM ((hipStream_t)stream)

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ float4 ld4(const float* p) {
  return *reinterpret_cast<const float4*>(p);
}
__device__ __forceinline__ void st4(float* p, float4 v) {
  *reinterpret_cast<float4*>(p) = v;
}

// ------------------------------------------------------------------ gather ---
// grid (ceil(seg / (V * 256)), N); seg = w * P floats per image.
template <int V>
__global__ __launch_bounds__(kThreads) void res2_gather_kernel(
    const float* __restrict__ u, const float* __restrict__ addend,
    float* __restrict__ y, size_t img, size_t off, size_t seg) {
  const size_t i = ((size_t)blockIdx.x * kThreads + threadIdx.x) * V;
  if (i >= seg) return;
  const size_t n = blockIdx.y;
  const float* src = u + n * img + off + i;
  float* dst = y + n * seg + i;
  if (V == 4) {
    float4 v = ld4(src);
    if (addend) {
      const float4 a = ld4(addend + n * seg + i);
      v.x = a.x + v.x;
      v.y = a.y + v.y;
      v.z = a.z + v.z;
      v.w = a.w + v.w;
    }
    st4(dst, v);
  } else {
    float v = *src;
    if (addend) v = addend[n * seg + i] + v;
    *dst = v;
  }
}

// ------------------------------------------------------------------ concat ---
struct CatArgs {
  const float* part[3];  // (N, w, Py) each
  const float* t;        // (N, Ct, Pt): the tail's source
  float* y;              // (N, 4w, Py)
  size_t seg;            // w * Py
  size_t t_img;          // Ct * Pt
  size_t t_off;          // tslice * w * Pt
  int H, W;              // the unpooled map
  int Ho, Wo;            // the pooled map
  int stride;
};

// AvgPool2d(3, stride, padding=1), count_include_pad=True: the divisor counts
// the padding (window clipped to the padded extent), the sum only what is valid.
__device__ __forceinline__ float pool3_fwd(const float* __restrict__ plane, int H,
                                           int W, int stride, int oh, int ow) {
  int hs = oh * stride - 1, ws = ow * stride - 1;
  int he = min(hs + 3, H + 1), we = min(ws + 3, W + 1);
  const int div = (he - hs) * (we - ws);
  hs = max(hs, 0);
  ws = max(ws, 0);
  he = min(he, H);
  we = min(we, W);
  float s = 0.f;
  for (int h = hs; h < he; ++h)
    for (int w = ws; w < we; ++w) s += plane[(size_t)h * W + w];
  return s / (float)div;
}

__device__ __forceinline__ float pool3_bwd(const float* __restrict__ dplane, int H,
                                           int W, int Ho, int Wo, int stride, int h,
                                           int w) {
  // windows [o*stride - 1, o*stride + 1] that contain the input position
  const int oh0 = h <= 1 ? 0 : (h - 1 + stride - 1) / stride;
  const int ow0 = w <= 1 ? 0 : (w - 1 + stride - 1) / stride;
  const int oh1 = min(Ho - 1, (h + 1) / stride);
  const int ow1 = min(Wo - 1, (w + 1) / stride);
  float s = 0.f;
  for (int oh = oh0; oh <= oh1; ++oh) {
    const int hs = oh * stride - 1;
    const int dh = min(hs + 3, H + 1) - hs;
    for (int ow = ow0; ow <= ow1; ++ow) {
      const int ws = ow * stride - 1;
      const int div = dh * (min(ws + 3, W + 1) - ws);
      s += dplane[(size_t)oh * Wo + ow] / (float)div;
    }
  }
  return s;
}

// MODE 0: tail copied; 1: tail = pool(t) (t at H x W, y at Ho x Wo);
// 2: tail = pool backward of t (t at Ho x Wo, y at H x W).
// grid (ceil(4 * seg / (V * 256)), N).
template <int V, int MODE>
__global__ __launch_bounds__(kThreads) void res2_concat_kernel(CatArgs a) {
  const size_t e = ((size_t)blockIdx.x * kThreads + threadIdx.x) * V;
  if (e >= 4 * a.seg) return;
  const size_t n = blockIdx.y;
  const int part = (int)(e / a.seg);
  const size_t r = e - (size_t)part * a.seg;
  float* dst = a.y + n * 4 * a.seg + e;
  if (part < 3) {  // V == 4: seg % 4 == 0, a vector never straddles two parts
    const float* src = a.part[part] + n * a.seg + r;
    if (V == 4)
      st4(dst, ld4(src));
    else
      *dst = *src;
    return;
  }
  const float* timg = a.t + n * a.t_img + a.t_off;
  if (MODE == 0) {
    if (V == 4)
      st4(dst, ld4(timg + r));
    else
      *dst = timg[r];
    return;
  }
  const int Hy = MODE == 1 ? a.Ho : a.H, Wy = MODE == 1 ? a.Wo : a.W;
  const size_t Py = (size_t)Hy * Wy;
  const size_t Pt = MODE == 1 ? (size_t)a.H * a.W : (size_t)a.Ho * a.Wo;
  float v[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const size_t q = r + j;
    const size_t c = q / Py;
    const int p = (int)(q - c * Py);
    const int h = p / Wy, w = p - h * Wy;
    const float* plane = timg + c * Pt;
    v[j] = MODE == 1 ? pool3_fwd(plane, a.H, a.W, a.stride, h, w)
                     : pool3_bwd(plane, a.H, a.W, a.Ho, a.Wo, a.stride, h, w);
  }
  if (V == 4)
    st4(dst, make_float4(v[0], v[V > 1 ? 1 : 0], v[V > 2 ? 2 : 0], v[V > 3 ? 3 : 0]));
  else
    *dst = v[0];
}

// ----------------------------------------------------------- shortcut pool ---
// AvgPool2d(k, k, ceil_mode=True, count_include_pad=False): window o covers
// [o*k, min(o*k + k, H)); the divisor is the number of valid elements.
__global__ __launch_bounds__(kThreads) void avgpool_ceil_fwd_kernel(
    const float* __restrict__ x, size_t rows, int H, int W, int Ho, int Wo, int k,
    float* __restrict__ y) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= rows * Ho * Wo) return;
  const int ow = (int)(i % Wo);
  const size_t q = i / Wo;
  const int oh = (int)(q % Ho);
  const float* plane = x + (q / Ho) * H * W;
  const int hs = oh * k, ws = ow * k;
  const int he = min(hs + k, H), we = min(ws + k, W);
  float s = 0.f;
  for (int h = hs; h < he; ++h)
    for (int w = ws; w < we; ++w) s += plane[(size_t)h * W + w];
  y[i] = s / (float)((he - hs) * (we - ws));
}

__global__ __launch_bounds__(kThreads) void avgpool_ceil_bwd_kernel(
    const float* __restrict__ dy, size_t rows, int H, int W, int Ho, int Wo, int k,
    float* __restrict__ dx) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= rows * H * W) return;
  const int w = (int)(i % W);
  const size_t q = i / W;
  const int h = (int)(q % H);
  const int oh = h / k, ow = w / k;  // the one window this element belongs to
  const int div = (min(oh * k + k, H) - oh * k) * (min(ow * k + k, W) - ow * k);
  dx[i] = 0.f + dy[((q / H) * Ho + oh) * Wo + ow] / (float)div;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int pooled(int h, int stride) { return (h + 2 - 3) / stride + 1; }
constexpr size_t kMaxGridX = 0x7fffffffu;

}  // namespace

extern "C" int ld_res2_gather(const float* u, const float* addend, int N, int C, int w,
                              int slice, long long P, float* y, ld_stream_t stream) {
  if (!u || !y || N < 1 || N > 65535 || C < 1 || w < 1 || slice < 0 || P < 1 ||
      (long long)(slice + 1) * w > C)
    return LD_EINVAL;
  const size_t img = (size_t)C * (size_t)P, seg = (size_t)w * (size_t)P;
  const size_t off = (size_t)slice * seg;
  if ((seg + kThreads - 1) / kThreads > kMaxGridX) return LD_EINVAL;
  const bool vec = seg % 4 == 0 && off % 4 == 0 && img % 4 == 0 && aligned16(u) &&
                   aligned16(y) && (!addend || aligned16(addend));
  if (vec) {
    const size_t threads = seg / 4;
    LD_LAUNCH(res2_gather_kernel<4>, dim3((unsigned)((threads + kThreads - 1) / kThreads), N),
              dim3(kThreads), 0, LD_STREAM, u, addend, y, img, off, seg);
  } else {
    LD_LAUNCH(res2_gather_kernel<1>, dim3((unsigned)((seg + kThreads - 1) / kThreads), N),
              dim3(kThreads), 0, LD_STREAM, u, addend, y, img, off, seg);
  }
  return (int)hipGetLastError();
}

extern "C" int ld_res2_concat(const float* a, const float* b, const float* c,
                              const float* t, int N, int w, int Ct, int tslice, int H,
                              int W, int stride, int mode, float* y,
                              ld_stream_t stream) {
  if (!a || !b || !c || !t || !y || N < 1 || N > 65535 || w < 1 || Ct < 1 ||
      tslice < 0 || (long long)(tslice + 1) * w > Ct || H < 1 || W < 1 ||
      stride < 1 || mode < LD_RES2_TAIL_COPY || mode > LD_RES2_TAIL_POOL_BWD ||
      (long long)H * W > 0x7fffffffLL)
    return LD_EINVAL;
  CatArgs k;
  k.part[0] = a;
  k.part[1] = b;
  k.part[2] = c;
  k.t = t;
  k.y = y;
  k.H = H;
  k.W = W;
  k.stride = stride;
  const bool pool = mode != LD_RES2_TAIL_COPY;
  k.Ho = pool ? pooled(H, stride) : H;
  k.Wo = pool ? pooled(W, stride) : W;
  const size_t P = (size_t)H * W, Po = (size_t)k.Ho * k.Wo;
  const size_t Py = mode == LD_RES2_TAIL_POOL ? Po : P;
  const size_t Pt = mode == LD_RES2_TAIL_POOL_BWD ? Po : P;
  k.seg = (size_t)w * Py;
  k.t_img = (size_t)Ct * Pt;
  k.t_off = (size_t)tslice * w * Pt;
  if ((4 * k.seg + kThreads - 1) / kThreads > kMaxGridX) return LD_EINVAL;
  // the tail is read with vectors only when it is copied
  const bool vec = k.seg % 4 == 0 && aligned16(a) && aligned16(b) && aligned16(c) &&
                   aligned16(y) &&
                   (pool || (k.t_img % 4 == 0 && k.t_off % 4 == 0 && aligned16(t)));
  const size_t threads = vec ? k.seg : 4 * k.seg;
  const dim3 grid((unsigned)((threads + kThreads - 1) / kThreads), N);
#define LD_CAT(V, M) \
  LD_LAUNCH((res2_concat_kernel<V, M>), grid, dim3(kThreads), 0, LD_STREAM, k)
  if (mode == LD_RES2_TAIL_COPY) {
    if (vec) LD_CAT(4, 0); else LD_CAT(1, 0);
  } else if (mode == LD_RES2_TAIL_POOL) {
    if (vec) LD_CAT(4, 1); else LD_CAT(1, 1);
  } else {
    if (vec) LD_CAT(4, 2); else LD_CAT(1, 2);
  }
#undef LD_CAT
  return (int)hipGetLastError();
}

static int avgpool_ceil(const float* src, long long rows, int H, int W, int k, float* dst,
                        bool backward, ld_stream_t stream) {
  if (!src || !dst || rows < 1 || H < 1 || W < 1 || k < 1) return LD_EINVAL;
  const int Ho = (H + k - 1) / k, Wo = (W + k - 1) / k;
  const size_t total = (size_t)rows * (backward ? (size_t)H * W : (size_t)Ho * Wo);
  if ((total + kThreads - 1) / kThreads > kMaxGridX) return LD_EINVAL;
  const dim3 grid((unsigned)((total + kThreads - 1) / kThreads));
  if (backward)
    LD_LAUNCH(avgpool_ceil_bwd_kernel, grid, dim3(kThreads), 0, LD_STREAM, src,
              (size_t)rows, H, W, Ho, Wo, k, dst);
  else
    LD_LAUNCH(avgpool_ceil_fwd_kernel, grid, dim3(kThreads), 0, LD_STREAM, src,
              (size_t)rows, H, W, Ho, Wo, k, dst);
  return (int)hipGetLastError();
}

extern "C" int ld_avgpool_ceil_forward(const float* x, long long rows, int H, int W,
                                       int k, float* y, ld_stream_t stream) {
  return avgpool_ceil(x, rows, H, W, k, y, false, stream);
}

extern "C" int ld_avgpool_ceil_backward(const float* dy, long long rows, int H, int W,
                                        int k, float* dx, ld_stream_t stream) {
  return avgpool_ceil(dy, rows, H, W, k, dx, true, stream);
}
