// AP landscape and teacher-student discrepancy on gfx950: the reference's
// AP_landscape/ tool (detectors/single_stage.py:113-121, apis/test.py:105-177).
//
// Replaces (reference file:line)
//   p_l = 0.9 * x[l] + 0.7 * former_x[l], five levels      single_stage.py:115-119
//   abs(t - s).mean(1).sum() per level, three families     apis/test.py:114-177
//   pearsonr(f5_s, f5_t).mean() on the P5 channel maps     apis/test.py:106-111
//
// Every tensor is the level-concatenated (N, C, P) fp32 layout of the head
// towers (nn.hip ld_pack_levels); a level is a segment of the P axis.
//
// levels_mix_kernel: out[k][i] = a_k * own[i] + b_k * other[i] for K grid points
// in one pass: an element of own / other is read once and K outputs are written,
// (2 + K) * 4 B per element.  Two fp32 multiplies and one fp32 add in that order
// (this file is built with -ffp-contract=off): torch's a * x + b * y, bit for
// bit.  float4 accesses when the three bases and every out + k * n are 16-byte
// aligned, a scalar tail behind them, scalar throughout otherwise.
//
// levels_abs_err_kernel: a workgroup owns 256 consecutive positions of one
// level of one image and a slice of <= 32 channels; a thread owns one position
// and walks the slice's channels (a wave reads 256 consecutive bytes of each
// operand per channel).  |t - s| is taken in fp32, the values the reference
// sums; everything after that is double.  One partial per workgroup, then
// levels_abs_err_sum_kernel: one thread per (image, level) adds its partials in
// index order and divides by C.
//
// levels_pearson_kernel: a row is one (n, c) and one level segment.  Segments of
// <= kShort positions take one wave per row, longer ones a workgroup per row.
// Pass 1 the means, pass 2 the centred sums Sxy, Sxx, Syy, all double; the
// second pass re-reads a segment of at most 67 KB that the first just pulled
// in.  r = Sxy / sqrt(Sxx * Syy) goes to a (N, L, C) table, NaN for a
// degenerate row (< 2 positions, Sxx == 0 or Syy == 0: torch gives NaN there);
// levels_pearson_sum_kernel: one wave per (image, level) sums the valid r and
// counts valid / degenerate rows.
//
// No float atomics; every output has one writer and every sum a fixed order:
// two calls on the same input give the same bits.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/ld_hip.h"
#include "eval_common.h"
#include "ld_launch.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSlice = 32;    // channels of one abs_err workgroup
constexpr int kShort = 1024;  // longest segment a single wave takes

struct MixCoefs {
  float a[LD_LEVELS_MIX_MAX_K];
  float b[LD_LEVELS_MIX_MAX_K];
  int K;
};

__global__ __launch_bounds__(kThreads) void levels_mix_kernel(const float* __restrict__ own,
                                                             const float* __restrict__ other,
                                                             float* __restrict__ out,
                                                             long long n, long long n4,
                                                             MixCoefs cf) {
  const long long step = (long long)gridDim.x * kThreads;
  const long long tid = (long long)blockIdx.x * kThreads + threadIdx.x;
  const float4* own4 = (const float4*)own;
  const float4* other4 = (const float4*)other;
  for (long long i = tid; i < n4; i += step) {
    const float4 x = own4[i], y = other4[i];
#pragma unroll
    for (int k = 0; k < LD_LEVELS_MIX_MAX_K; ++k) {
      if (k >= cf.K) break;
      const float a = cf.a[k], b = cf.b[k];
      float4 o;
      o.x = a * x.x + b * y.x;
      o.y = a * x.y + b * y.y;
      o.z = a * x.z + b * y.z;
      o.w = a * x.w + b * y.w;
      ((float4*)(out + (long long)k * n))[i] = o;
    }
  }
  for (long long i = n4 * 4 + tid; i < n; i += step) {
    const float x = own[i], y = other[i];
    for (int k = 0; k < cf.K; ++k) out[(long long)k * n + i] = cf.a[k] * x + cf.b[k] * y;
  }
}

// ---- level tables ----------------------------------------------------------
struct Segs {
  int L, P;
  int off[LD_MAX_LEVELS];    // first position of the level
  int len[LD_MAX_LEVELS];    // its positions
  int first[LD_MAX_LEVELS];  // its first chunk (abs_err) / workgroup (pearson)
  int total;                 // chunks / workgroups of all levels
};

// -> 0 and the offsets, or LD_EINVAL: 1..LD_MAX_LEVELS levels of >= 1 positions
// that fill P exactly
int fill_segs(Segs& s, const ld_levels_t* lv, int P) {
  if (!lv || P <= 0) return LD_EINVAL;
  if (lv->num_levels < 1 || lv->num_levels > LD_MAX_LEVELS) return LD_EINVAL;
  long long off = 0;
  for (int l = 0; l < lv->num_levels; ++l) {
    if (lv->H[l] <= 0 || lv->W[l] <= 0) return LD_EINVAL;
    const long long len = (long long)lv->H[l] * lv->W[l];
    if (off + len > P) return LD_EINVAL;
    s.off[l] = (int)off;
    s.len[l] = (int)len;
    off += len;
  }
  if (off != P) return LD_EINVAL;
  s.L = lv->num_levels;
  s.P = P;
  return 0;
}

__device__ __forceinline__ int level_of(const Segs& s, int unit) {
  int l = 0;
  while (l + 1 < s.L && unit >= s.first[l + 1]) ++l;
  return l;
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// sum over the workgroup, returned to every thread; s_red holds kWaves doubles
__device__ __forceinline__ double block_sum(double v, double* s_red) {
  v = wave_sum(v);
  __syncthreads();  // the previous use of s_red is over
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  double o = 0.0;
  for (int k = 0; k < kWaves; ++k) o += s_red[k];
  return o;
}

// ---- mean absolute error -----------------------------------------------------
// grid (chunks of all levels, channel slices, N); partial[(n * slices + z) *
// total + chunk]
__global__ __launch_bounds__(kThreads) void levels_abs_err_kernel(const float* __restrict__ t,
                                                                 const float* __restrict__ s,
                                                                 int C, Segs sg,
                                                                 double* __restrict__ partial) {
  __shared__ double s_red[kWaves];
  const int chunk = blockIdx.x, z = blockIdx.y, n = blockIdx.z;
  const int l = level_of(sg, chunk);
  const int p = (chunk - sg.first[l]) * kThreads + threadIdx.x;
  const int c0 = z * kSlice, c1 = min(C, c0 + kSlice);
  double acc = 0.0;
  if (p < sg.len[l]) {
    const size_t base = ((size_t)n * C + c0) * sg.P + sg.off[l] + p;
    const float* tp = t + base;
    const float* sp = s + base;
    for (int c = c0; c < c1; ++c) {
      acc += (double)fabsf(*tp - *sp);
      tp += sg.P;
      sp += sg.P;
    }
  }
  acc = block_sum(acc, s_red);
  if (threadIdx.x == 0)
    partial[((size_t)n * gridDim.y + z) * sg.total + chunk] = acc;
}

__global__ void levels_abs_err_sum_kernel(const double* __restrict__ partial, int N, int C,
                                          int slices, Segs sg, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * sg.L) return;
  const int n = i / sg.L, l = i - n * sg.L;
  const int k0 = sg.first[l], k1 = l + 1 < sg.L ? sg.first[l + 1] : sg.total;
  double acc = 0.0;
  for (int z = 0; z < slices; ++z) {
    const double* row = partial + ((size_t)n * slices + z) * sg.total;
    for (int k = k0; k < k1; ++k) acc += row[k];
  }
  out[i] = acc / (double)C;
}

// ---- Pearson r -----------------------------------------------------------------
__device__ __forceinline__ double pearson_r(int len, double sxy, double sxx, double syy) {
  if (len < 2 || sxx == 0.0 || syy == 0.0) return NAN;
  return sxy / sqrt(sxx * syy);
}

// rows = N * C; rtab[(n * L + l) * C + c]
__global__ __launch_bounds__(kThreads) void levels_pearson_kernel(const float* __restrict__ t,
                                                                 const float* __restrict__ s,
                                                                 int rows, int C, Segs sg,
                                                                 double* __restrict__ rtab) {
  __shared__ double s_red[kWaves];
  const int l = level_of(sg, blockIdx.x);
  const int len = sg.len[l];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool wide = len > kShort;  // uniform over the workgroup
  const int unit = blockIdx.x - sg.first[l];
  const int row = wide ? unit : unit * kWaves + w;
  const int i0 = wide ? threadIdx.x : lane, di = wide ? kThreads : 64;
  const bool live = row < rows;  // uniform over the wave
  const size_t base = (size_t)(live ? row : 0) * sg.P + sg.off[l];
  const float* x = t + base;
  const float* y = s + base;
  double sx = 0.0, sy = 0.0;
  if (live)
    for (int i = i0; i < len; i += di) sx += (double)x[i], sy += (double)y[i];
  if (wide) {
    sx = block_sum(sx, s_red);
    sy = block_sum(sy, s_red);
  } else {
    sx = wave_sum(sx);
    sy = wave_sum(sy);
  }
  const double mx = sx / (double)len, my = sy / (double)len;
  double sxy = 0.0, sxx = 0.0, syy = 0.0;
  if (live)
    for (int i = i0; i < len; i += di) {
      const double dx = (double)x[i] - mx, dy = (double)y[i] - my;
      sxy += dx * dy;
      sxx += dx * dx;
      syy += dy * dy;
    }
  if (wide) {
    sxy = block_sum(sxy, s_red);
    sxx = block_sum(sxx, s_red);
    syy = block_sum(syy, s_red);
  } else {
    sxy = wave_sum(sxy);
    sxx = wave_sum(sxx);
    syy = wave_sum(syy);
  }
  if (live && (wide ? threadIdx.x == 0 : lane == 0)) {
    const int n = row / C, c = row - n * C;
    rtab[((size_t)n * sg.L + l) * C + c] = pearson_r(len, sxy, sxx, syy);
  }
}

// one wave per (n, l): lane j takes rows j, j + 64, ... in order, then the tree
__global__ __launch_bounds__(64) void levels_pearson_sum_kernel(const double* __restrict__ rtab,
                                                               int C, double* __restrict__ r_sum,
                                                               int32_t* __restrict__ counts) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const double* row = rtab + (size_t)i * C;
  double acc = 0.0;
  int valid = 0, bad = 0;
  for (int c = lane; c < C; c += 64) {
    const double r = row[c];
    if (r != r) {
      ++bad;
    } else {
      acc += r;
      ++valid;
    }
  }
  acc = wave_sum(acc);
  for (int off = 32; off > 0; off >>= 1) {
    valid += __shfl_xor(valid, off, 64);
    bad += __shfl_xor(bad, off, 64);
  }
  if (lane == 0) {
    r_sum[i] = acc;
    counts[2 * i] = valid;
    counts[2 * i + 1] = bad;
  }
}

int abs_err_plan(Segs& sg, const ld_levels_t* lv, int N, int C, int P, int& slices) {
  if (N <= 0 || C <= 0) return LD_EINVAL;
  const int rc = fill_segs(sg, lv, P);
  if (rc) return rc;
  int total = 0;
  for (int l = 0; l < sg.L; ++l) {
    sg.first[l] = total;
    total += (sg.len[l] + kThreads - 1) / kThreads;
  }
  sg.total = total;
  slices = (C + kSlice - 1) / kSlice;
  if (slices > 65535 || N > 65535) return LD_EUNSUPPORTED;
  return 0;
}

int pearson_plan(Segs& sg, const ld_levels_t* lv, int N, int C, int P) {
  if (N <= 0 || C <= 0) return LD_EINVAL;
  const int rc = fill_segs(sg, lv, P);
  if (rc) return rc;
  if ((long long)N * C >= (1ll << 24)) return LD_EUNSUPPORTED;
  const int rows = N * C;
  long long total = 0;
  for (int l = 0; l < sg.L; ++l) {
    sg.first[l] = (int)total;
    total += sg.len[l] > kShort ? rows : (rows + kWaves - 1) / kWaves;
  }
  if (total >= (1ll << 31)) return LD_EUNSUPPORTED;
  sg.total = (int)total;
  return 0;
}

}  // namespace

extern "C" {

int ld_levels_mix(const float* own, const float* other, long long n, int K,
                  const float* coefs, float* out, ld_stream_t stream_) {
  if (!own || !other || !coefs || !out) return LD_EINVAL;
  if (n <= 0 || K < 1 || K > LD_LEVELS_MIX_MAX_K) return LD_EINVAL;
  if (n >= (1ll << 40)) return LD_EUNSUPPORTED;
  MixCoefs cf{};
  cf.K = K;
  for (int k = 0; k < K; ++k) cf.a[k] = coefs[2 * k], cf.b[k] = coefs[2 * k + 1];
  const bool vec = (((uintptr_t)own | (uintptr_t)other | (uintptr_t)out) & 15) == 0 &&
                   (K == 1 || n % 4 == 0);
  const long long n4 = vec ? n / 4 : 0;
  const long long work = n4 + (n - 4 * n4);
  long long blocks = (work + kThreads - 1) / kThreads;
  if (blocks > (1 << 20)) blocks = 1 << 20;
  LD_LAUNCH(levels_mix_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream_,
            own, other, out, n, n4, cf);
  return (int)hipGetLastError();
}

size_t ld_levels_abs_err_workspace_bytes(const ld_levels_t* lv, int N, int C, int P) {
  Segs sg{};
  int slices = 0;
  if (abs_err_plan(sg, lv, N, C, P, slices)) return 0;
  return ldeval::align_up((size_t)N * slices * sg.total * sizeof(double)) + 256;
}

int ld_levels_abs_err(const ld_levels_t* lv, const float* t, const float* s, int N, int C,
                      int P, double* out, void* workspace, size_t workspace_bytes,
                      ld_stream_t stream_) {
  Segs sg{};
  int slices = 0;
  const int rc = abs_err_plan(sg, lv, N, C, P, slices);
  if (rc) return rc;
  if (!t || !s || !out) return LD_EINVAL;
  const size_t need = (size_t)N * slices * sg.total * sizeof(double);
  if (!workspace || workspace_bytes < need) return LD_ENOSPACE;
  if ((uintptr_t)workspace & 7) return LD_EINVAL;  // doubles inside
  double* partial = (double*)workspace;
  LD_LAUNCH(levels_abs_err_kernel, dim3(sg.total, slices, N), dim3(kThreads), 0,
            (hipStream_t)stream_, t, s, C, sg, partial);
  LD_LAUNCH(levels_abs_err_sum_kernel, dim3((N * sg.L + 63) / 64), dim3(64), 0,
            (hipStream_t)stream_, (const double*)partial, N, C, slices, sg, out);
  return (int)hipGetLastError();
}

size_t ld_levels_pearson_workspace_bytes(const ld_levels_t* lv, int N, int C, int P) {
  Segs sg{};
  if (pearson_plan(sg, lv, N, C, P)) return 0;
  return ldeval::align_up((size_t)N * sg.L * C * sizeof(double)) + 256;
}

int ld_levels_pearson(const ld_levels_t* lv, const float* t, const float* s, int N, int C,
                      int P, double* r_sum, int32_t* counts, void* workspace,
                      size_t workspace_bytes, ld_stream_t stream_) {
  Segs sg{};
  const int rc = pearson_plan(sg, lv, N, C, P);
  if (rc) return rc;
  if (!t || !s || !r_sum || !counts) return LD_EINVAL;
  const size_t need = (size_t)N * sg.L * C * sizeof(double);
  if (!workspace || workspace_bytes < need) return LD_ENOSPACE;
  if ((uintptr_t)workspace & 7) return LD_EINVAL;  // doubles inside
  double* rtab = (double*)workspace;
  LD_LAUNCH(levels_pearson_kernel, dim3(sg.total), dim3(kThreads), 0, (hipStream_t)stream_, t,
            s, N * C, C, sg, rtab);
  LD_LAUNCH(levels_pearson_sum_kernel, dim3(N * sg.L), dim3(64), 0, (hipStream_t)stream_,
            (const double*)rtab, C, r_sum, counts);
  return (int)hipGetLastError();
}

}  // extern "C"
