// The optimizer of a config's training recipe on gfx950 (mmcv 1.2
// DefaultOptimizerConstructor + OptimizerHook, restated by ld_amd.optim):
//
//   ld_sgd_step_classes  torch.optim.SGD over the flat arena with (lr, wd) from
//                        a per-class table (paramwise_cfg: bias_lr_mult,
//                        bias_decay_mult, norm_decay_mult, custom_keys, ...);
//                        the class of an element is the uint8 id of its
//                        64-float chunk (train.GradArena aligns every parameter
//                        to 64 floats, so a chunk never spans two parameters)
//   ld_grad_norm         torch.nn.utils.clip_grad_norm_(max_norm, norm_type=2)
//                        of the averaged gradient: [total_norm, clip_coef]
//
//   ld_vrank_reduce      the cross-rank mean of a virtual-rank step
//                        (train.SGDTrainer(virtual_ranks=W)): a (W, n) table of
//                        per-rank values -> their ascending-order fp32 sum / W,
//                        what all_reduce(SUM) + div_(world) leaves on every rank
//
// The first two are HBM-bound single passes.  Everything that may change between
// replays of a captured step (momentum, 1/world, the class table, max_norm, the
// clip coefficient) is read from device memory.  Compiled with the default
// contraction, like nn.hip: with one class and clip_coef == 1 the update is
// bit-identical to sgd_kernel / sgd_dev_kernel.
#include <hip/hip_runtime.h>

#include "ld_launch.h"
#include "ld_math.h"

#include "../../include/ld_hip.h"

namespace {

constexpr size_t kChunk = 64;     // floats per class id (GradArena align)
constexpr int kNormBlocks = 1024; // fixed grid: a fixed summation order
constexpr int kNormThreads = 256;

// hyper layout (include/ld_hip.h): [momentum, grad_scale, max_norm, 0,
//                                   lr_0, wd_0, lr_1, wd_1, ...]
constexpr int kHyperHead = 4;

__global__ __launch_bounds__(256) void sgd_classes_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
    size_t n, const uint8_t* __restrict__ chunk_class, int num_classes,
    const float* __restrict__ hyper, const float* __restrict__ clip) {
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  const float mu = hyper[0];
  // the gradient scale: 1/world, times the clip coefficient when clipping
  const float s = clip ? hyper[1] * clip[1] : hyper[1];
  // the 4 elements of a thread share one 64-float chunk
  int c = chunk_class[i / kChunk];
  c = c < num_classes ? c : num_classes - 1;
  const float lr = hyper[kHyperHead + 2 * c], wd = hyper[kHyperHead + 2 * c + 1];
  if (i + 3 < n) {
    float4 pv = *reinterpret_cast<float4*>(p + i);
    const float4 gv = *reinterpret_cast<const float4*>(g + i);
    float4 bv = *reinterpret_cast<float4*>(buf + i);
    bv.x = mu * bv.x + (gv.x * s + wd * pv.x);
    bv.y = mu * bv.y + (gv.y * s + wd * pv.y);
    bv.z = mu * bv.z + (gv.z * s + wd * pv.z);
    bv.w = mu * bv.w + (gv.w * s + wd * pv.w);
    pv.x -= lr * bv.x; pv.y -= lr * bv.y; pv.z -= lr * bv.z; pv.w -= lr * bv.w;
    *reinterpret_cast<float4*>(p + i) = pv;
    *reinterpret_cast<float4*>(buf + i) = bv;
  } else {
    for (size_t k = i; k < n; ++k) {
      const float b = mu * buf[k] + (g[k] * s + wd * p[k]);
      buf[k] = b;
      p[k] -= lr * b;
    }
  }
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// block-wide sum (256 threads) in a fixed order, valid in thread 0
__device__ __forceinline__ double block_sum(double v) {
  __shared__ double part[kNormThreads / 64];
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kNormThreads / 64; ++w) s += part[w];
  return s;
}

// stage 1: sum of squares in fp64, one partial per block of the fixed grid
__global__ __launch_bounds__(kNormThreads) void grad_sq_partial_kernel(
    const float* __restrict__ g, size_t n, double* __restrict__ partial) {
  const size_t n4 = n / 4;
  const size_t stride = (size_t)kNormBlocks * kNormThreads;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  double acc = 0.0;
  for (size_t v = (size_t)blockIdx.x * kNormThreads + threadIdx.x; v < n4;
       v += stride) {
    const float4 x = g4[v];
    acc += (double)x.x * (double)x.x + (double)x.y * (double)x.y +
           (double)x.z * (double)x.z + (double)x.w * (double)x.w;
  }
  if (blockIdx.x == 0 && threadIdx.x < n - 4 * n4) {
    const double x = g[4 * n4 + threadIdx.x];
    acc += x * x;
  }
  const double s = block_sum(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// stage 2: one block sums the partials in a fixed order; torch's
// clip_grad_norm_ coefficient in fp32: min(1, max_norm / (total + 1e-6))
__global__ __launch_bounds__(kNormThreads) void grad_norm_final_kernel(
    const double* __restrict__ partial, const float* __restrict__ hyper,
    float* __restrict__ out) {
  double acc = 0.0;
  for (int b = threadIdx.x; b < kNormBlocks; b += kNormThreads) acc += partial[b];
  const double ss = block_sum(acc);
  if (threadIdx.x == 0) {
    const float total = (float)((double)hyper[1] * sqrt(ss));
    const float coef = hyper[2] / (total + 1e-6f);
    out[0] = total;
    out[1] = coef > 1.0f ? 1.0f : coef;  // a NaN norm stays NaN, as in torch
  }
}

// One thread per column; every lane of the launch runs the same W iterations (W is
// a kernel argument: a wave-uniform trip count, no divergence), each a coalesced
// read of one table row.  n is 2 (the loss normalisers) or ~9 (the logged values):
// a single 64-lane workgroup in practice, bound by its launch, so nothing is staged
// or vectorised.  Rank order and the IEEE division are the result's definition.
__global__ __launch_bounds__(64) void vrank_reduce_kernel(
    const float* __restrict__ table, int W, int n, size_t row_stride,
    float* __restrict__ out) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= n) return;
  out[c] = ld::vrank_mean(table + c, W, row_stride);
}

}  // namespace

extern "C" int ld_vrank_reduce(const float* table, int W, int n, size_t row_stride,
                               float* out, ld_stream_t stream) {
  if (!table || !out || W < 1 || n < 1 || row_stride < (size_t)n) return LD_EINVAL;
  LD_LAUNCH(vrank_reduce_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0,
            (hipStream_t)stream, table, W, n, row_stride, out);
  return (int)hipGetLastError();
}

extern "C" int ld_sgd_step_classes(float* params, const float* grads,
                                   float* momentum_buf, size_t n,
                                   const uint8_t* chunk_class, int num_classes,
                                   const float* hyper, const float* clip,
                                   ld_stream_t stream) {
  if (!params || !grads || !momentum_buf || !chunk_class || !hyper ||
      num_classes < 1 || num_classes > LD_SGD_MAX_CLASSES)
    return LD_EINVAL;
  if (n == 0) return 0;
  if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)momentum_buf) % 16)
    return LD_EINVAL;
  const size_t threads = (n + 3) / 4;
  LD_LAUNCH(sgd_classes_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256),
            0, (hipStream_t)stream, params, grads, momentum_buf, n, chunk_class,
            num_classes, hyper, clip);
  return (int)hipGetLastError();
}

extern "C" size_t ld_grad_norm_workspace_bytes(void) {
  return (size_t)kNormBlocks * sizeof(double);
}

extern "C" int ld_grad_norm(const float* grads, size_t n, const float* hyper,
                            float* out, void* workspace, size_t workspace_bytes,
                            ld_stream_t stream) {
  if (!grads || !hyper || !out || !workspace) return LD_EINVAL;
  if (workspace_bytes < ld_grad_norm_workspace_bytes()) return LD_ENOSPACE;
  if (((uintptr_t)grads % 16) || ((uintptr_t)workspace % 8)) return LD_EINVAL;
  double* partial = (double*)workspace;
  LD_LAUNCH(grad_sq_partial_kernel, dim3(kNormBlocks), dim3(kNormThreads), 0,
            (hipStream_t)stream, grads, n, partial);
  LD_LAUNCH(grad_norm_final_kernel, dim3(1), dim3(kNormThreads), 0,
            (hipStream_t)stream, (const double*)partial, hyper, out);
  return (int)hipGetLastError();
}
