// What the evaluation sources share (eval.hip, eval_image.hip, coco_eval.hip,
// recall.hip, landscape.hip): the image lookup, the score key, the block scan,
// the stable LSD radix sort with its host driver, and the workspace carving.
// Include only from files compiled with -ffp-contract=off.  Everything with a
// kernel in it sits in an anonymous namespace: each including file gets its own
// copy with internal linkage.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "ld_launch.h"

namespace ldeval {

// ------------------------------------------------------- workspace ------
inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// carves a workspace into 256-byte aligned pieces: take() returns the offset of
// the next piece, `off` is the size of everything taken so far
struct Carver {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t at = off;
    off += align_up(bytes);
    return at;
  }
};

namespace {

constexpr int kScanThreads = 256;  // 4 waves of 64
constexpr int kScanItems = 16;
constexpr int kScanTile = kScanThreads * kScanItems;
constexpr int kRadixBits = 8;
constexpr int kBins = 1 << kRadixBits;

// last b with off[b] <= i (images may be empty)
__device__ __forceinline__ int find_img(const int32_t* off, int num_imgs, int i) {
  int lo = 0, hi = num_imgs - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// a score as an unsigned key ascending with it, a strict total order:
// sign-flipped bits, 0.0 and -0.0 one score, NaN past every number of its sign
__device__ __forceinline__ uint32_t order_key(float s) {
  const uint32_t u = __float_as_uint(s == 0.0f ? 0.0f : s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// descending score as an ascending key: ~order_key(s), with the NOT taken into
// both arms (the compiler does not do that through the inlined call)
__device__ __forceinline__ uint32_t desc_key(float s) {
  const uint32_t u = __float_as_uint(s == 0.0f ? 0.0f : s);
  return (u & 0x80000000u) ? u : (u ^ 0x7fffffffu);
}

// exclusive prefix sum of a 256-thread block; *total gets the block's sum
__device__ __forceinline__ int block_excl_scan(int v, int* sh, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
  for (int off = 1; off < 64; off <<= 1) {
    int y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) sh[w] = x;
  __syncthreads();
  int pre = 0, tot = 0;
  for (int k = 0; k < kScanThreads / 64; ++k) {
    if (k < w) pre += sh[k];
    tot += sh[k];
  }
  __syncthreads();
  *total = tot;
  return pre + x - v;
}

// in place exclusive scan of m ints, one workgroup per row (blockIdx.y); a
// template so that only the files that launch it carry it
template <typename T>
__global__ __launch_bounds__(kScanThreads) void excl_scan_kernel(T* data, int m) {
  __shared__ int sh[kScanThreads / 64];
  T* row = data + (size_t)blockIdx.y * m;
  int carry = 0;
  for (int base = 0; base < m; base += kScanTile) {
    const int i0 = base + threadIdx.x * kScanItems;
    int v[kScanItems], s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
      v[k] = (i0 + k < m) ? row[i0 + k] : 0;
      s += v[k];
    }
    int tot;
    int run = carry + block_excl_scan(s, sh, &tot);
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
      if (i0 + k < m) {
        row[i0 + k] = run;
        run += v[k];
      }
    carry += tot;
  }
}

// ------------------------------------------------------------ sort ------
// Stable LSD radix sort of (hi, lo) keys with a 32-bit value: 8-bit digits, one
// kScanTile-element tile per workgroup, the digits of lo first (LOW only), then
// those of hi from its least significant byte.
template <bool LOW>
struct SortKeys;

template <>
struct SortKeys<false> {  // 64-bit key
  uint64_t* hi;
  __device__ uint32_t low(int) const { return 0u; }
  __device__ void set_low(int, uint32_t) const {}
};

template <>
struct SortKeys<true> {  // 64-bit key over a 32-bit low word
  uint64_t* hi;
  uint32_t* lo;
  __device__ uint32_t low(int i) const { return lo[i]; }
  __device__ void set_low(int i, uint32_t v) const { lo[i] = v; }
};

template <bool LOW>
__device__ __forceinline__ int digit_of(uint64_t hi, uint32_t lo, int pass, int lo_passes) {
  if (LOW && pass < lo_passes) return (int)((lo >> (pass * kRadixBits)) & (kBins - 1));
  return (int)((hi >> ((pass - lo_passes) * kRadixBits)) & (kBins - 1));
}

template <bool LOW>
__global__ __launch_bounds__(kScanThreads) void radix_hist_kernel(SortKeys<LOW> in, int n,
                                                                 int pass, int lo_passes,
                                                                 int nb, int32_t* hist) {
  __shared__ int h[kBins];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int base = blockIdx.x * kScanTile;
  for (int c = 0; c < kScanItems; ++c) {
    const int i = base + c * kScanThreads + threadIdx.x;
    if (i < n) atomicAdd(&h[digit_of<LOW>(in.hi[i], in.low(i), pass, lo_passes)], 1);
  }
  __syncthreads();
  hist[threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];
}

// stable scatter: element order = (chunk, wave, lane), so ranks inside a wave
// from the ballot match mask keep equal digits in input order
template <bool LOW>
__global__ __launch_bounds__(kScanThreads) void radix_scatter_kernel(
    SortKeys<LOW> in, const uint32_t* vin, SortKeys<LOW> out, uint32_t* vout, int n,
    int pass, int lo_passes, int nb, const int32_t* hist) {
  __shared__ int base[kBins];
  __shared__ int wcnt[kScanThreads / 64][kBins];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  base[tid] = hist[tid * nb + blockIdx.x];
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  for (int c = 0; c < kScanItems; ++c) {
    const int i = blockIdx.x * kScanTile + c * kScanThreads + tid;
    const bool valid = i < n;
    for (int k = 0; k < kScanThreads / 64; ++k) wcnt[k][tid] = 0;
    __syncthreads();
    const uint64_t h = valid ? in.hi[i] : 0ull;
    const uint32_t l = valid ? in.low(i) : 0u, v = valid ? vin[i] : 0u;
    const int dig = digit_of<LOW>(h, l, pass, lo_passes);
    uint64_t mask = __ballot(valid);
#pragma unroll
    for (int bt = 0; bt < kRadixBits; ++bt) {
      const bool on = (dig >> bt) & 1;
      const uint64_t m = __ballot(valid && on);
      mask &= on ? m : ~m;
    }
    const int rank = __popcll(mask & lt);
    if (valid && rank == 0) wcnt[w][dig] = __popcll(mask);
    __syncthreads();
    int run = base[tid];
    for (int k = 0; k < kScanThreads / 64; ++k) {
      const int x = wcnt[k][tid];
      wcnt[k][tid] = run;
      run += x;
    }
    base[tid] = run;
    __syncthreads();
    if (valid) {
      const int dst = wcnt[w][dig] + rank;
      out.hi[dst] = h;
      out.set_low(dst, l);
      vout[dst] = v;
    }
    __syncthreads();
  }
}

inline int sort_tiles(int n) { return (n + kScanTile - 1) / kScanTile; }

// lo_passes + hi_passes rounds of hist -> scan -> scatter over the ping-pong
// buffers keys[2] / vals[2], starting from [0]; hist holds kBins * sort_tiles(n)
// ints.  Returns the index of the buffers that hold the sorted records.
template <bool LOW>
int radix_sort(const SortKeys<LOW> (&keys)[2], uint32_t* const (&vals)[2], int n,
               int lo_passes, int hi_passes, int32_t* hist, hipStream_t stream) {
  const int nb = sort_tiles(n);
  int cur = 0;
  for (int pass = 0; pass < lo_passes + hi_passes; ++pass) {
    LD_LAUNCH(radix_hist_kernel<LOW>, dim3(nb), dim3(kScanThreads), 0, stream, keys[cur], n,
              pass, lo_passes, nb, hist);
    LD_LAUNCH(excl_scan_kernel<int32_t>, dim3(1), dim3(kScanThreads), 0, stream, hist,
              kBins * nb);
    LD_LAUNCH(radix_scatter_kernel<LOW>, dim3(nb), dim3(kScanThreads), 0, stream, keys[cur],
              (const uint32_t*)vals[cur], keys[cur ^ 1], vals[cur ^ 1], n, pass, lo_passes,
              nb, (const int32_t*)hist);
    cur ^= 1;
  }
  return cur;
}

}  // namespace
}  // namespace ldeval
