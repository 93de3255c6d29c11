// Proposal recall on gfx950: the reference's eval_recalls / _recalls
// (core/evaluation/recall.py:10-40, 83-103).
//
// Replaces (reference file:line)
//   score sort, cap at proposal_nums[-1], GT x proposal IoU   recall.py:88-101
//   bbox_overlaps (fp32)                         core/evaluation/bbox_overlaps.py
//   greedy GT <-> proposal matching per proposal budget       recall.py:16-33
//   recalls = count(iou >= thr) / total_gt                    recall.py:35-38
//
// recall_match_kernel: one workgroup of 256 threads per image, nothing leaves
// the workgroup:
//   1. order   one thread per proposal, by counting: its position in descending
//              score order (equal scores: the later index first).  Only the
//              first Kc = min(k, proposal_nums[-1]) positions are kept.
//   2. iou     the G x Kc tile, GT rows, proposals in sorted order, fp32 in the
//              reference's op order (ldeval::iou_ref).
//   3. match   per budget p the prefix of kp = min(Kc, nums[p]) columns and
//              min(G, kp) rounds.  A round takes the live GT with the largest
//              row maximum (lowest GT on ties), records that IoU, and kills the
//              row and its argmax column (lowest column on ties).  The tile is
//              never written: dead rows / columns are flags, which is the
//              reference's "-1" since a live IoU is >= 0.  Every round takes
//              the maxima of the live rows anew, one wave per row.  Rounds past
//              kp record -1 (every column is dead), a budget with no column
//              records 0.
// The tile, the order and the flags sit in LDS when they fit (kTile floats,
// kMaxK columns, kMaxG rows); otherwise, or with LD_EVAL_RECALLS_NO_LDS, in the
// caller's workspace.  Same code, pointers chosen once, same bits.
//
// recall_count_kernel: one workgroup per budget: integer counts of
// (double)iou >= thr per threshold, then count / total_gt in float64.
// No float atomics; every output has one writer.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/ld_hip.h"
#include "eval_common.h"
#include "eval_iou.h"
#include "ld_launch.h"

namespace {

using ldeval::box_area;
using ldeval::iou_ref;
using ldeval::order_key;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 12288;  // IoU tile floats held in LDS (48 KiB)
constexpr int kMaxK = 1024;   // kept proposals of an image held in LDS
constexpr int kMaxG = 256;    // GTs of an image held in LDS

struct RecallParams {
  int nums[LD_EVAL_RECALLS_MAX_NUMS];
  int P, cols, cap_k, no_lds;
  long long stride, base;  // gt_ious row stride and first column of the batch
};

// workspace of the route that does not fit LDS, in bytes of the whole batch
struct RecallPlan {
  size_t tile, order, dead, rmax, rarg, rdead, total;
};

RecallPlan recall_plan(long long num_props, long long num_gts, long long cap_k) {
  RecallPlan o{};
  ldeval::Carver ws;
  o.tile = ws.take((size_t)num_gts * (size_t)cap_k * 4);
  o.order = ws.take((size_t)num_props * 4);
  o.dead = ws.take((size_t)num_props);
  o.rmax = ws.take((size_t)num_gts * 4);
  o.rarg = ws.take((size_t)num_gts * 4);
  o.rdead = ws.take((size_t)num_gts);
  o.total = ws.off;
  return o;
}

// maximum and lowest column holding it over the live columns [0, kp) of a row;
// the whole wave calls it, every lane returns the result.  arg = -1: no live
// column.
__device__ __forceinline__ void row_max(const float* row, const uint8_t* dead, int kp,
                                        int lane, float& best, int& arg) {
  float b = -1.0f;
  int a = -1;
  for (int c = lane; c < kp; c += 64) {
    if (dead[c]) continue;
    const float v = row[c];
    if (a < 0 || v > b) b = v, a = c;  // ascending c: the first maximum stays
  }
  for (int off = 32; off > 0; off >>= 1) {
    const float ob = __shfl_xor(b, off, 64);
    const int oa = __shfl_xor(a, off, 64);
    if (oa >= 0 && (a < 0 || ob > b || (ob == b && oa < a))) b = ob, a = oa;
  }
  best = b;
  arg = a;
}

__global__ __launch_bounds__(kThreads) void recall_match_kernel(
    const float* props, const int32_t* prop_off, const float* gts, const int32_t* gt_off,
    RecallParams p, RecallPlan plan, char* ws, float* gt_ious) {
  __shared__ float s_tile[kTile];
  __shared__ int s_order[kMaxK];
  __shared__ uint8_t s_dead[kMaxK];
  __shared__ float s_rmax[kMaxG];
  __shared__ int s_rarg[kMaxG];
  __shared__ uint8_t s_rdead[kMaxG];

  const int img = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int d0 = prop_off[img], K = prop_off[img + 1] - d0;
  const int g0 = gt_off[img], G = gt_off[img + 1] - g0;
  if (G <= 0) return;  // recall.py:97-98: no row of the table is this image's
  const int cols = p.cols;
  const int Kc = min(min(K, p.nums[p.P - 1]), p.cap_k);
  const bool fast = !p.no_lds && Kc <= kMaxK && G <= kMaxG &&
                    (long long)G * Kc <= (long long)kTile;

  float* tile = fast ? s_tile : (float*)(ws + plan.tile) + (size_t)g0 * p.cap_k;
  int* order = fast ? s_order : (int*)(ws + plan.order) + d0;
  uint8_t* dead = fast ? s_dead : (uint8_t*)(ws + plan.dead) + d0;
  float* rmax = fast ? s_rmax : (float*)(ws + plan.rmax) + g0;
  int* rarg = fast ? s_rarg : (int*)(ws + plan.rarg) + g0;
  uint8_t* rdead = fast ? s_rdead : (uint8_t*)(ws + plan.rdead) + g0;
  const float* pr = props + (size_t)d0 * cols;
  const float* gt = gts + (size_t)g0 * 4;

  // ---- 1. order
  if (cols == 5 && Kc > 0) {
    // the keys pass through the tile's LDS, which is idle until step 2, kTile at
    // a time; a thread counts for one proposal of each group of kThreads
    uint32_t* s_key = (uint32_t*)s_tile;
    for (int i0 = 0; i0 < K; i0 += kThreads) {
      const int i = i0 + tid;
      const uint32_t ki = i < K ? order_key(pr[(size_t)i * 5 + 4]) : 0u;
      int pos = 0;
      for (int c0 = 0; c0 < K; c0 += kTile) {
        const int n = min(kTile, K - c0);
        if (i0 == 0 || K > kTile) {  // one chunk stays; more are staged again
          __syncthreads();
          for (int j = tid; j < n; j += kThreads)
            s_key[j] = order_key(pr[(size_t)(c0 + j) * 5 + 4]);
          __syncthreads();
        }
        if (i < K)
          for (int j = 0; j < n; ++j) {
            const uint32_t kj = s_key[j];
            pos += (kj > ki || (kj == ki && c0 + j > i)) ? 1 : 0;
          }
      }
      if (i < K && pos < Kc) order[pos] = i;
    }
  } else {
    for (int i = tid; i < Kc; i += kThreads) order[i] = i;
  }
  __syncthreads();

  // ---- 2. IoU tile
  for (int k = tid; k < G * Kc; k += kThreads) {
    const int g = k / Kc, c = k - g * Kc;
    const float* b = pr + (size_t)order[c] * cols;
    tile[k] = iou_ref(b, box_area(b), gt + g * 4);
  }
  __syncthreads();

  // ---- 3. greedy matching of every budget
  for (int q = 0; q < p.P; ++q) {
    float* out = gt_ious + (size_t)q * p.stride + p.base + g0;
    const int kp = min(Kc, p.nums[q]);
    const int rounds = min(G, kp);
    // recall.py:20-23 (no column: zeros); rounds past the last live column
    for (int j = tid; j < G; j += kThreads)
      if (j >= rounds) out[j] = kp > 0 ? -1.0f : 0.0f;
    if (kp <= 0) continue;
    for (int c = tid; c < kp; c += kThreads) dead[c] = 0;
    for (int g = tid; g < G; g += kThreads) rdead[g] = 0;
    __syncthreads();
    for (int j = 0; j < rounds; ++j) {
      for (int g = w; g < G; g += kWaves) {  // one wave per live row
        if (rdead[g]) continue;              // wave-uniform
        float b;
        int a;
        row_max(tile + (size_t)g * Kc, dead, kp, lane, b, a);
        if (lane == 0) rmax[g] = b, rarg[g] = a;
      }
      __syncthreads();
      if (w == 0) {  // the live GT with the largest maximum, lowest on ties
        float b = -1.0f;
        int a = -1;
        for (int g = lane; g < G; g += 64) {
          if (rdead[g]) continue;
          const float v = rmax[g];
          if (a < 0 || v > b) b = v, a = g;
        }
        for (int off = 32; off > 0; off >>= 1) {
          const float ob = __shfl_xor(b, off, 64);
          const int oa = __shfl_xor(a, off, 64);
          if (oa >= 0 && (a < 0 || ob > b || (ob == b && oa < a))) b = ob, a = oa;
        }
        if (lane == 0) {  // j < min(G, kp): a live row with a live column exists
          const int box = a >= 0 ? rarg[a] : -1;
          out[j] = b;
          if (a >= 0) rdead[a] = 1;
          if (box >= 0) dead[box] = 1;
        }
      }
      __syncthreads();
    }
  }
}

struct CountParams {
  double thr[LD_EVAL_MAX_THRS];
  int T;
  long long total, stride;
};

__global__ __launch_bounds__(kThreads) void recall_count_kernel(const float* gt_ious,
                                                               CountParams p,
                                                               double* recalls) {
  __shared__ int s_cnt[kWaves][LD_EVAL_MAX_THRS];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* row = gt_ious + (size_t)q * p.stride;
  int cnt[LD_EVAL_MAX_THRS];
#pragma unroll
  for (int t = 0; t < LD_EVAL_MAX_THRS; ++t) cnt[t] = 0;
  for (long long g = tid; g < p.total; g += kThreads) {
    const double v = (double)row[g];
#pragma unroll
    for (int t = 0; t < LD_EVAL_MAX_THRS; ++t)
      if (t < p.T) cnt[t] += v >= p.thr[t] ? 1 : 0;
  }
#pragma unroll
  for (int t = 0; t < LD_EVAL_MAX_THRS; ++t) {
    int c = cnt[t];
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if (lane == 0) s_cnt[w][t] = c;
  }
  __syncthreads();
  if (tid < p.T) {
    int c = 0;
    for (int k = 0; k < kWaves; ++k) c += s_cnt[k][tid];
    // total_gt == 0: 0 / 0 = NaN, as the reference's division gives
    recalls[(size_t)q * p.T + tid] = (double)c / (double)p.total;
  }
}

int fill_nums(RecallParams& p, int num_nums, const int32_t* nums) {
  if (!nums || num_nums < 1 || num_nums > LD_EVAL_RECALLS_MAX_NUMS) return LD_EINVAL;
  for (int i = 0; i < num_nums; ++i) {
    if (nums[i] < 0) return LD_EINVAL;
    p.nums[i] = nums[i];
  }
  p.P = num_nums;
  return 0;
}

}  // namespace

extern "C" {

size_t ld_eval_recalls_workspace_bytes(int num_props, int num_gts, int max_img_props,
                                       int cap) {
  if (num_props < 0 || num_gts < 0 || max_img_props < 0 || cap < 0) return 0;
  const int cap_k = max_img_props < cap ? max_img_props : cap;
  return recall_plan(num_props, num_gts, cap_k).total + 256;
}

int ld_eval_recalls_match(const float* props, int prop_cols, const int32_t* prop_off,
                          const float* gts, const int32_t* gt_off, int num_imgs,
                          int num_props, int num_gts, int max_img_props, int num_nums,
                          const int32_t* proposal_nums, int flags, float* gt_ious,
                          long long gt_stride, long long gt_base, void* workspace,
                          size_t workspace_bytes, ld_stream_t stream_) {
  if (prop_cols != 4 && prop_cols != 5) return LD_EINVAL;
  if (flags & ~LD_EVAL_RECALLS_NO_LDS) return LD_EINVAL;
  if (num_imgs < 0 || num_props < 0 || num_gts < 0 || max_img_props < 0) return LD_EINVAL;
  if (max_img_props > num_props || gt_base < 0 || gt_stride < 0) return LD_EINVAL;
  RecallParams p{};
  const int rc = fill_nums(p, num_nums, proposal_nums);
  if (rc) return rc;
  if (num_imgs == 0 || num_gts == 0) return 0;
  if (!prop_off || !gt_off || !gts || !gt_ious) return LD_EINVAL;
  if (num_props && !props) return LD_EINVAL;
  if (gt_base + num_gts > gt_stride) return LD_EINVAL;
  if ((long long)num_props * prop_cols >= (1ll << 31)) return LD_EUNSUPPORTED;
  p.cols = prop_cols;
  p.cap_k = max_img_props < p.nums[p.P - 1] ? max_img_props : p.nums[p.P - 1];
  p.no_lds = (flags & LD_EVAL_RECALLS_NO_LDS) ? 1 : 0;
  p.stride = gt_stride;
  p.base = gt_base;
  const RecallPlan plan = recall_plan(num_props, num_gts, p.cap_k);
  if (workspace_bytes < plan.total || !workspace) return LD_ENOSPACE;
  if ((uintptr_t)workspace & 3) return LD_EINVAL;  // float / int arrays inside
  LD_LAUNCH(recall_match_kernel, dim3(num_imgs), dim3(kThreads), 0, (hipStream_t)stream_,
            props, prop_off, gts, gt_off, p, plan, (char*)workspace, gt_ious);
  return (int)hipGetLastError();
}

int ld_eval_recalls_count(const float* gt_ious, long long gt_stride, long long total_gt,
                          int num_nums, int num_thrs, const double* iou_thrs,
                          double* recalls, ld_stream_t stream_) {
  if (num_nums < 1 || num_nums > LD_EVAL_RECALLS_MAX_NUMS) return LD_EINVAL;
  if (num_thrs < 1 || num_thrs > LD_EVAL_MAX_THRS || !iou_thrs || !recalls)
    return LD_EINVAL;
  if (total_gt < 0 || gt_stride < total_gt) return LD_EINVAL;
  if (total_gt >= (1ll << 31)) return LD_EUNSUPPORTED;
  if (total_gt && !gt_ious) return LD_EINVAL;
  CountParams p{};
  p.T = num_thrs;
  p.total = total_gt;
  p.stride = gt_stride;
  for (int t = 0; t < num_thrs; ++t) p.thr[t] = iou_thrs[t];
  LD_LAUNCH(recall_count_kernel, dim3(num_nums), dim3(kThreads), 0, (hipStream_t)stream_,
            gt_ious, p, recalls);
  return (int)hipGetLastError();
}

}  // extern "C"
