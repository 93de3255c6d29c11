// Detection mAP evaluation on gfx950: TP/FP per detection and the per-class
// precision / recall / AP of every IoU threshold and scale range, on the device.
//
// Replaces (reference file:line)
//   tpfp_default           core/evaluation/mean_ap.py:153-237
//   get_cls_results        core/evaluation/mean_ap.py:240-264
//   eval_map (num_gts, sort, cumsum, recall/precision)  mean_ap.py:320-342
//   average_precision      core/evaluation/mean_ap.py:12-55 ('area', '11points')
//   bbox_overlaps          core/evaluation/bbox_overlaps.py (fp32, eps 1e-6)
//
// Integer / fp32 work bound by memory traffic and, for the sort, by passes:
//   1. match    one thread per detection: IoU against the same-class GTs then
//               ignored GTs of its image, fp32 in the reference's op order
//               (compiled with -ffp-contract=off), first maximum wins
//   2. decide   one thread per (detection, IoU threshold): the greedy loop of
//               tpfp_default is not sequential in disguise.  gt_covered is set
//               only by matched detections, so detection i is TP exactly when
//               no detection before it in score order (descending score, ties
//               by position in the class array) has the same argmax GT and
//               ious_max >= thr.  O(dets per image) per thread.
//               Records (score, segment = thr * C + class, TP/FP bits per scale)
//               land in image-major order, which is np.vstack order per class.
//   3. sort     stable LSD radix sort of (segment << 32 | descending score):
//               8-bit digits, one 4096-element tile per workgroup, ranks inside
//               a wave from 8 ballots.  Segments of any length (VOC07 test has
//               ~500k detections in one class).
//   4. scan     inclusive int32 scan of every TP / FP bit over all records;
//               the value before a segment's first record is subtracted.
//   5. ap       one workgroup per (segment, scale): suffix-max envelope walked
//               from the end in tiles, float64 sum; or the 11-point maxima.
#include <hip/hip_runtime.h>

#include <float.h>
#include <stdint.h>

#include "../../include/ld_hip.h"
#include "eval_common.h"
#include "eval_iou.h"
#include "ld_launch.h"

namespace {

using ldeval::block_excl_scan;
using ldeval::box_area;
using ldeval::desc_key;
using ldeval::excl_scan_kernel;
using ldeval::find_img;
using ldeval::iou_ref;

constexpr int kThreads = ldeval::kScanThreads;  // 4 waves of 64
constexpr int kItems = ldeval::kScanItems;
constexpr int kTile = ldeval::kScanTile;  // the sort's tile as well
constexpr int kTpShift = 0;   // TP of scale k: bit k
constexpr int kFpShift = 16;  // FP of scale k: bit 16 + k

struct EvalParams {
  float lo[LD_EVAL_MAX_SCALES], hi[LD_EVAL_MAX_SCALES];
  float thr[LD_EVAL_MAX_THRS];
  int C, S, T, has_ranges;
  int num_imgs, num_gts;
};

__global__ void eval_match_kernel(ld_eval_batch_t b, EvalParams p, float* iou_max,
                                  int* argmax) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.num_dets) return;
  int img = find_img(b.det_off, b.num_imgs, i);
  int64_t lab = b.det_labels[i];
  float best = 0.0f;
  int arg = -1;
  if (lab >= 0 && lab < p.C) {
    const float* d = b.dets + (size_t)i * 5;
    float ad = box_area(d);
    for (int j = b.gt_off[img]; j < b.gt_off[img + 1]; ++j) {
      if (b.gt_labels[j] != lab) continue;
      float v = iou_ref(d, ad, b.gts + (size_t)j * 4);
      if (arg < 0 || v > best) best = v, arg = j;
    }
    for (int j = b.ign_off[img]; j < b.ign_off[img + 1]; ++j) {
      if (b.ign_labels[j] != lab) continue;
      float v = iou_ref(d, ad, b.ign + (size_t)j * 4);
      if (arg < 0 || v > best) best = v, arg = b.num_gts + j;
    }
  }
  iou_max[i] = best;
  argmax[i] = arg;
}

__global__ void eval_decide_kernel(ld_eval_batch_t b, EvalParams p, const float* iou_max,
                                   const int* argmax, float* rec_score, int32_t* rec_seg,
                                   uint32_t* rec_bits) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= b.num_dets * p.T) return;
  int i = idx / p.T, t = idx - i * p.T;
  const float* d = b.dets + (size_t)i * 5;
  float score = d[4];
  int64_t lab = b.det_labels[i];
  rec_score[idx] = score;
  if (lab < 0 || lab >= p.C) {  // no class array holds it: sorts past every segment
    rec_seg[idx] = p.T * p.C;
    rec_bits[idx] = 0u;
    return;
  }
  rec_seg[idx] = t * p.C + (int)lab;
  const float thr = p.thr[t];
  const int arg = argmax[i];
  const bool matched = arg >= 0 && iou_max[i] >= thr;
  const int S = p.has_ranges ? p.S : 1;
  uint32_t bits = 0u;
  if (!matched) {
    float ad = box_area(d);
    for (int k = 0; k < S; ++k)
      if (!p.has_ranges || (ad >= p.lo[k] && ad < p.hi[k])) bits |= 1u << (kFpShift + k);
  } else if (arg < b.num_gts) {  // a matched ignored GT gives neither
    // covered: an earlier detection (score order, stable) took the same GT
    int img = find_img(b.det_off, b.num_imgs, i);
    bool covered = false;
    for (int j = b.det_off[img]; j < b.det_off[img + 1] && !covered; ++j) {
      if (j == i || b.det_labels[j] != lab || argmax[j] != arg) continue;
      float sj = b.dets[(size_t)j * 5 + 4];
      bool before = sj > score || (sj == score && j < i);
      covered = before && iou_max[j] >= thr;
    }
    float ag = box_area(b.gts + (size_t)arg * 4);
    for (int k = 0; k < S; ++k) {
      if (p.has_ranges && (ag < p.lo[k] || ag >= p.hi[k])) continue;
      bits |= 1u << ((covered ? kFpShift : kTpShift) + k);
    }
  }
  rec_bits[idx] = bits;
}

// mean_ap.py:320-330: ignored GTs are not counted, nor GTs out of range
__global__ void eval_count_gts_kernel(ld_eval_batch_t b, EvalParams p, int32_t* num_gts) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= b.num_gts) return;
  int64_t lab = b.gt_labels[j];
  if (lab < 0 || lab >= p.C) return;
  if (!p.has_ranges) {
    atomicAdd(num_gts + lab * p.S, 1);
    return;
  }
  float a = box_area(b.gts + (size_t)j * 4);
  for (int k = 0; k < p.S; ++k)
    if (a >= p.lo[k] && a < p.hi[k]) atomicAdd(num_gts + lab * p.S + k, 1);
}

// ------------------------------------------------------------ sort ------
__global__ void eval_keys_kernel(int n, const float* score, const int32_t* seg,
                                 const uint32_t* bits, int num_segs, uint64_t* keys,
                                 uint32_t* vals) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t s = (uint32_t)min(max(seg[i], 0), num_segs);
  keys[i] = ((uint64_t)s << 32) | desc_key(score[i]);
  vals[i] = bits[i];
}

__global__ void seg_start_kernel(const uint64_t* keys, int n, int num_segs,
                                 int32_t* seg_start) {
  int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > num_segs) return;
  int lo = 0, hi = n;  // first record whose segment >= s
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if ((int)(keys[mid] >> 32) < s) lo = mid + 1;
    else hi = mid;
  }
  seg_start[s] = lo;
}

__device__ __forceinline__ int lane_bit(int l, int S) {
  return l < S ? kTpShift + l : kFpShift + (l - S);
}

// per tile and lane (TP of every scale, then FP of every scale): its count
__global__ __launch_bounds__(kThreads) void bit_count_kernel(const uint32_t* bits, int n,
                                                            int S, int nb,
                                                            int32_t* bsum) {
  __shared__ int cnt[2 * LD_EVAL_MAX_SCALES];
  if (threadIdx.x < 2 * S) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int i0 = blockIdx.x * kTile + threadIdx.x * kItems;
  for (int l = 0; l < 2 * S; ++l) {
    int c = 0;
    for (int k = 0; k < kItems; ++k)
      if (i0 + k < n) c += (bits[i0 + k] >> lane_bit(l, S)) & 1u;
    if (c) atomicAdd(&cnt[l], c);
  }
  __syncthreads();
  if (threadIdx.x < 2 * S) bsum[threadIdx.x * nb + blockIdx.x] = cnt[threadIdx.x];
}

// inclusive scan of every lane, offset by the scanned tile sums
__global__ __launch_bounds__(kThreads) void bit_scan_kernel(const uint32_t* bits, int n,
                                                           int S, int nb,
                                                           const int32_t* bsum,
                                                           int32_t* cum) {
  __shared__ int sh[kThreads / 64];
  const int i0 = blockIdx.x * kTile + threadIdx.x * kItems;
  uint32_t v[kItems];
#pragma unroll
  for (int k = 0; k < kItems; ++k) v[k] = (i0 + k < n) ? bits[i0 + k] : 0u;
  for (int l = 0; l < 2 * S; ++l) {
    const int sb = lane_bit(l, S);
    int s = 0;
#pragma unroll
    for (int k = 0; k < kItems; ++k) s += (v[k] >> sb) & 1u;
    int tot;
    int run = bsum[l * nb + blockIdx.x] + block_excl_scan(s, sh, &tot);
    int32_t* out = cum + (size_t)l * n;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      run += (v[k] >> sb) & 1u;
      if (i0 + k < n) out[i0 + k] = run;
    }
  }
}

// mean_ap.py:335-342: recall float64 over max(num_gts, eps); precision fp32
__global__ void pr_kernel(const uint64_t* keys, int n, int S, int C, int num_segs,
                          const int32_t* seg_start, const int32_t* cum,
                          const int32_t* num_gts, double* recall, float* precision) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * S) return;
  const int k = idx / n, r = idx - k * n;
  const int seg = (int)(keys[r] >> 32);
  if (seg >= num_segs) return;
  const int st = seg_start[seg];
  const int32_t* ctp = cum + (size_t)k * n;
  const int32_t* cfp = cum + (size_t)(S + k) * n;
  const int tp = ctp[r] - (st > 0 ? ctp[st - 1] : 0);
  const int fp = cfp[r] - (st > 0 ? cfp[st - 1] : 0);
  const int ng = num_gts[(seg % C) * S + k];
  recall[(size_t)k * n + r] = (double)tp / fmax((double)ng, (double)FLT_EPSILON);
  const float ftp = (float)tp;
  precision[(size_t)k * n + r] = ftp / fmaxf(ftp + (float)fp, FLT_EPSILON);
}

__device__ __forceinline__ double block_sum_double(double v, double* sh) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if (lane == 0) sh[w] = v;
  __syncthreads();
  double t = 0.0;
  for (int k = 0; k < kThreads / 64; ++k) t += sh[k];
  __syncthreads();
  return t;
}

__device__ __forceinline__ float block_max_float(float v, float* sh) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, 64));
  if (lane == 0) sh[w] = v;
  __syncthreads();
  float t = sh[0];
  for (int k = 1; k < kThreads / 64; ++k) t = fmaxf(t, sh[k]);
  __syncthreads();
  return t;
}

// one workgroup per (segment, scale)
__global__ __launch_bounds__(kThreads) void ap_kernel(int n, int S, int num_segs,
                                                     int eleven, const int32_t* seg_start,
                                                     const double* recall,
                                                     const float* precision, float* ap) {
  __shared__ double shd[kThreads / 64];
  __shared__ float shf[kThreads / 64];
  const int seg = blockIdx.x / S, k = blockIdx.x - seg * S;
  const int st = seg_start[seg], en = seg_start[seg + 1];
  const double* rec = recall + (size_t)k * n;
  const float* pre = precision + (size_t)k * n;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (eleven) {
    // mean_ap.py:44-50: thresholds np.arange(0, 1 + 1e-3, 0.1) = i * 0.1
    float acc = 0.0f;
    for (int j = 0; j <= 10; ++j) {
      const double thr = (double)j * 0.1;
      float m = -1.0f;  // no precision at recall >= thr: adds 0
      for (int r = st + threadIdx.x; r < en; r += kThreads)
        if (rec[r] >= thr) m = fmaxf(m, pre[r]);
      m = block_max_float(m, shf);
      if (m >= 0.0f) acc = acc + m;
    }
    // `ap /= 11` inside the per-scale loop: scale k is divided S - k times
    for (int q = k; q < S; ++q) acc = acc / 11.0f;
    if (threadIdx.x == 0) ap[blockIdx.x] = acc;
    return;
  }
  // 'area' (mean_ap.py:32-43): sum over i of (r_i - r_{i-1}) * max(p_i..p_end),
  // r_{-1} = 0; the closing point (1 - r_last) * 0 adds nothing
  float carry = 0.0f;  // max precision of every later tile (mpre ends in 0)
  double sum = 0.0;
  const int ntiles = (en - st + kTile - 1) / kTile;
  for (int tile = ntiles - 1; tile >= 0; --tile) {
    const int i0 = st + tile * kTile + threadIdx.x * kItems;
    float suf[kItems];
    float m = 0.0f;
#pragma unroll
    for (int q = kItems - 1; q >= 0; --q) {
      if (i0 + q < en) m = fmaxf(m, pre[i0 + q]);
      suf[q] = m;
    }
    // exclusive suffix max over the later threads of this tile
    float x = m;
    for (int off = 1; off < 64; off <<= 1) {
      float y = __shfl_down(x, off, 64);
      if (lane + off < 64) x = fmaxf(x, y);
    }
    float after = __shfl_down(x, 1, 64);
    if (lane == 63) after = 0.0f;
    if (lane == 0) shf[w] = x;
    __syncthreads();
    for (int q = w + 1; q < kThreads / 64; ++q) after = fmaxf(after, shf[q]);
    float tile_max = shf[0];
    for (int q = 1; q < kThreads / 64; ++q) tile_max = fmaxf(tile_max, shf[q]);
    __syncthreads();
    after = fmaxf(after, carry);
#pragma unroll
    for (int q = 0; q < kItems; ++q) {
      const int i = i0 + q;
      if (i < en) {
        const double prev = (i > st) ? rec[i - 1] : 0.0;
        const double d = rec[i] - prev;
        if (d != 0.0) sum += d * (double)fmaxf(suf[q], after);
      }
    }
    carry = fmaxf(carry, tile_max);
  }
  sum = block_sum_double(sum, shd);
  if (threadIdx.x == 0) ap[blockIdx.x] = (float)sum;
}

// ------------------------------------------------------- ld_rank_images ------
// ascending float64 score as an ascending unsigned key (NaN-free, -0 ties +0)
__global__ void rank_keys_kernel(int n, const double* score, uint64_t* keys,
                                 uint32_t* vals) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = score[i];
  uint64_t u = (uint64_t)__double_as_longlong(s == 0.0 ? 0.0 : s);
  keys[i] = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
  vals[i] = (uint32_t)i;
}

__global__ void rank_gather_kernel(int n, const uint32_t* vals, const double* score,
                                   int32_t* order, double* sorted) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = vals[i];
  order[i] = (int32_t)j;
  sorted[i] = score[j];
}

struct ApPlan {
  size_t keys0, keys1, vals0, vals1, hist, bsum, cum, total;
  int nb;
};

ApPlan ap_plan(int n, int S) {
  ApPlan o{};
  o.nb = ldeval::sort_tiles(n);
  ldeval::Carver ws;
  o.keys0 = ws.take((size_t)n * 8);
  o.keys1 = ws.take((size_t)n * 8);
  o.vals0 = ws.take((size_t)n * 4);
  o.vals1 = ws.take((size_t)n * 4);
  o.hist = ws.take((size_t)ldeval::kBins * o.nb * 4);
  o.bsum = ws.take((size_t)2 * S * o.nb * 4);
  o.cum = ws.take((size_t)2 * S * n * 4);
  o.total = ws.off;
  return o;
}

int eval_params(int num_classes, int num_scales, const float* area_ranges, int num_thrs,
                const float* iou_thrs, EvalParams* p) {
  if (num_classes < 1 || num_thrs < 1 || num_thrs > LD_EVAL_MAX_THRS || !iou_thrs)
    return LD_EINVAL;
  if (num_scales < 1 || num_scales > LD_EVAL_MAX_SCALES) return LD_EINVAL;
  if (!area_ranges && num_scales != 1) return LD_EINVAL;
  if ((long long)num_thrs * num_classes >= (1ll << 24)) return LD_EUNSUPPORTED;
  *p = EvalParams{};
  p->C = num_classes;
  p->S = num_scales;
  p->T = num_thrs;
  p->has_ranges = area_ranges != nullptr;
  for (int k = 0; k < num_scales && area_ranges; ++k) {
    p->lo[k] = area_ranges[2 * k];
    p->hi[k] = area_ranges[2 * k + 1];
  }
  for (int t = 0; t < num_thrs; ++t) p->thr[t] = iou_thrs[t];
  return 0;
}

}  // namespace

extern "C" {

size_t ld_eval_tpfp_workspace_bytes(int num_dets) {
  if (num_dets < 0) return 0;
  return ldeval::align_up((size_t)num_dets * 4) * 2 + 256;
}

int ld_eval_tpfp(const ld_eval_batch_t* b, int num_classes, int num_scales,
                 const float* area_ranges, int num_thrs, const float* iou_thrs,
                 float* rec_score, int32_t* rec_seg, uint32_t* rec_bits, int32_t* num_gts,
                 void* workspace, size_t workspace_bytes, ld_stream_t stream_) {
  EvalParams p;
  if (!b) return LD_EINVAL;
  if (int e = eval_params(num_classes, num_scales, area_ranges, num_thrs, iou_thrs, &p))
    return e;
  if (b->num_imgs < 1 || b->num_dets < 0 || b->num_gts < 0 || b->num_ign < 0)
    return LD_EINVAL;
  if ((long long)b->num_dets * num_thrs >= (1ll << 31) ||
      (long long)b->num_gts + b->num_ign >= (1ll << 31))
    return LD_EUNSUPPORTED;
  if (!b->det_off || !b->gt_off || !b->ign_off || !num_gts) return LD_EINVAL;
  if (b->num_dets && (!b->dets || !b->det_labels || !rec_score || !rec_seg || !rec_bits))
    return LD_EINVAL;
  if (b->num_gts && (!b->gts || !b->gt_labels)) return LD_EINVAL;
  if (b->num_ign && (!b->ign || !b->ign_labels)) return LD_EINVAL;
  if (workspace_bytes < ld_eval_tpfp_workspace_bytes(b->num_dets) ||
      (b->num_dets && !workspace))
    return LD_ENOSPACE;
  p.num_imgs = b->num_imgs;
  p.num_gts = b->num_gts;
  hipStream_t stream = (hipStream_t)stream_;
  const int N = b->num_dets;
  float* iou_max = (float*)workspace;
  int* argmax = (int*)((char*)workspace + ldeval::align_up((size_t)N * 4));
  if (b->num_gts > 0)
    LD_LAUNCH(eval_count_gts_kernel, dim3((b->num_gts + 255) / 256), dim3(256), 0, stream,
              *b, p, num_gts);
  if (N > 0) {
    LD_LAUNCH(eval_match_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, *b, p,
              iou_max, argmax);
    const int NT = N * num_thrs;
    LD_LAUNCH(eval_decide_kernel, dim3((NT + 255) / 256), dim3(256), 0, stream, *b, p,
              (const float*)iou_max, (const int*)argmax, rec_score, rec_seg, rec_bits);
  }
  return (int)hipGetLastError();
}

size_t ld_eval_ap_workspace_bytes(int num_records, int num_scales) {
  if (num_records < 0 || num_scales < 1 || num_scales > LD_EVAL_MAX_SCALES) return 0;
  return ap_plan(num_records, num_scales).total + 256;
}

int ld_eval_ap(int num_records, const float* rec_score, const int32_t* rec_seg,
               const uint32_t* rec_bits, int num_classes, int num_thrs, int num_scales,
               const int32_t* num_gts, int flags, int32_t* seg_start, double* recall,
               float* precision, float* ap, void* workspace, size_t workspace_bytes,
               ld_stream_t stream_) {
  const int n = num_records;
  if (n < 0 || num_classes < 1 || num_thrs < 1 || num_scales < 1 ||
      num_scales > LD_EVAL_MAX_SCALES)
    return LD_EINVAL;
  if ((long long)num_thrs * num_classes >= (1ll << 24)) return LD_EUNSUPPORTED;
  if ((long long)n * num_scales >= (1ll << 31)) return LD_EUNSUPPORTED;
  if (flags & ~LD_EVAL_11POINTS) return LD_EINVAL;
  if (!num_gts || !seg_start || !ap) return LD_EINVAL;
  if (n > 0 && (!rec_score || !rec_seg || !rec_bits || !recall || !precision))
    return LD_EINVAL;
  const ApPlan o = ap_plan(n, num_scales);
  if (workspace_bytes < o.total || (o.total && !workspace)) return LD_ENOSPACE;
  const int S = num_scales, C = num_classes, num_segs = num_thrs * num_classes;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  const ldeval::SortKeys<false> keys[2] = {{(uint64_t*)(ws + o.keys0)},
                                           {(uint64_t*)(ws + o.keys1)}};
  uint32_t* const vals[2] = {(uint32_t*)(ws + o.vals0), (uint32_t*)(ws + o.vals1)};
  int32_t* hist = (int32_t*)(ws + o.hist);
  int32_t* bsum = (int32_t*)(ws + o.bsum);
  int32_t* cum = (int32_t*)(ws + o.cum);
  int cur = 0;
  if (n > 0) {
    LD_LAUNCH(eval_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, rec_score,
              rec_seg, rec_bits, num_segs, keys[0].hi, vals[0]);
    int seg_bits = 0;
    while ((1 << seg_bits) <= num_segs) ++seg_bits;  // num_segs itself: the sentinel
    const int passes = (32 + seg_bits + ldeval::kRadixBits - 1) / ldeval::kRadixBits;
    cur = ldeval::radix_sort(keys, vals, n, 0, passes, hist, stream);
  }
  LD_LAUNCH(seg_start_kernel, dim3((num_segs + 1 + 255) / 256), dim3(256), 0, stream,
            (const uint64_t*)keys[cur].hi, n, num_segs, seg_start);
  if (n > 0) {
    LD_LAUNCH(bit_count_kernel, dim3(o.nb), dim3(kThreads), 0, stream,
              (const uint32_t*)vals[cur], n, S, o.nb, bsum);
    LD_LAUNCH(excl_scan_kernel<int32_t>, dim3(1, 2 * S), dim3(kThreads), 0, stream, bsum,
              o.nb);
    LD_LAUNCH(bit_scan_kernel, dim3(o.nb), dim3(kThreads), 0, stream,
              (const uint32_t*)vals[cur], n, S, o.nb, (const int32_t*)bsum, cum);
    LD_LAUNCH(pr_kernel, dim3((n * S + 255) / 256), dim3(256), 0, stream,
              (const uint64_t*)keys[cur].hi, n, S, C, num_segs, (const int32_t*)seg_start,
              (const int32_t*)cum, num_gts, recall, precision);
  }
  LD_LAUNCH(ap_kernel, dim3(num_segs * S), dim3(kThreads), 0, stream, n, S, num_segs,
            (flags & LD_EVAL_11POINTS) ? 1 : 0, (const int32_t*)seg_start,
            (const double*)recall, (const float*)precision, ap);
  return (int)hipGetLastError();
}

size_t ld_rank_images_workspace_bytes(int num_imgs) {
  if (num_imgs < 0) return 0;
  return ap_plan(num_imgs, 1).total + 256;
}

int ld_rank_images(int num_imgs, const double* scores, int32_t* order, double* sorted,
                   void* workspace, size_t workspace_bytes, ld_stream_t stream_) {
  const int n = num_imgs;
  if (n < 0) return LD_EINVAL;
  if (n == 0) return 0;
  if (!scores || !order || !sorted) return LD_EINVAL;
  const ApPlan o = ap_plan(n, 1);
  if (workspace_bytes < o.total || !workspace) return LD_ENOSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  const ldeval::SortKeys<false> keys[2] = {{(uint64_t*)(ws + o.keys0)},
                                           {(uint64_t*)(ws + o.keys1)}};
  uint32_t* const vals[2] = {(uint32_t*)(ws + o.vals0), (uint32_t*)(ws + o.vals1)};
  int32_t* hist = (int32_t*)(ws + o.hist);
  LD_LAUNCH(rank_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, scores,
            keys[0].hi, vals[0]);
  const int cur =
      ldeval::radix_sort(keys, vals, n, 0, 64 / ldeval::kRadixBits, hist, stream);
  LD_LAUNCH(rank_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n,
            (const uint32_t*)vals[cur], scores, order, sorted);
  return (int)hipGetLastError();
}

}  // extern "C"
