// Per-image mAP on gfx950: the reference's bbox_map_eval
// (tools/analysis_tools/analyze_results.py:13-45) for every image of a batch in
// one launch, and the box and label painters of its good / bad image dumps and
// of show_result.
//
// Replaces (reference file:line)
//   bbox_map_eval: eval_map of a one-image dataset at every IoU threshold,
//   mean over the thresholds        tools/analysis_tools/analyze_results.py:38-45
//   tpfp_default, area_ranges=None  core/evaluation/mean_ap.py:153-237
//   recall / precision / 'area' AP  mean_ap.py:32-43, 353-364
//   mean over classes with GTs      mean_ap.py:392-396 (float32 np.mean)
//
// One workgroup of 256 threads per image; nothing leaves the workgroup:
//   1. stage   detections, GTs then ignored GTs of the image into LDS when they
//              fit (kMaxD detections, kMaxG GTs + ignored); otherwise every
//              array below lives in the caller's workspace and the boxes are
//              read from the batch.  Same code, pointers chosen once.
//   2. match   one thread per detection: argmax IoU over its class's GTs then
//              ignored GTs (fp32, reference op order, first maximum wins)
//   3. rank    one thread per detection, by counting: its position in (class,
//              descending score, position) order, and the largest ious_max of
//              the detections before it in its class that share its argmax GT.
//              It is TP at thr exactly when it matches a real GT and that
//              maximum is below thr (the rule of eval_decide_kernel), so no
//              threshold needs the greedy loop.
//   4. ap      one wave per (class with GT, threshold): cumulative TP / FP from
//              ballots, precision fp32, recall float64, suffix maximum from the
//              end by shuffles; the recall steps are summed in float64 in
//              numpy's pairwise order (np.sum), one lane.
//   5. mean    one thread per threshold: float32 np.mean over the classes with
//              GTs; thread 0: float64 mean over thresholds.
// No float atomics, no host round trip.  Integer / compare work on at most a few
// hundred boxes per workgroup: bound by launch latency and LDS round trips, not
// by memory bandwidth.
#include <hip/hip_runtime.h>

#include <float.h>
#include <stdint.h>

#include "../../include/ld_hip.h"
#include "eval_common.h"
#include "eval_iou.h"
#include "font5x7.h"
#include "ld_launch.h"

namespace {

using ldeval::box_area;
using ldeval::iou_ref;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxD = 256;  // detections of an image held in LDS
constexpr int kMaxG = 128;  // GTs + ignored GTs of an image held in LDS
constexpr int kPwBlock = 128;  // numpy's PW_BLOCKSIZE

struct ImageMapParams {
  double thr[LD_EVAL_MAX_THRS];
  int C, T, no_lds;
};

// np.add.reduce of a contiguous vector (numpy pairwise_sum): < 8 sequential from
// 0; <= 128 eight running sums over blocks of 8, combined as a fixed tree, then
// the remainder; above, split at n / 2 rounded down to a multiple of 8.  The
// elements are consumed strictly left to right, so they come from next().
template <typename T, typename Next>
__device__ T np_sum_leaf(int n, Next& next) {
  if (n < 8) {
    T res = 0;
    for (int i = 0; i < n; ++i) res += next();
    return res;
  }
  T r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = next();
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] += next();
  }
  T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += next();
  return res;
}

template <typename T, typename Next>
__device__ T np_sum(int n, Next next) {
  if (n <= kPwBlock) return np_sum_leaf<T>(n, next);
  constexpr int kDepth = 28;  // halves from 2**31 down to 128
  int fn[kDepth], fs[kDepth];
  T fl[kDepth];
  int sp = 0;
  fn[0] = n;
  fs[0] = 0;
  T ret = 0;
  while (sp >= 0) {
    const int m = fn[sp];
    if (m <= kPwBlock) {
      ret = np_sum_leaf<T>(m, next);
      --sp;
      continue;
    }
    int n2 = m / 2;
    n2 -= n2 % 8;
    if (fs[sp] == 0) {
      fs[sp] = 1;
      ++sp;
      fn[sp] = n2;
      fs[sp] = 0;
    } else if (fs[sp] == 1) {
      fl[sp] = ret;
      fs[sp] = 2;
      ++sp;
      fn[sp] = m - n2;
      fs[sp] = 0;
    } else {
      ret = fl[sp] + ret;
      --sp;
    }
  }
  return ret;
}

// workspace of the path that does not fit LDS, in elements of the whole batch
struct ImgPlan {
  size_t iou, arg, prev, order, prec, ctp, term, total;
};

ImgPlan img_plan(int num_dets, int num_imgs) {
  ImgPlan o{};
  ldeval::Carver ws;
  const size_t N = (size_t)num_dets;
  o.iou = ws.take(N * 4);
  o.arg = ws.take(N * 4);
  o.prev = ws.take(N * 4);
  o.order = ws.take(N * 4);
  o.prec = ws.take(N * 4 * kWaves);
  o.ctp = ws.take(N * 4 * kWaves);
  o.term = ws.take((N + (size_t)num_imgs) * 8 * kWaves);  // one closing step per class
  o.total = ws.off;
  return o;
}

__global__ __launch_bounds__(kThreads) void eval_image_map_kernel(
    ld_eval_batch_t b, ImageMapParams p, ImgPlan plan, char* ws, float* ap,
    uint8_t* has_gt, double* map) {
  __shared__ float s_det[kMaxD * 5];
  __shared__ int s_dlab[kMaxD];
  __shared__ float s_gt[kMaxG * 4];
  __shared__ int s_glab[kMaxG];
  __shared__ float s_iou[kMaxD], s_prev[kMaxD];
  __shared__ int s_arg[kMaxD], s_order[kMaxD];
  __shared__ float s_prec[kWaves][kMaxD];
  __shared__ int s_ctp[kWaves][kMaxD];
  __shared__ double s_term[kWaves][kMaxD + 1];
  __shared__ float s_mean[LD_EVAL_MAX_THRS];

  const int img = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int C = p.C, T = p.T;
  const int d0 = b.det_off[img], n = b.det_off[img + 1] - d0;
  const int g0 = b.gt_off[img], g = b.gt_off[img + 1] - g0;
  const int i0 = b.ign_off[img], ng_all = g + (b.ign_off[img + 1] - i0);
  const bool fast = !p.no_lds && n <= kMaxD && ng_all <= kMaxG;

  // a label no class array holds sorts past every class
  auto norm = [C](int64_t l) { return (l >= 0 && l < C) ? (int)l : C; };
  auto det = [&](int i) -> const float* {
    return fast ? s_det + i * 5 : b.dets + (size_t)(d0 + i) * 5;
  };
  auto dlab = [&](int i) { return fast ? s_dlab[i] : norm(b.det_labels[d0 + i]); };
  auto gtbox = [&](int j) -> const float* {  // GTs, then ignored GTs
    if (fast) return s_gt + j * 4;
    return j < g ? b.gts + (size_t)(g0 + j) * 4 : b.ign + (size_t)(i0 + j - g) * 4;
  };
  auto glab = [&](int j) {
    if (fast) return s_glab[j];
    return norm(j < g ? b.gt_labels[g0 + j] : b.ign_labels[i0 + j - g]);
  };
  float* iou = fast ? s_iou : (float*)(ws + plan.iou) + d0;
  int* arg = fast ? s_arg : (int*)(ws + plan.arg) + d0;
  float* prev = fast ? s_prev : (float*)(ws + plan.prev) + d0;
  int* order = fast ? s_order : (int*)(ws + plan.order) + d0;
  float* wprec = fast ? s_prec[w] : (float*)(ws + plan.prec) + (size_t)w * b.num_dets + d0;
  int* wctp = fast ? s_ctp[w] : (int*)(ws + plan.ctp) + (size_t)w * b.num_dets + d0;
  double* wterm = fast ? s_term[w]
                       : (double*)(ws + plan.term) +
                             (size_t)w * ((size_t)b.num_dets + b.num_imgs) + d0 + img;

  // ---- 1. stage, clear this image's outputs
  if (fast) {
    for (int k = tid; k < n * 5; k += kThreads) s_det[k] = b.dets[(size_t)d0 * 5 + k];
    for (int k = tid; k < n; k += kThreads) s_dlab[k] = norm(b.det_labels[d0 + k]);
    for (int k = tid; k < ng_all * 4; k += kThreads) {
      const int j = k >> 2, q = k & 3;
      s_gt[k] = j < g ? b.gts[(size_t)(g0 + j) * 4 + q] : b.ign[(size_t)(i0 + j - g) * 4 + q];
    }
    for (int j = tid; j < ng_all; j += kThreads)
      s_glab[j] = norm(j < g ? b.gt_labels[g0 + j] : b.ign_labels[i0 + j - g]);
  }
  float* ap_img = ap + (size_t)img * T * C;
  uint8_t* hg = has_gt + (size_t)img * C;
  for (int k = tid; k < T * C; k += kThreads) ap_img[k] = 0.0f;
  for (int c = tid; c < C; c += kThreads) hg[c] = 0;
  __syncthreads();
  for (int j = tid; j < g; j += kThreads) {
    const int l = glab(j);
    if (l < C) hg[l] = 1;
  }

  // ---- 2. match
  for (int i = tid; i < n; i += kThreads) {
    const int lab = dlab(i);
    float best = 0.0f;
    int a = -1;
    if (lab < C) {
      const float* d = det(i);
      const float ad = box_area(d);
      for (int j = 0; j < ng_all; ++j) {
        if (glab(j) != lab) continue;
        const float v = iou_ref(d, ad, gtbox(j));
        if (a < 0 || v > best) best = v, a = j;
      }
    }
    iou[i] = best;
    arg[i] = a;
  }
  __syncthreads();

  // ---- 3. rank by counting
  for (int i = tid; i < n; i += kThreads) {
    const int li = dlab(i), ai = arg[i];
    const float si = det(i)[4];
    int pos = 0;
    float pm = -1.0f;  // IoUs are >= 0
    for (int j = 0; j < n; ++j) {
      const int lj = dlab(j);
      const float sj = det(j)[4];
      const bool ahead = sj > si || (sj == si && j < i);
      if (lj < li || (lj == li && ahead)) ++pos;
      if (lj == li && ahead && ai >= 0 && arg[j] == ai) pm = fmaxf(pm, iou[j]);
    }
    order[pos] = i;
    prev[i] = pm;
  }
  __syncthreads();

  // ---- 4. AP of every (class with GT, threshold), one wave each
  const uint64_t le = (lane == 63) ? ~0ull : ((1ull << (lane + 1)) - 1ull);
  int task = 0;
  for (int c = 0; c < C; ++c) {
    if (!hg[c]) continue;
    if ((w - task % kWaves + kWaves) % kWaves >= T) {  // none of its T tasks is ours
      task += T;
      continue;
    }
    // this class's slice of the sorted detections, and its GT count
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (dlab(order[mid]) < c) lo = mid + 1;
      else hi = mid;
    }
    const int cs = lo;
    hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (dlab(order[mid]) <= c) lo = mid + 1;
      else hi = mid;
    }
    const int k = lo - cs;
    int num_gts = 0;
    for (int base = 0; base < g; base += 64) {
      const int j = base + lane;
      num_gts += __popcll(__ballot(j < g && glab(j) == c));
    }
    // mean_ap.py:363: max(num_gts, eps); num_gts >= 1 here
    const double den = fmax((double)num_gts, (double)FLT_EPSILON);
    for (int t = 0; t < T; ++t, ++task) {
      if (task % kWaves != w) continue;
      const double thr = p.thr[t];
      int ctp = 0, cfp = 0;
      for (int base = 0; base < k; base += 64) {
        const int q = base + lane;
        const bool valid = q < k;
        bool tp = false, fp = false;
        if (valid) {
          const int i = order[cs + q];
          const int a = arg[i];
          const bool matched = a >= 0 && (double)iou[i] >= thr;
          if (!matched) fp = true;
          else if (a < g) {  // a matched ignored GT gives neither
            const bool covered = (double)prev[i] >= thr;
            tp = !covered;
            fp = covered;
          }
        }
        const uint64_t btp = __ballot(tp), bfp = __ballot(fp);
        const int mytp = ctp + __popcll(btp & le), myfp = cfp + __popcll(bfp & le);
        if (valid) {
          const float ftp = (float)mytp;
          wprec[q] = ftp / fmaxf(ftp + (float)myfp, FLT_EPSILON);
          wctp[q] = mytp * 2 + (tp ? 1 : 0);
        }
        ctp += __popcll(btp);
        cfp += __popcll(bfp);
      }
      // mean_ap.py:36-43: steps of mrec = [0, recall, 1] times the maximum of
      // mpre = [0, precision, 0] from there on; step m is TP number m
      const int nterms = ctp + (ctp != num_gts ? 1 : 0);
      float carry = 0.0f;
      for (int base = ((k - 1) / 64) * 64; base >= 0 && k > 0; base -= 64) {
        const int q = base + lane;
        const bool valid = q < k;
        float x = valid ? wprec[q] : 0.0f;
        for (int off = 1; off < 64; off <<= 1) {
          const float y = __shfl_down(x, off, 64);
          if (lane + off < 64) x = fmaxf(x, y);
        }
        x = fmaxf(x, carry);
        if (valid) {
          const int e = wctp[q];
          if (e & 1) {
            const int m = e >> 1;  // cumulative TP, this one included
            wterm[m - 1] = ((double)m / den - (double)(m - 1) / den) * (double)x;
          }
        }
        carry = __shfl(x, 0, 64);
      }
      if (lane == 0 && ctp != num_gts) wterm[ctp] = (1.0 - (double)ctp / den) * 0.0;
      __threadfence_block();
      if (lane == 0) {
        int cur = 0;
        const double s = np_sum<double>(nterms, [&]() { return wterm[cur++]; });
        ap_img[t * C + c] = (float)s;
      }
      __threadfence_block();  // the next task reuses wterm
    }
  }
  __syncthreads();

  // ---- 5. mean over classes with GTs (float32), then over thresholds
  if (tid < T) {
    int ncls = 0;
    for (int c = 0; c < C; ++c) ncls += hg[c] ? 1 : 0;
    float m = 0.0f;
    if (ncls > 0) {
      int c = 0;
      const float* row = ap_img + tid * C;
      const float s = np_sum<float>(ncls, [&]() {
        while (!hg[c]) ++c;
        return row[c++];
      });
      m = s / (float)ncls;
    }
    s_mean[tid] = m;
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int t = 0; t < T; ++t) s += (double)s_mean[t];
    map[img] = s / (double)T;
  }
}

// ------------------------------------------------------------- painter ------
struct DrawParams {
  int H, W, num_gts, num_dets, thickness;
  float score_thr;
  uint32_t gt_color, det_color;  // channel 0 in bits 0-7, 1 in 8-15, 2 in 16-23
};

// bbox.astype(np.int32) for values an image can hold; the cast saturates, and
// the clamp keeps x + thickness inside int32
__device__ __forceinline__ int trunc_i32(float v) {
  const int x = (int)v;
  return min(max(x, -(1 << 30)), 1 << 30);
}

__global__ __launch_bounds__(kThreads) void draw_boxes_kernel(uint8_t* img, DrawParams p,
                                                             const float* gts,
                                                             const float* dets) {
  __shared__ int s_box[kThreads][4];
  __shared__ uint32_t s_col[kThreads];
  const int tid = threadIdx.x;
  const long long pix = (long long)blockIdx.x * kThreads + tid;
  const bool inside = pix < (long long)p.H * p.W;
  const int y = inside ? (int)(pix / p.W) : 0, x = inside ? (int)(pix - (long long)y * p.W) : 0;
  const int total = p.num_gts + p.num_dets;
  bool hit = false;
  uint32_t col = 0u;
  for (int base = 0; base < total; base += kThreads) {
    __syncthreads();
    const int k = base + tid;
    if (k < total) {
      const bool is_gt = k < p.num_gts;
      const float* bx = is_gt ? gts + (size_t)k * 4 : dets + (size_t)(k - p.num_gts) * 5;
      const bool keep = is_gt || bx[4] >= p.score_thr;
      s_box[tid][0] = keep ? trunc_i32(bx[0]) : 0;
      s_box[tid][1] = keep ? trunc_i32(bx[1]) : 0;
      s_box[tid][2] = keep ? trunc_i32(bx[2]) : -1;  // x2 < x1: paints nothing
      s_box[tid][3] = keep ? trunc_i32(bx[3]) : -1;
      s_col[tid] = is_gt ? p.gt_color : p.det_color;
    }
    __syncthreads();
    const int cnt = min(kThreads, total - base);
    for (int q = 0; q < cnt; ++q) {  // in order: a later box paints over
      const int x1 = s_box[q][0], y1 = s_box[q][1], x2 = s_box[q][2], y2 = s_box[q][3];
      if (x < x1 || x > x2 || y < y1 || y > y2) continue;
      if (x < x1 + p.thickness || x > x2 - p.thickness || y < y1 + p.thickness ||
          y > y2 - p.thickness) {
        hit = true;
        col = s_col[q];
      }
    }
  }
  if (inside && hit) {
    uint8_t* px = img + (size_t)pix * 3;
    px[0] = (uint8_t)(col & 255u);
    px[1] = (uint8_t)((col >> 8) & 255u);
    px[2] = (uint8_t)((col >> 16) & 255u);
  }
}

// ------------------------------------------------------------- labels -------
constexpr int kFontChars = LD_FONT_LAST - LD_FONT_FIRST + 1;
constexpr int kCellW = 6, kCellH = 8;  // glyph at columns 1-5, rows 1-7
constexpr int kMaxScale = 1 << 10;     // keeps every extent below inside int32

const uint8_t kFontHost[kFontChars * LD_FONT_ROWS] = {LD_FONT5X7_TABLE};
__constant__ uint8_t kFont[kFontChars * LD_FONT_ROWS] = {LD_FONT5X7_TABLE};

struct LabelParams {
  int H, W, num_labels, scale;
  uint32_t fg, bg;
};

// One thread per pixel.  Every pixel finds the LAST label whose rectangle
// covers it and takes that label's colour there, which is what painting the
// labels in index order leaves; nothing depends on the order threads run in.
__global__ __launch_bounds__(kThreads) void draw_labels_kernel(uint8_t* img, LabelParams p,
                                                              const uint8_t* text,
                                                              const int32_t* desc) {
  __shared__ int s_lab[kThreads][3];  // x0, y0, width in pixels
  const int tid = threadIdx.x;
  const long long pix = (long long)blockIdx.x * kThreads + tid;
  const bool inside = pix < (long long)p.H * p.W;
  const int y = inside ? (int)(pix / p.W) : 0, x = inside ? (int)(pix - (long long)y * p.W) : 0;
  const int ch = kCellH * p.scale;
  int best = -1, bx = 0, by = 0;
  for (int base = 0; base < p.num_labels; base += kThreads) {
    __syncthreads();
    const int k = base + tid;
    if (k < p.num_labels) {
      const int32_t* d = desc + (size_t)k * 4;
      const int lim = 1 << 30;
      const int x1 = min(max(d[0], -lim), lim), y1 = min(max(d[1], -lim), lim);
      const int len = min(max(d[2], 0), LD_LABEL_MAX_LEN);
      s_lab[tid][0] = x1;
      s_lab[tid][1] = y1 - ch >= 0 ? y1 - ch : y1;  // above the box, else inside it
      s_lab[tid][2] = len * kCellW * p.scale;
    }
    __syncthreads();
    const int cnt = min(kThreads, p.num_labels - base);
    for (int q = 0; q < cnt; ++q) {
      const int x0 = s_lab[q][0], y0 = s_lab[q][1], w = s_lab[q][2];
      // x0 + w and y0 + ch stay below 2^30 + 2^19: no overflow
      if (x >= x0 && x < x0 + w && y >= y0 && y < y0 + ch) best = base + q, bx = x0, by = y0;
    }
  }
  if (!inside || best < 0) return;
  const int cx = (x - bx) / p.scale, cy = (y - by) / p.scale;  // cy < kCellH
  const int gx = cx % kCellW;
  int c = text[(size_t)best * LD_LABEL_MAX_LEN + cx / kCellW];  // cx / 6 < len <= MAX_LEN
  if (c < LD_FONT_FIRST || c > LD_FONT_LAST) c = '?';
  const bool on = gx >= 1 && cy >= 1 &&
                  ((kFont[(c - LD_FONT_FIRST) * LD_FONT_ROWS + cy - 1] >> (kCellW - 1 - gx)) & 1);
  const uint32_t col = on ? p.fg : p.bg;
  uint8_t* px = img + (size_t)pix * 3;
  px[0] = (uint8_t)(col & 255u);
  px[1] = (uint8_t)((col >> 8) & 255u);
  px[2] = (uint8_t)((col >> 16) & 255u);
}

}  // namespace

extern "C" {

size_t ld_eval_image_map_workspace_bytes(int num_dets, int num_imgs) {
  if (num_dets < 0 || num_imgs < 0) return 0;
  return img_plan(num_dets, num_imgs).total + 256;
}

int ld_eval_image_map(const ld_eval_batch_t* b, int num_classes, int num_thrs,
                      const double* iou_thrs, int flags, float* ap, uint8_t* has_gt,
                      double* map, void* workspace, size_t workspace_bytes,
                      ld_stream_t stream_) {
  if (!b || !iou_thrs) return LD_EINVAL;
  if (num_classes < 1 || num_thrs < 1 || num_thrs > LD_EVAL_MAX_THRS) return LD_EINVAL;
  if (flags & ~LD_EVAL_IMAGE_NO_LDS) return LD_EINVAL;
  if (b->num_imgs < 0 || b->num_dets < 0 || b->num_gts < 0 || b->num_ign < 0)
    return LD_EINVAL;
  if (b->num_imgs == 0) return 0;
  if ((long long)b->num_imgs * num_thrs * num_classes >= (1ll << 31) ||
      (long long)b->num_gts + b->num_ign >= (1ll << 31))
    return LD_EUNSUPPORTED;
  if (!b->det_off || !b->gt_off || !b->ign_off || !ap || !has_gt || !map) return LD_EINVAL;
  if (b->num_dets && (!b->dets || !b->det_labels)) return LD_EINVAL;
  if (b->num_gts && (!b->gts || !b->gt_labels)) return LD_EINVAL;
  if (b->num_ign && (!b->ign || !b->ign_labels)) return LD_EINVAL;
  const ImgPlan plan = img_plan(b->num_dets, b->num_imgs);
  if (workspace_bytes < plan.total || !workspace) return LD_ENOSPACE;
  ImageMapParams p{};
  p.C = num_classes;
  p.T = num_thrs;
  p.no_lds = (flags & LD_EVAL_IMAGE_NO_LDS) ? 1 : 0;
  for (int t = 0; t < num_thrs; ++t) p.thr[t] = iou_thrs[t];
  LD_LAUNCH(eval_image_map_kernel, dim3(b->num_imgs), dim3(kThreads), 0,
            (hipStream_t)stream_, *b, p, plan, (char*)workspace, ap, has_gt, map);
  return (int)hipGetLastError();
}

int ld_draw_boxes(uint8_t* img, int height, int width, const float* gt_boxes, int num_gts,
                  const float* dets, int num_dets, float score_thr, int thickness,
                  uint32_t gt_color, uint32_t det_color, ld_stream_t stream_) {
  if (height < 0 || width < 0 || num_gts < 0 || num_dets < 0 || thickness < 1)
    return LD_EINVAL;
  const long long pixels = (long long)height * width;
  if (pixels == 0 || num_gts + num_dets == 0) return 0;
  if (!img || (num_gts && !gt_boxes) || (num_dets && !dets)) return LD_EINVAL;
  if (pixels >= (1ll << 31) || thickness > (1 << 20)) return LD_EUNSUPPORTED;
  DrawParams p{height, width, num_gts, num_dets, thickness, score_thr, gt_color, det_color};
  LD_LAUNCH(draw_boxes_kernel, dim3((unsigned)((pixels + kThreads - 1) / kThreads)),
            dim3(kThreads), 0, (hipStream_t)stream_, img, p, gt_boxes, dets);
  return (int)hipGetLastError();
}

int ld_font_glyph(int c, int row) {
  if (c < LD_FONT_FIRST || c > LD_FONT_LAST || row < 0 || row >= LD_FONT_ROWS) return -1;
  return kFontHost[(c - LD_FONT_FIRST) * LD_FONT_ROWS + row];
}

int ld_draw_labels(uint8_t* img, int height, int width, const uint8_t* text_bytes,
                   const int32_t* desc, int num_labels, int scale, uint32_t fg_color,
                   uint32_t bg_color, ld_stream_t stream_) {
  if (height < 0 || width < 0 || num_labels < 0 || scale < 1) return LD_EINVAL;
  const long long pixels = (long long)height * width;
  if (pixels == 0 || num_labels == 0) return 0;
  if (!img || !text_bytes || !desc) return LD_EINVAL;
  if (pixels >= (1ll << 31) || scale > kMaxScale) return LD_EUNSUPPORTED;
  LabelParams p{height, width, num_labels, scale, fg_color, bg_color};
  LD_LAUNCH(draw_labels_kernel, dim3((unsigned)((pixels + kThreads - 1) / kThreads)),
            dim3(kThreads), 0, (hipStream_t)stream_, img, p, text_bytes, desc);
  return (int)hipGetLastError();
}

}  // extern "C"
