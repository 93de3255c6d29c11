// COCO-style bbox evaluation on gfx950: pycocotools' COCOeval(iouType='bbox')
// evaluate() + accumulate() as mmdet's CocoDataset.evaluate drives them, on the
// device, float64 in pycocotools' order of operations (-ffp-contract=off).
//
// Replaces (reference file:line, and the pycocotools functions it calls)
//   CocoDataset._det2json / results2json       datasets/coco.py:216-231
//   COCO.loadRes (bbox area, id)               pycocotools coco.py
//   COCOeval.computeIoU / maskApi bbIou        float64, crowd union = det area
//   COCOeval.evaluateImg                       per (image, category) greedy match
//   COCOeval.accumulate                        precision / recall / scores
// summarize() runs on the host over the device precision / recall arrays.
//
// ld_coco_match (one call per batch of images)
//   1. rank     one thread per detection: category index through the label map,
//               rank inside its (image, category) cell (descending score, ties
//               by position: a stable sort) and its slot in the image's
//               category-major order.  O(dets of its image) per thread.
//   2. match    one wave64 per (image, category) cell.  The D x G float64 IoU
//               tile is computed once by all lanes into LDS (kLdsTile doubles);
//               lane t * A + a then runs evaluateImg's sequential greedy for
//               threshold t and area range a, its "GT matched" bitmask in LDS.
//               Per detection two ballots give the matched / ignored bits of
//               every (t, a).  npig (non-ignored GTs per category and area) is
//               added with integer atomics.  Bound by the greedy's D x G LDS
//               reads per lane.
//   3. big      cells whose tile exceeds the LDS budget (or with more than
//               kLdsG GTs) are queued by step 2 and matched by kSlots
//               workgroups, each with its own global-memory tile.
// ld_coco_accumulate (once)
//   1. sort     stable LSD radix sort of (category, descending score, image
//               rank, rank in cell): accumulate's mergesort order of every
//               maxDets slice, since a slice keeps the order of the whole.
//   2. tiles    each category is cut into kTile-record tiles, so one category
//               spans as many workgroups as it needs.  Per tile and lane
//               (t, a, m): TP / FP counts of the records with rank < maxDets[m]
//               -> per-category exclusive prefix -> per-tile maximum of the
//               precision -> suffix maximum over the later tiles.
//   3. final    per record: cumulative TP / FP, rc and pr in float64, the
//               precision envelope (in-tile reverse max-scan + later tiles), and
//               the recall thresholds whose searchsorted index is this record.
// Everything but the sort is bound by block-wide scans (one per lane and tile).
//
// ld_coco_match_errors (tools/analysis_tools/coco_error_analysis.py: the main
// COCOeval pass and the two per-category passes of analyze_individual_category
// in one match).  Same rank step, same wave64 per (image, category) cell, but
// the GTs of a cell are the image's whole GT span in annotation order
// (imgToAnns order, which the relabel keeps), each with its category index:
//   rows t < T0   plain evaluateImg at iou_thrs[t]: only the cell's own GTs;
//   row  T0       "Sim" at err_thr: own GTs + the GTs of the other categories
//                 of the same supercategory, relabelled ignore = iscrowd = 1;
//   row  T0 + 1   "Oth" at err_thr: own GTs + every other GT of the image,
//                 relabelled likewise (unknown categories included).
// A relabelled GT is a crowd (overlap = intersection / detection area, never
// consumed) and ignored in every area range, so it leaves npig alone.  One IoU
// tile (D x image GTs) serves every row.  Lane t * A + a writes bit t * A + a,
// so one ld_coco_accumulate call with T0 + 2 thresholds and M = 1 gives every
// row.  Images with more than kLdsG GTs or tiles over kLdsTile take the
// global-tile path; more than LD_COCO_MAX_CELL_GTS GTs in an image is refused.
#include <hip/hip_runtime.h>

#include <float.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/ld_hip.h"
#include "eval_common.h"
#include "ld_launch.h"

namespace {

using ldeval::block_excl_scan;
using ldeval::desc_key;
using ldeval::find_img;

constexpr int kWave = 64;
constexpr int kLdsTile = 2048;  // doubles: 16 KiB IoU tile per match workgroup
constexpr int kLdsG = 256;      // GTs per cell on the LDS path (bitmask words)
constexpr int kSlots = 16;      // workgroups (global tiles) of the big-cell path
constexpr int kThreads = 256;
constexpr int kItems = 8;
constexpr int kTile = kThreads * kItems;  // records per accumulate tile
constexpr int kMaxLanes = 64 * LD_COCO_MAX_MAXDETS;  // (t, a) <= 64 times maxDets
constexpr uint32_t kFlagCrowd = 1u << 8;
constexpr uint32_t kFlagIdNz = 1u << 9;  // annotation id != 0

struct MatchParams {
  double iou0[LD_COCO_MAX_THRS];  // min(t, 1 - 1e-10), host float64
  double lo[LD_COCO_MAX_AREAS], hi[LD_COCO_MAX_AREAS];
  int T, A, K, max_det, max_d;
  long long slot_elems;
};

struct AccParams {
  double rec[LD_COCO_MAX_REC_THRS];
  int max_dets[LD_COCO_MAX_MAXDETS];
  int T, A, M, R, K, L, n, nt, max_det;
};

__device__ __forceinline__ int det_cat(const ld_coco_batch_t& b, int j) {
  const int64_t lab = b.labels[j];
  return (lab >= 0 && lab < b.num_labels) ? b.label_cat[lab] : -1;
}

// maskApi bbIou: boxes xywh float64, crowd: union = detection box area
__device__ __forceinline__ double bb_iou(const double* d, const double* g, bool crowd) {
  double w = fmin(d[2] + d[0], g[2] + g[0]) - fmax(d[0], g[0]);
  if (w <= 0) return 0.0;
  double h = fmin(d[3] + d[1], g[3] + g[1]) - fmax(d[1], g[1]);
  if (h <= 0) return 0.0;
  double i = w * h;
  double da = d[2] * d[3], ga = g[2] * g[3];
  double u = crowd ? da : da + ga - i;
  return i / u;
}

// _det2json: [x1, y1, x2 - x1, y2 - y1] in float64 of the fp32 values
__device__ __forceinline__ void det_xywh(const float* p, double* o) {
  o[0] = (double)p[0];
  o[1] = (double)p[1];
  o[2] = (double)p[2] - (double)p[0];
  o[3] = (double)p[3] - (double)p[1];
}

__global__ void coco_rank_kernel(ld_coco_batch_t b, MatchParams p, int32_t* order,
                                 float* rec_score, int32_t* rec_cat, uint32_t* rec_pos,
                                 uint64_t* rec_match, uint64_t* rec_ign) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.num_dets) return;
  const int img = find_img(b.det_off, b.num_imgs, i);
  const int k = det_cat(b, i);
  const float s = b.dets[(size_t)i * 5 + 4];
  int rank = 0, lt = 0;
  if (k >= 0) {
    for (int j = b.det_off[img]; j < b.det_off[img + 1]; ++j) {
      const int kj = det_cat(b, j);
      if (kj < 0) continue;
      if (kj < k) ++lt;
      if (kj != k) continue;
      const float sj = b.dets[(size_t)j * 5 + 4];
      rank += (sj > s || (sj == s && j < i));
    }
    order[b.det_off[img] + lt + rank] = i;
  }
  const bool kept = k >= 0 && rank < p.max_det;
  rec_score[i] = s;
  rec_cat[i] = kept ? k : p.K;  // p.K: not scored (sorts after every category)
  rec_pos[i] = kept ? (uint32_t)b.img_rank[img] * (uint32_t)p.max_det + (uint32_t)rank : 0u;
  rec_match[i] = 0ull;
  rec_ign[i] = 0ull;
}

__device__ __forceinline__ int wave_sum(int v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// BIG = false: every (batch image, category) cell, LDS tile; cells that do not
// fit are appended to big_list.  BIG = true: the queued cells, one global tile
// per workgroup.
template <bool BIG>
__global__ __launch_bounds__(kWave) void coco_match_kernel(
    ld_coco_batch_t b, MatchParams p, const int32_t* order, int32_t* big_list,
    double* slots, uint64_t* rec_match, uint64_t* rec_ign, int32_t* npig) {
  constexpr int GMAX = BIG ? LD_COCO_MAX_CELL_GTS : kLdsG;
  __shared__ double tile_s[BIG ? 1 : kLdsTile];
  __shared__ uint32_t gfl[GMAX];
  __shared__ uint32_t gm[GMAX / 32][kWave];
  const int lane = threadIdx.x;
  const int K = p.K, A = p.A;
  const int n_cells = BIG ? big_list[0] : 1;
  for (int e = BIG ? blockIdx.x : 0; e < n_cells; e += BIG ? gridDim.x : 1) {
    const int cell = BIG ? big_list[1 + e] : blockIdx.x;
    const int bi = cell / K, k = cell - bi * K;
    const int d0 = b.det_off[bi], d1 = b.det_off[bi + 1];
    int lt = 0, eq = 0;
    for (int j = d0 + lane; j < d1; j += kWave) {
      const int kj = det_cat(b, j);
      lt += (kj >= 0 && kj < k);
      eq += (kj == k);
    }
    lt = wave_sum(lt);
    eq = wave_sum(eq);
    const int D = min(min(eq, p.max_det), p.max_d);
    const int gc = b.img_rank[bi] * K + k;
    const int g0 = b.gt_cell_off[gc];
    const int G = min(b.gt_cell_off[gc + 1] - g0, b.max_cell_gts);
    if (!BIG && lane < A && G > 0) {
      int c = 0;
      for (int g = 0; g < G; ++g) {
        const double ar = b.gt_area[g0 + g];
        c += !b.gt_crowd[g0 + g] && !(ar < p.lo[lane] || ar > p.hi[lane]);
      }
      if (c) atomicAdd(npig + k * A + lane, c);
    }
    if (D == 0) continue;
    if (!BIG && (G > kLdsG || (long long)D * G > kLdsTile)) {
      if (lane == 0) big_list[1 + atomicAdd(big_list, 1)] = cell;
      continue;
    }
    double* tile = BIG ? slots + (size_t)blockIdx.x * p.slot_elems : tile_s;
    const int cs = d0 + lt;  // this cell's detections: order[cs .. cs + D)
    for (int g = lane; g < G; g += kWave) {
      const double ar = b.gt_area[g0 + g];
      const bool crowd = b.gt_crowd[g0 + g] != 0;
      uint32_t f = (crowd ? kFlagCrowd : 0u) | (b.gt_id[g0 + g] != 0 ? kFlagIdNz : 0u);
      for (int a = 0; a < A; ++a)
        if (crowd || ar < p.lo[a] || ar > p.hi[a]) f |= 1u << a;
      gfl[g] = f;
    }
    for (int w = 0; w < (G + 31) / 32; ++w) gm[w][lane] = 0u;
    for (int idx = lane; idx < D * G; idx += kWave) {
      const int d = idx / G, g = idx - d * G;
      double db[4];
      det_xywh(b.dets + (size_t)order[cs + d] * 5, db);
      tile[idx] = bb_iou(db, b.gt_box + (size_t)(g0 + g) * 4, b.gt_crowd[g0 + g] != 0);
    }
    __syncthreads();
    const bool active = lane < p.T * A;
    const int t = active ? lane / A : 0, a = active ? lane - t * A : 0;
    const double lo = p.lo[a], hi = p.hi[a];
    for (int d = 0; d < D; ++d) {
      const int i = order[cs + d];
      double db[4];
      det_xywh(b.dets + (size_t)i * 5, db);
      const double da = db[2] * db[3];
      const double* row = tile + (size_t)d * G;
      bool mbit = false, ibit = false;
      if (active) {
        // evaluateImg with the GTs stably reordered non-ignored first: the
        // ignored ones are visited only while nothing is matched ("break")
        double iou = p.iou0[t];
        int m = -1;
        for (int pass = 0; pass < 2 && m < 0; ++pass) {
          for (int g = 0; g < G; ++g) {
            const uint32_t f = gfl[g];
            if ((int)((f >> a) & 1u) != pass) continue;
            if (((gm[g >> 5][lane] >> (g & 31)) & 1u) && !(f & kFlagCrowd)) continue;
            const double v = row[g];
            if (v < iou) continue;
            iou = v;
            m = g;
          }
        }
        if (m >= 0) {
          gm[m >> 5][lane] |= 1u << (m & 31);
          mbit = (gfl[m] & kFlagIdNz) != 0;  // dtm = gt id: id 0 reads as unmatched
          ibit = (gfl[m] >> a) & 1u;
        }
        if (!mbit && (da < lo || da > hi)) ibit = true;
      }
      const uint64_t mb = __ballot(mbit), ib = __ballot(ibit);
      if (lane == 0) {
        rec_match[i] = mb;
        rec_ign[i] = ib;
      }
    }
    __syncthreads();  // the next cell rewrites the tile and the flags
  }
}

// ------------------------------------------------------ error analysis ----
constexpr uint32_t kFlagOwn = 1u << 10;  // a GT of the cell's own category
constexpr uint32_t kFlagSim = 1u << 11;  // another category, same supercategory

// the image-major GT span of ld_coco_err_batch_t (device pointers)
struct ErrGts {
  const double* box;
  const double* area;
  const int32_t* crowd;
  const int64_t* id;
  const int32_t* cat;
  const int32_t* img_off;
  const int32_t* cat_sup;
  int max_img_gts;
};

// As coco_match_kernel, over the image's GT span; rows t < T0 plain, T0 Sim,
// T0 + 1 Oth (file comment).  BIG: the queued cells, one global tile per
// workgroup.
template <bool BIG>
__global__ __launch_bounds__(kWave) void coco_match_errors_kernel(
    ld_coco_batch_t b, ErrGts eg, MatchParams p, int T0, const int32_t* order,
    int32_t* big_list, double* slots, uint64_t* rec_match, uint64_t* rec_ign,
    int32_t* npig) {
  constexpr int GMAX = BIG ? LD_COCO_MAX_CELL_GTS : kLdsG;
  __shared__ double tile_s[BIG ? 1 : kLdsTile];
  __shared__ uint32_t gfl[GMAX];
  __shared__ uint32_t gm[GMAX / 32][kWave];
  const int lane = threadIdx.x;
  const int K = p.K, A = p.A;
  const int n_cells = BIG ? big_list[0] : 1;
  for (int e = BIG ? blockIdx.x : 0; e < n_cells; e += BIG ? gridDim.x : 1) {
    const int cell = BIG ? big_list[1 + e] : blockIdx.x;
    const int bi = cell / K, k = cell - bi * K;
    const int d0 = b.det_off[bi], d1 = b.det_off[bi + 1];
    int lt = 0, eq = 0;
    for (int j = d0 + lane; j < d1; j += kWave) {
      const int kj = det_cat(b, j);
      lt += (kj >= 0 && kj < k);
      eq += (kj == k);
    }
    lt = wave_sum(lt);
    eq = wave_sum(eq);
    const int D = min(min(eq, p.max_det), p.max_d);
    const int ir = b.img_rank[bi];
    const int g0 = eg.img_off[ir];
    const int G = min(eg.img_off[ir + 1] - g0, eg.max_img_gts);
    if (!BIG && lane < A) {
      int c = 0;
      for (int g = 0; g < G; ++g) {
        if (eg.cat[g0 + g] != k) continue;
        const double ar = eg.area[g0 + g];
        c += !eg.crowd[g0 + g] && !(ar < p.lo[lane] || ar > p.hi[lane]);
      }
      if (c) atomicAdd(npig + k * A + lane, c);
    }
    if (D == 0) continue;
    if (!BIG && (G > kLdsG || (long long)D * G > kLdsTile)) {
      if (lane == 0) big_list[1 + atomicAdd(big_list, 1)] = cell;
      continue;
    }
    double* tile = BIG ? slots + (size_t)blockIdx.x * p.slot_elems : tile_s;
    const int cs = d0 + lt;
    const int sk = eg.cat_sup[k];
    for (int g = lane; g < G; g += kWave) {
      const int c = eg.cat[g0 + g];
      uint32_t f = eg.id[g0 + g] != 0 ? kFlagIdNz : 0u;
      if (c == k) {
        const double ar = eg.area[g0 + g];
        const bool crowd = eg.crowd[g0 + g] != 0;
        f |= kFlagOwn | (crowd ? kFlagCrowd : 0u);
        for (int a = 0; a < A; ++a)
          if (crowd || ar < p.lo[a] || ar > p.hi[a]) f |= 1u << a;
      } else {  // relabelled: crowd, ignored in every area range
        f |= kFlagCrowd | ((1u << A) - 1u);
        if (c >= 0 && c < K && sk >= 0 && eg.cat_sup[c] == sk) f |= kFlagSim;
      }
      gfl[g] = f;
    }
    for (int w = 0; w < (G + 31) / 32; ++w) gm[w][lane] = 0u;
    __syncthreads();  // gfl is read by every lane below
    for (int idx = lane; idx < D * G; idx += kWave) {
      const int d = idx / G, g = idx - d * G;
      double db[4];
      det_xywh(b.dets + (size_t)order[cs + d] * 5, db);
      tile[idx] = bb_iou(db, eg.box + (size_t)(g0 + g) * 4, (gfl[g] & kFlagCrowd) != 0);
    }
    __syncthreads();
    const bool active = lane < p.T * A;
    const int t = active ? lane / A : 0, a = active ? lane - t * A : 0;
    // the GTs row t sees: own only, own + Sim, or all (mem == 0)
    const uint32_t mem = t < T0 ? kFlagOwn : (t == T0 ? (kFlagOwn | kFlagSim) : 0u);
    const double lo = p.lo[a], hi = p.hi[a];
    for (int d = 0; d < D; ++d) {
      const int i = order[cs + d];
      double db[4];
      det_xywh(b.dets + (size_t)i * 5, db);
      const double da = db[2] * db[3];
      const double* row = tile + (size_t)d * G;
      bool mbit = false, ibit = false;
      if (active) {
        double iou = p.iou0[t];
        int m = -1;
        for (int pass = 0; pass < 2 && m < 0; ++pass) {
          for (int g = 0; g < G; ++g) {
            const uint32_t f = gfl[g];
            if (mem && !(f & mem)) continue;
            if ((int)((f >> a) & 1u) != pass) continue;
            if (((gm[g >> 5][lane] >> (g & 31)) & 1u) && !(f & kFlagCrowd)) continue;
            const double v = row[g];
            if (v < iou) continue;
            iou = v;
            m = g;
          }
        }
        if (m >= 0) {
          gm[m >> 5][lane] |= 1u << (m & 31);
          mbit = (gfl[m] & kFlagIdNz) != 0;
          ibit = (gfl[m] >> a) & 1u;
        }
        if (!mbit && (da < lo || da > hi)) ibit = true;
      }
      const uint64_t mb = __ballot(mbit), ib = __ballot(ibit);
      if (lane == 0) {
        rec_match[i] = mb;
        rec_ign[i] = ib;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------- sort ------
__global__ void acc_keys_kernel(int n, int K, const float* score, const int32_t* cat,
                                const uint32_t* pos, uint64_t* hi, uint32_t* lo,
                                uint32_t* val) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = (uint32_t)min(max(cat[i], 0), K);
  hi[i] = ((uint64_t)k << 32) | desc_key(score[i]);
  lo[i] = pos[i];
  val[i] = (uint32_t)i;
}

// max over the LATER threads of the block (exclusive suffix max); -1 if none
__device__ __forceinline__ double block_excl_suffix_max(double v, double* sh) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double x = v;
  for (int off = 1; off < 64; off <<= 1) {
    double y = __shfl_down(x, off, 64);
    if (lane + off < 64) x = fmax(x, y);
  }
  double after = __shfl_down(x, 1, 64);
  if (lane == 63) after = -1.0;
  if (lane == 0) sh[w] = x;
  __syncthreads();
  for (int q = w + 1; q < kThreads / 64; ++q) after = fmax(after, sh[q]);
  __syncthreads();
  return after;
}

__device__ __forceinline__ double block_max(double v, double* sh) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  if (lane == 0) sh[w] = v;
  __syncthreads();
  double t = sh[0];
  for (int q = 1; q < kThreads / 64; ++q) t = fmax(t, sh[q]);
  __syncthreads();
  return t;
}

// one workgroup: seg_start[k] (first sorted record of category >= k, k <= K)
// and tile_off[k] (first tile of category k; tile_off[K] tiles in all)
__global__ __launch_bounds__(kThreads) void acc_segments_kernel(const uint64_t* hi, int n,
                                                               int K, int32_t* seg_start,
                                                               int32_t* tile_off) {
  for (int k = threadIdx.x; k <= K; k += kThreads) {
    int lo = 0, h = n;
    while (lo < h) {
      const int mid = (lo + h) >> 1;
      if ((int)(hi[mid] >> 32) < k) lo = mid + 1;
      else h = mid;
    }
    seg_start[k] = lo;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int k = 0; k < K; ++k) {
      tile_off[k] = acc;
      acc += (seg_start[k + 1] - seg_start[k] + kTile - 1) / kTile;
    }
    tile_off[K] = acc;
  }
}

// precision / scores: -1 where the (category, area) has no non-ignored GT
// (accumulate's `if npig == 0: continue`), else 0 (no searchsorted hit)
__global__ void acc_init_kernel(AccParams p, const int32_t* npig, double* precision,
                                double* scores) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)p.T * p.R * p.K * p.A * p.M;
  if (i >= total) return;
  const int a = (int)((i / p.M) % p.A), k = (int)((i / ((long long)p.M * p.A)) % p.K);
  const double v = npig[k * p.A + a] == 0 ? -1.0 : 0.0;
  precision[i] = v;
  scores[i] = v;
}

struct TileView {
  int k, st, en, r0, r1;  // category, its records [st, en), this tile [r0, r1)
};

__device__ __forceinline__ bool tile_view(const int32_t* seg_start,
                                          const int32_t* tile_off, int K, int tile,
                                          TileView* v) {
  if (tile >= tile_off[K]) return false;
  int lo = 0, hi = K - 1;  // last k with tile_off[k] <= tile
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tile_off[mid] <= tile) lo = mid;
    else hi = mid - 1;
  }
  v->k = lo;  // the last: categories without records own no tiles
  v->st = seg_start[lo];
  v->en = seg_start[lo + 1];
  v->r0 = v->st + (tile - tile_off[lo]) * kTile;
  v->r1 = min(v->r0 + kTile, v->en);
  return true;
}

// lane l = (m * A + a) * T + t; its bit in the match / ignore masks is t * A + a
__device__ __forceinline__ void lane_split(const AccParams& p, int l, int* t, int* a,
                                           int* m) {
  *t = l % p.T;
  *a = (l / p.T) % p.A;
  *m = l / (p.T * p.A);
}

// per thread's kItems records of the tile: packed (fp << 16 | tp) increments of
// lane l, and whether each record is in the maxDets[m] slice
__device__ __forceinline__ int lane_incs(const AccParams& p, int l, const uint64_t* mb,
                                         const uint64_t* ib, const int* rank, int nvalid,
                                         int* inc) {
  int t, a, m;
  lane_split(p, l, &t, &a, &m);
  const int bit = t * p.A + a, md = p.max_dets[m];
  int s = 0;
#pragma unroll
  for (int q = 0; q < kItems; ++q) {
    int v = -1;  // not in the slice
    if (q < nvalid && rank[q] < md) {
      const bool ig = (ib[q] >> bit) & 1ull, mt = (mb[q] >> bit) & 1ull;
      v = ig ? 0 : (mt ? 1 : (1 << 16));
      s += v;
    }
    inc[q] = v;
  }
  return s;
}

__device__ __forceinline__ void load_records(const TileView& v, const uint32_t* lo_sorted,
                                             const uint32_t* val, const uint64_t* rec_match,
                                             const uint64_t* rec_ign, int max_det,
                                             uint64_t* mb, uint64_t* ib, int* rank,
                                             int* nvalid) {
  const int i0 = v.r0 + threadIdx.x * kItems;
  *nvalid = max(0, min(kItems, v.r1 - i0));
#pragma unroll
  for (int q = 0; q < kItems; ++q) {
    if (q < *nvalid) {
      const uint32_t r = val[i0 + q];
      mb[q] = rec_match[r];
      ib[q] = rec_ign[r];
      rank[q] = (int)(lo_sorted[i0 + q] % (uint32_t)max_det);
    } else {
      mb[q] = ib[q] = 0ull;
      rank[q] = 0;
    }
  }
}

__global__ __launch_bounds__(kThreads) void acc_count_kernel(
    AccParams p, const int32_t* seg_start, const int32_t* tile_off,
    const uint32_t* lo_sorted, const uint32_t* val, const uint64_t* rec_match,
    const uint64_t* rec_ign, int32_t* cnt_tp, int32_t* cnt_fp) {
  __shared__ int sh[kThreads / 64][kMaxLanes];
  TileView v;
  if (!tile_view(seg_start, tile_off, p.K, blockIdx.x, &v)) return;
  uint64_t mb[kItems], ib[kItems];
  int rank[kItems], nvalid, inc[kItems];
  load_records(v, lo_sorted, val, rec_match, rec_ign, p.max_det, mb, ib, rank, &nvalid);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int l = 0; l < p.L; ++l) {
    int s = lane_incs(p, l, mb, ib, rank, nvalid, inc);
    s = wave_sum(s);
    if (lane == 0) sh[w][l] = s;
  }
  __syncthreads();
  for (int l = threadIdx.x; l < p.L; l += kThreads) {
    int s = 0;
    for (int q = 0; q < kThreads / 64; ++q) s += sh[q][l];
    cnt_tp[(size_t)l * p.nt + blockIdx.x] = s & 0xffff;
    cnt_fp[(size_t)l * p.nt + blockIdx.x] = s >> 16;
  }
}

// one workgroup, thread per lane: tile counts -> exclusive prefix inside each
// category (in place); recall = rc[-1] (or 0 without detections, -1 when npig
// is 0)
__global__ __launch_bounds__(kThreads) void acc_prefix_kernel(
    AccParams p, const int32_t* seg_start, const int32_t* tile_off, const int32_t* npig,
    int32_t* cnt_tp, int32_t* cnt_fp, double* recall) {
  for (int l = threadIdx.x; l < p.L; l += kThreads) {
    int t, a, m;
    lane_split(p, l, &t, &a, &m);
    int32_t* ct = cnt_tp + (size_t)l * p.nt;
    int32_t* cf = cnt_fp + (size_t)l * p.nt;
    for (int k = 0; k < p.K; ++k) {
      int tp = 0, fp = 0;
      for (int j = tile_off[k]; j < tile_off[k + 1]; ++j) {
        const int x = ct[j], y = cf[j];
        ct[j] = tp;
        cf[j] = fp;
        tp += x;
        fp += y;
      }
      const int np = npig[k * p.A + a];
      const bool nd = seg_start[k + 1] > seg_start[k];
      recall[(((size_t)t * p.K + k) * p.A + a) * p.M + m] =
          np == 0 ? -1.0 : (nd ? (double)tp / (double)np : 0.0);
    }
  }
}

// cumulative TP / FP of lane l for this thread's records, and pr (-1 outside
// the slice); returns the thread's maximum pr
__device__ __forceinline__ double lane_pr(const AccParams& p, int l, const uint64_t* mb,
                                          const uint64_t* ib, const int* rank, int nvalid,
                                          int tp0, int fp0, int* sh, int* tpc,
                                          double* pr) {
  int inc[kItems];
  const int s = lane_incs(p, l, mb, ib, rank, nvalid, inc);
  int tot;
  const int pre = block_excl_scan(s, sh, &tot);
  int tp = tp0 + (pre & 0xffff), fp = fp0 + (pre >> 16);
  double mx = -1.0;
#pragma unroll
  for (int q = 0; q < kItems; ++q) {
    pr[q] = -1.0;
    tpc[q] = -1;
    if (inc[q] < 0) continue;
    tp += inc[q] & 0xffff;
    fp += inc[q] >> 16;
    const double dtp = (double)tp, dfp = (double)fp;
    pr[q] = dtp / (dfp + dtp + DBL_EPSILON);  // tp / (fp + tp + np.spacing(1))
    tpc[q] = tp;
    mx = fmax(mx, pr[q]);
  }
  return mx;
}

__global__ __launch_bounds__(kThreads) void acc_max_kernel(
    AccParams p, const int32_t* seg_start, const int32_t* tile_off,
    const uint32_t* lo_sorted, const uint32_t* val, const uint64_t* rec_match,
    const uint64_t* rec_ign, const int32_t* cnt_tp, const int32_t* cnt_fp, double* tmax) {
  __shared__ int sh[kThreads / 64];
  __shared__ double shd[kThreads / 64];
  TileView v;
  if (!tile_view(seg_start, tile_off, p.K, blockIdx.x, &v)) return;
  uint64_t mb[kItems], ib[kItems];
  int rank[kItems], nvalid, tpc[kItems];
  double pr[kItems];
  load_records(v, lo_sorted, val, rec_match, rec_ign, p.max_det, mb, ib, rank, &nvalid);
  for (int l = 0; l < p.L; ++l) {
    const size_t at = (size_t)l * p.nt + blockIdx.x;
    const double mx =
        lane_pr(p, l, mb, ib, rank, nvalid, cnt_tp[at], cnt_fp[at], sh, tpc, pr);
    const double bm = block_max(mx, shd);
    if (threadIdx.x == 0) tmax[at] = bm;
  }
}

// one workgroup, thread per lane: tmax -> max over the LATER tiles of the same
// category (in place; -1 for the last tile)
__global__ __launch_bounds__(kThreads) void acc_suffix_kernel(AccParams p,
                                                             const int32_t* tile_off,
                                                             double* tmax) {
  for (int l = threadIdx.x; l < p.L; l += kThreads) {
    double* x = tmax + (size_t)l * p.nt;
    for (int k = 0; k < p.K; ++k) {
      double run = -1.0;
      for (int j = tile_off[k + 1] - 1; j >= tile_off[k]; --j) {
        const double y = x[j];
        x[j] = run;
        run = fmax(run, y);
      }
    }
  }
}

// first r with rec[r] > x (rec sorted ascending)
__device__ __forceinline__ int rec_upper(const AccParams& p, double x) {
  int lo = 0, hi = p.R;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (p.rec[mid] > x) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void acc_final_kernel(
    AccParams p, const int32_t* seg_start, const int32_t* tile_off,
    const uint32_t* lo_sorted, const uint32_t* val, const float* rec_score,
    const uint64_t* rec_match, const uint64_t* rec_ign, const int32_t* cnt_tp,
    const int32_t* cnt_fp, const double* after, const int32_t* npig, double* precision,
    double* scores) {
  __shared__ int sh[kThreads / 64];
  __shared__ double shd[kThreads / 64];
  TileView v;
  if (!tile_view(seg_start, tile_off, p.K, blockIdx.x, &v)) return;
  uint64_t mb[kItems], ib[kItems];
  int rank[kItems], nvalid, tpc[kItems];
  double pr[kItems];
  load_records(v, lo_sorted, val, rec_match, rec_ign, p.max_det, mb, ib, rank, &nvalid);
  const int i0 = v.r0 + threadIdx.x * kItems;
  for (int l = 0; l < p.L; ++l) {
    int t, a, m;
    lane_split(p, l, &t, &a, &m);
    const int np = npig[v.k * p.A + a];
    const size_t at = (size_t)l * p.nt + blockIdx.x;
    const double mx =
        lane_pr(p, l, mb, ib, rank, nvalid, cnt_tp[at], cnt_fp[at], sh, tpc, pr);
    double env = fmax(block_excl_suffix_max(mx, shd), after[at]);
    if (np == 0) continue;  // uniform across the block: after the barriers
    const double dnp = (double)np;
    const int bit = t * p.A + a;
#pragma unroll
    for (int q = kItems - 1; q >= 0; --q) {
      if (tpc[q] < 0) continue;
      env = fmax(env, pr[q]);  // pr[i - 1] = max(pr[i - 1], pr[i]) from the end
      // searchsorted(rc, recThrs, 'left') picks this record for every r with
      // rc[i - 1] < recThrs[r] <= rc[i]; rc only grows at a TP, and the first
      // record of the category takes every r up to rc[0]
      const bool first = i0 + q == v.st;
      const bool is_tp = ((mb[q] >> bit) & 1ull) && !((ib[q] >> bit) & 1ull);
      if (!first && !is_tp) continue;
      const double cur = (double)tpc[q] / dnp;  // rc = tp / npig
      const int r0 = first ? 0 : rec_upper(p, (double)(tpc[q] - 1) / dnp);
      const int r1 = rec_upper(p, cur);
      const double sc = (double)rec_score[val[i0 + q]];
      for (int r = r0; r < r1; ++r) {
        const size_t o = ((((size_t)t * p.R + r) * p.K + v.k) * p.A + a) * p.M + m;
        precision[o] = env;
        scores[o] = sc;
      }
    }
  }
}

struct MatchPlan {
  size_t order, big, slots, total;
};

MatchPlan match_plan(int num_dets, int max_d, int max_cell_gts) {
  MatchPlan o{};
  ldeval::Carver ws;
  o.order = ws.take((size_t)num_dets * 4);
  o.big = ws.take(((size_t)num_dets + 1) * 4);
  const bool may_spill = max_cell_gts > kLdsG || (long long)max_d * max_cell_gts > kLdsTile;
  o.slots = ws.take(may_spill ? (size_t)kSlots * max_d * max_cell_gts * 8 : 0);
  o.total = ws.off;
  return o;
}

struct AccPlan {
  size_t hi0, hi1, lo0, lo1, val0, val1, hist, seg, toff, ctp, cfp, tmax, total;
  int nb, nt;
};

AccPlan acc_plan(int n, int K, int L) {
  AccPlan o{};
  o.nb = ldeval::sort_tiles(n);
  o.nt = (n + kTile - 1) / kTile + K;  // tiles never straddle categories
  ldeval::Carver ws;
  o.hi0 = ws.take((size_t)n * 8);
  o.hi1 = ws.take((size_t)n * 8);
  o.lo0 = ws.take((size_t)n * 4);
  o.lo1 = ws.take((size_t)n * 4);
  o.val0 = ws.take((size_t)n * 4);
  o.val1 = ws.take((size_t)n * 4);
  o.hist = ws.take((size_t)ldeval::kBins * o.nb * 4);
  o.seg = ws.take(((size_t)K + 1) * 4);
  o.toff = ws.take(((size_t)K + 1) * 4);
  o.ctp = ws.take((size_t)L * o.nt * 4);
  o.cfp = ws.take((size_t)L * o.nt * 4);
  o.tmax = ws.take((size_t)L * o.nt * 8);
  o.total = ws.off;
  return o;
}

int bits_for(unsigned long long x) {  // bits to hold values < x
  int b = 0;
  while (b < 64 && (1ull << b) < x) ++b;
  return b;
}

}  // namespace

extern "C" {

size_t ld_coco_match_workspace_bytes(int num_dets, int max_img_dets, int max_det,
                                     int max_cell_gts) {
  if (num_dets < 0 || max_img_dets < 0 || max_det < 1 || max_cell_gts < 0 ||
      max_cell_gts > LD_COCO_MAX_CELL_GTS)
    return 0;
  return match_plan(num_dets, std::min(max_det, max_img_dets), max_cell_gts).total + 256;
}

int ld_coco_match(const ld_coco_batch_t* b, int num_thrs, const double* iou_thrs,
                  int num_areas, const double* area_rng, int max_det, float* rec_score,
                  int32_t* rec_cat, uint32_t* rec_pos, uint64_t* rec_match,
                  uint64_t* rec_ign, int32_t* npig, void* workspace,
                  size_t workspace_bytes, ld_stream_t stream_) {
  if (!b || !iou_thrs || !area_rng || !npig) return LD_EINVAL;
  if (num_thrs < 1 || num_thrs > LD_COCO_MAX_THRS || num_areas < 1 ||
      num_areas > LD_COCO_MAX_AREAS || num_thrs * num_areas > 64 || max_det < 1)
    return LD_EINVAL;
  if (b->num_imgs < 1 || b->num_dets < 0 || b->num_labels < 0 || b->max_img_dets < 0 ||
      b->num_all_imgs < 1 || b->num_cats < 1 || b->num_gts < 0 || b->max_cell_gts < 0)
    return LD_EINVAL;
  if (b->max_cell_gts > LD_COCO_MAX_CELL_GTS) return LD_EUNSUPPORTED;
  if ((long long)b->num_imgs * b->num_cats >= (1ll << 31) ||
      (long long)b->num_all_imgs * max_det >= (1ll << 32))
    return LD_EUNSUPPORTED;
  if (!b->det_off || !b->img_rank || !b->gt_cell_off) return LD_EINVAL;
  if (b->num_dets && (!b->dets || !b->labels || !rec_score || !rec_cat || !rec_pos ||
                      !rec_match || !rec_ign || (b->num_labels && !b->label_cat)))
    return LD_EINVAL;
  if (b->num_gts && (!b->gt_box || !b->gt_area || !b->gt_crowd || !b->gt_id))
    return LD_EINVAL;
  const int max_d = std::min(max_det, b->max_img_dets);
  const MatchPlan o = match_plan(b->num_dets, max_d, b->max_cell_gts);
  if (workspace_bytes < o.total || (o.total && !workspace)) return LD_ENOSPACE;
  MatchParams p{};
  for (int t = 0; t < num_thrs; ++t) p.iou0[t] = std::min(iou_thrs[t], 1.0 - 1e-10);
  for (int a = 0; a < num_areas; ++a) {
    p.lo[a] = area_rng[2 * a];
    p.hi[a] = area_rng[2 * a + 1];
  }
  p.T = num_thrs;
  p.A = num_areas;
  p.K = b->num_cats;
  p.max_det = max_det;
  p.max_d = max_d;
  p.slot_elems = (long long)max_d * b->max_cell_gts;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  int32_t* order = (int32_t*)(ws + o.order);
  int32_t* big = (int32_t*)(ws + o.big);
  double* slots = (double*)(ws + o.slots);
  hipError_t e = ldrec::memset_async(big, 0, 4, stream);
  if (e != hipSuccess) return (int)e;
  if (b->num_dets > 0)
    LD_LAUNCH(coco_rank_kernel, dim3((b->num_dets + 255) / 256), dim3(256), 0, stream, *b,
              p, order, rec_score, rec_cat, rec_pos, rec_match, rec_ign);
  LD_LAUNCH(coco_match_kernel<false>, dim3(b->num_imgs * b->num_cats), dim3(kWave), 0,
            stream, *b, p, (const int32_t*)order, big, slots, rec_match, rec_ign, npig);
  if (b->num_dets > 0 && o.slots != o.total)
    LD_LAUNCH(coco_match_kernel<true>, dim3(kSlots), dim3(kWave), 0, stream, *b, p,
              (const int32_t*)order, big, slots, rec_match, rec_ign, npig);
  return (int)hipGetLastError();
}

size_t ld_coco_match_errors_workspace_bytes(int num_dets, int max_img_dets, int max_det,
                                            int max_img_gts) {
  return ld_coco_match_workspace_bytes(num_dets, max_img_dets, max_det, max_img_gts);
}

int ld_coco_match_errors(const ld_coco_err_batch_t* e, int num_thrs, const double* iou_thrs,
                         double err_thr, int num_areas, const double* area_rng, int max_det,
                         float* rec_score, int32_t* rec_cat, uint32_t* rec_pos,
                         uint64_t* rec_match, uint64_t* rec_ign, int32_t* npig,
                         void* workspace, size_t workspace_bytes, ld_stream_t stream_) {
  if (!e || !iou_thrs || !area_rng || !npig) return LD_EINVAL;
  const int T = num_thrs + 2;  // + Sim + Oth
  if (num_thrs < 1 || T > LD_COCO_MAX_THRS || num_areas < 1 ||
      num_areas > LD_COCO_MAX_AREAS || T * num_areas > 64 || max_det < 1)
    return LD_EINVAL;
  if (e->num_imgs < 1 || e->num_dets < 0 || e->num_labels < 0 || e->max_img_dets < 0 ||
      e->num_all_imgs < 1 || e->num_cats < 1 || e->num_gts < 0 || e->max_img_gts < 0)
    return LD_EINVAL;
  if (e->max_img_gts > LD_COCO_MAX_CELL_GTS) return LD_EUNSUPPORTED;
  if ((long long)e->num_imgs * e->num_cats >= (1ll << 31) ||
      (long long)e->num_all_imgs * max_det >= (1ll << 32))
    return LD_EUNSUPPORTED;
  if (!e->det_off || !e->img_rank || !e->gt_img_off || !e->cat_sup) return LD_EINVAL;
  if (e->num_dets && (!e->dets || !e->labels || !rec_score || !rec_cat || !rec_pos ||
                      !rec_match || !rec_ign || (e->num_labels && !e->label_cat)))
    return LD_EINVAL;
  if (e->num_gts && (!e->gt_box || !e->gt_area || !e->gt_crowd || !e->gt_id || !e->gt_cat))
    return LD_EINVAL;
  const int max_d = std::min(max_det, e->max_img_dets);
  const MatchPlan o = match_plan(e->num_dets, max_d, e->max_img_gts);
  if (workspace_bytes < o.total || (o.total && !workspace)) return LD_ENOSPACE;
  MatchParams p{};
  for (int t = 0; t < num_thrs; ++t) p.iou0[t] = std::min(iou_thrs[t], 1.0 - 1e-10);
  p.iou0[num_thrs] = p.iou0[num_thrs + 1] = std::min(err_thr, 1.0 - 1e-10);
  for (int a = 0; a < num_areas; ++a) {
    p.lo[a] = area_rng[2 * a];
    p.hi[a] = area_rng[2 * a + 1];
  }
  p.T = T;
  p.A = num_areas;
  p.K = e->num_cats;
  p.max_det = max_det;
  p.max_d = max_d;
  p.slot_elems = (long long)max_d * e->max_img_gts;
  // the detection half as ld_coco_match reads it (no cell-grouped GTs)
  ld_coco_batch_t b{};
  b.dets = e->dets;
  b.labels = e->labels;
  b.det_off = e->det_off;
  b.img_rank = e->img_rank;
  b.label_cat = e->label_cat;
  b.num_imgs = e->num_imgs;
  b.num_dets = e->num_dets;
  b.num_labels = e->num_labels;
  b.max_img_dets = e->max_img_dets;
  b.num_all_imgs = e->num_all_imgs;
  b.num_cats = e->num_cats;
  const ErrGts eg{e->gt_box, e->gt_area, e->gt_crowd, e->gt_id, e->gt_cat,
                  e->gt_img_off, e->cat_sup, e->max_img_gts};
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  int32_t* order = (int32_t*)(ws + o.order);
  int32_t* big = (int32_t*)(ws + o.big);
  double* slots = (double*)(ws + o.slots);
  hipError_t err = ldrec::memset_async(big, 0, 4, stream);
  if (err != hipSuccess) return (int)err;
  if (b.num_dets > 0)
    LD_LAUNCH(coco_rank_kernel, dim3((b.num_dets + 255) / 256), dim3(256), 0, stream, b, p,
              order, rec_score, rec_cat, rec_pos, rec_match, rec_ign);
  LD_LAUNCH(coco_match_errors_kernel<false>, dim3(b.num_imgs * b.num_cats), dim3(kWave), 0,
            stream, b, eg, p, num_thrs, (const int32_t*)order, big, slots, rec_match,
            rec_ign, npig);
  if (b.num_dets > 0 && o.slots != o.total)
    LD_LAUNCH(coco_match_errors_kernel<true>, dim3(kSlots), dim3(kWave), 0, stream, b, eg,
              p, num_thrs, (const int32_t*)order, big, slots, rec_match, rec_ign, npig);
  return (int)hipGetLastError();
}

size_t ld_coco_accumulate_workspace_bytes(int num_records, int num_cats, int num_thrs,
                                          int num_areas, int num_max_dets) {
  if (num_records < 0 || num_cats < 1 || num_thrs < 1 || num_thrs > LD_COCO_MAX_THRS ||
      num_areas < 1 || num_areas > LD_COCO_MAX_AREAS || num_max_dets < 1 ||
      num_max_dets > LD_COCO_MAX_MAXDETS)
    return 0;
  return acc_plan(num_records, num_cats, num_thrs * num_areas * num_max_dets).total + 256;
}

int ld_coco_accumulate(int num_records, const float* rec_score, const int32_t* rec_cat,
                       const uint32_t* rec_pos, const uint64_t* rec_match,
                       const uint64_t* rec_ign, int num_cats, int num_all_imgs,
                       int num_thrs, int num_areas, int num_max_dets,
                       const int32_t* max_dets, int num_rec_thrs, const double* rec_thrs,
                       const int32_t* npig, double* precision, double* recall,
                       double* scores, void* workspace, size_t workspace_bytes,
                       ld_stream_t stream_) {
  const int n = num_records, K = num_cats;
  if (n < 0 || K < 1 || num_all_imgs < 1 || num_thrs < 1 ||
      num_thrs > LD_COCO_MAX_THRS || num_areas < 1 || num_areas > LD_COCO_MAX_AREAS ||
      num_thrs * num_areas > 64 || num_max_dets < 1 || num_max_dets > LD_COCO_MAX_MAXDETS ||
      num_rec_thrs < 1 || num_rec_thrs > LD_COCO_MAX_REC_THRS)
    return LD_EINVAL;
  if (!max_dets || !rec_thrs || !npig || !precision || !recall || !scores) return LD_EINVAL;
  if (n > 0 && (!rec_score || !rec_cat || !rec_pos || !rec_match || !rec_ign))
    return LD_EINVAL;
  AccParams p{};
  for (int m = 0; m < num_max_dets; ++m) {
    if (max_dets[m] < 1 || (m && max_dets[m] < max_dets[m - 1])) return LD_EINVAL;
    p.max_dets[m] = max_dets[m];
  }
  for (int r = 0; r < num_rec_thrs; ++r) {
    if (r && !(rec_thrs[r] >= rec_thrs[r - 1])) return LD_EINVAL;
    p.rec[r] = rec_thrs[r];
  }
  const int max_det = max_dets[num_max_dets - 1];
  if ((long long)num_all_imgs * max_det >= (1ll << 32) || K >= (1 << 24))
    return LD_EUNSUPPORTED;
  p.T = num_thrs;
  p.A = num_areas;
  p.M = num_max_dets;
  p.R = num_rec_thrs;
  p.K = K;
  p.L = num_thrs * num_areas * num_max_dets;
  p.n = n;
  p.max_det = max_det;
  const AccPlan o = acc_plan(n, K, p.L);
  p.nt = o.nt;
  if (workspace_bytes < o.total || (o.total && !workspace)) return LD_ENOSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  const ldeval::SortKeys<true> keys[2] = {
      {(uint64_t*)(ws + o.hi0), (uint32_t*)(ws + o.lo0)},
      {(uint64_t*)(ws + o.hi1), (uint32_t*)(ws + o.lo1)}};
  uint32_t* const val[2] = {(uint32_t*)(ws + o.val0), (uint32_t*)(ws + o.val1)};
  int32_t* hist = (int32_t*)(ws + o.hist);
  int32_t* seg = (int32_t*)(ws + o.seg);
  int32_t* toff = (int32_t*)(ws + o.toff);
  int32_t* ctp = (int32_t*)(ws + o.ctp);
  int32_t* cfp = (int32_t*)(ws + o.cfp);
  double* tmax = (double*)(ws + o.tmax);
  const long long total = (long long)p.T * p.R * K * p.A * p.M;
  LD_LAUNCH(acc_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
            p, npig, precision, scores);
  int cur = 0;
  if (n > 0) {
    LD_LAUNCH(acc_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, K,
              rec_score, rec_cat, rec_pos, keys[0].hi, keys[0].lo, val[0]);
    constexpr int kRadixBits = ldeval::kRadixBits;
    const int lo_passes =
        (bits_for((unsigned long long)num_all_imgs * max_det) + kRadixBits - 1) / kRadixBits;
    const int hi_passes = (32 + bits_for((unsigned long long)K + 1) + kRadixBits - 1) /
                          kRadixBits;
    cur = ldeval::radix_sort(keys, val, n, lo_passes, hi_passes, hist, stream);
  }
  LD_LAUNCH(acc_segments_kernel, dim3(1), dim3(kThreads), 0, stream,
            (const uint64_t*)keys[cur].hi, n, K, seg, toff);
  if (n > 0) {
    LD_LAUNCH(acc_count_kernel, dim3(o.nt), dim3(kThreads), 0, stream, p,
              (const int32_t*)seg, (const int32_t*)toff, (const uint32_t*)keys[cur].lo,
              (const uint32_t*)val[cur], rec_match, rec_ign, ctp, cfp);
  }
  LD_LAUNCH(acc_prefix_kernel, dim3(1), dim3(kThreads), 0, stream, p, (const int32_t*)seg,
            (const int32_t*)toff, npig, ctp, cfp, recall);
  if (n > 0) {
    LD_LAUNCH(acc_max_kernel, dim3(o.nt), dim3(kThreads), 0, stream, p,
              (const int32_t*)seg, (const int32_t*)toff, (const uint32_t*)keys[cur].lo,
              (const uint32_t*)val[cur], rec_match, rec_ign, (const int32_t*)ctp,
              (const int32_t*)cfp, tmax);
    LD_LAUNCH(acc_suffix_kernel, dim3(1), dim3(kThreads), 0, stream, p,
              (const int32_t*)toff, tmax);
    LD_LAUNCH(acc_final_kernel, dim3(o.nt), dim3(kThreads), 0, stream, p,
              (const int32_t*)seg, (const int32_t*)toff, (const uint32_t*)keys[cur].lo,
              (const uint32_t*)val[cur], rec_score, rec_match, rec_ign,
              (const int32_t*)ctp, (const int32_t*)cfp, (const double*)tmax, npig,
              precision, scores);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
