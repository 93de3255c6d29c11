// Scalar math shared by the LD loss / target kernels.
//
// Every function is `LD_HD` (host + device) and free of wave intrinsics so the
// exact same arithmetic can be compiled by g++ into the host-side unit-test
// harness (tests/host_harness.cpp, CPU tests only) and by hipcc into the
// gfx950 kernels (the product).  Reference formulas are cited per function
// (paths relative to the reference checkout).
//
// This translation unit family is compiled with -ffp-contract=off: target
// assignment must reproduce the reference's fp32 op sequence bit-for-bit
// (SURVEY.md K12), which an FMA contraction would break.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LD_HD __host__ __device__ __forceinline__
#else
#define LD_HD inline
#endif

namespace ld {

constexpr int kRegBins = 17;   // reg_max + 1 (gfl_head.py:86 reg_max=16)
constexpr float kNegInf = -100000000.0f;  // atss_assigner.py:63 INF

struct Box {
  float x1, y1, x2, y2;
};

LD_HD float fmaxf_(float a, float b) { return a > b ? a : b; }
LD_HD float fminf_(float a, float b) { return a < b ? a : b; }

// Mean over W virtual ranks of one column of a (W, n) table (ld_vrank_reduce,
// optim.hip): the fp32 sum in ASCENDING rank order, then one division by W -- what
// all_reduce(SUM) followed by div_(world) leaves on every rank of a W-process job
// (core/utils/dist_utils.py:63-69, base.py:211-214).  `col` points at row 0.
LD_HD float vrank_mean(const float* col, int W, size_t row_stride) {
  float acc = col[0];
  for (int r = 1; r < W; ++r) acc += col[(size_t)r * row_stride];
  return acc / (float)W;
}

// Anchor of level stride `s` at grid cell (x, y): square of side 8*s centred on
// (x*s, y*s) -- anchor_generator.py:142-185 (center_offset = 0,
// octave_base_scale = 8, ratio 1) and :229-270 (shift + base anchor).
LD_HD Box anchor_box(int x, int y, int stride, float half_side) {
  float cx = (float)(x * stride), cy = (float)(y * stride);
  return Box{cx - half_side, cy - half_side, cx + half_side, cy + half_side};
}

// iou2d_calculator.py:111-171, mode 'iou' (pairwise), eps = 1e-6.
LD_HD float iou_pair(const Box& a, const Box& b) {
  float area1 = (a.x2 - a.x1) * (a.y2 - a.y1);
  float area2 = (b.x2 - b.x1) * (b.y2 - b.y1);
  float w = fmaxf_(fminf_(a.x2, b.x2) - fmaxf_(a.x1, b.x1), 0.0f);
  float h = fmaxf_(fminf_(a.y2, b.y2) - fmaxf_(a.y1, b.y1), 0.0f);
  float overlap = w * h;
  float uni = area1 + area2 - overlap;
  uni = fmaxf_(uni, 1e-6f);
  return overlap / uni;
}

// iou2d_calculator.py:123-126,179-188, mode 'diou' -- fork-specific and
// IoF-based (quirk Q1): inter/area(a) - rho^2/c^2.
LD_HD float diou_pair(const Box& a, const Box& b) {
  float area1 = (a.x2 - a.x1) * (a.y2 - a.y1);
  float w = fmaxf_(fminf_(a.x2, b.x2) - fmaxf_(a.x1, b.x1), 0.0f);
  float h = fmaxf_(fminf_(a.y2, b.y2) - fmaxf_(a.y1, b.y1), 0.0f);
  float overlap = w * h;
  float uni = fmaxf_(area1, 1e-6f);
  float ious = overlap / uni;
  float l = (b.x1 + b.x2) - (a.x1 + a.x2);
  float r = (b.y1 + b.y2) - (a.y1 + a.y2);
  float left = (l * l) / 4.0f;
  float right = (r * r) / 4.0f;
  float rho2 = left + right;
  float ew = fmaxf_(fmaxf_(a.x2, b.x2) - fminf_(a.x1, b.x1), 0.0f);
  float eh = fmaxf_(fmaxf_(a.y2, b.y2) - fminf_(a.y1, b.y1), 0.0f);
  float ec = ew * ew + eh * eh;
  ec = fmaxf_(ec, 1e-6f);
  return ious - rho2 / ec;
}

// Centre distance, atss_assigner.py:93-103: (d).pow(2).sum(-1).sqrt()
LD_HD float centre_dist(float ax, float ay, float gx, float gy) {
  float dx = ax - gx, dy = ay - gy;
  float s = dx * dx + dy * dy;
  return sqrtf(s);
}

LD_HD float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// BCE-with-logits(x, 0) = softplus(x), computed as torch does:
// max(x,0) + log1p(exp(-|x|))
LD_HD float softplusf_(float x) {
  return fmaxf_(x, 0.0f) + log1pf(expf(-fabsf(x)));
}

// Quality focal loss element, beta = 2 (gfocal_loss.py:8-50).
//   negative entry : q = softplus(x) * sigma^2
//   positive entry : q = (softplus(x) - s*x) * (s - sigma)^2     (s = score)
// Returns q, writes dq/dx.
LD_HD float qfl_neg(float x, float* dq) {
  float s = sigmoidf_(x), sp = softplusf_(x);
  *dq = s * s * s + 2.0f * s * s * (1.0f - s) * sp;
  return sp * s * s;
}
LD_HD float qfl_pos(float x, float score, float* dq) {
  float s = sigmoidf_(x), sp = softplusf_(x);
  float bce = sp - score * x;
  float d = score - s;
  *dq = (s - score) * d * d - 2.0f * d * s * (1.0f - s) * bce;
  return bce * d * d;
}

// Sigmoid focal loss, gamma = 2 (losses/focal_loss.py:12-47, the pure-torch
// py_sigmoid_focal_loss the reference runs on CPU; the compiled mmcv op computes
// the same function):  bce_with_logits(x, t) * (alpha t + (1 - alpha)(1 - t)) *
// pt^2,  pt = (1 - p) t + p (1 - t).
//   t = 1 : f = alpha (1 - p)^2 softplus(-x),  df/dx = alpha (1 - p)^2 (2 p log p - (1 - p))
//   t = 0 : f = (1 - alpha) p^2 softplus(x),   df/dx = (1 - alpha) p^2 (p - 2 (1 - p) log(1 - p))
// (-log p = softplus(-x), -log(1 - p) = softplus(x))
LD_HD float focal_pos(float x, float alpha, float* df) {
  float p = sigmoidf_(x), spn = softplusf_(-x);
  float q = 1.0f - p;
  *df = alpha * q * q * (-2.0f * p * spn - q);
  return alpha * q * q * spn;
}
LD_HD float focal_neg(float x, float alpha, float* df) {
  float p = sigmoidf_(x), sp = softplusf_(x);
  *df = (1.0f - alpha) * p * p * (p + 2.0f * (1.0f - p) * sp);
  return (1.0f - alpha) * p * p * sp;
}
// binary_cross_entropy_with_logits(x, t) and d/dx (centerness,
// losses/cross_entropy_loss.py:52-90)
LD_HD float bce_logits(float x, float t, float* d) {
  *d = sigmoidf_(x) - t;
  return softplusf_(x) - t * x;
}

// Quality focal loss on PROBABILITIES (use_sigmoid=False: GFLv2, where the
// prediction is sigmoid(cls_feat) * quality; gfocal_loss.py:27-46 with
// F.binary_cross_entropy).  torch clamps the two logs at -100 in the forward
// and differentiates BCE as (p - t) / max(p (1 - p), 1e-12) in the backward
// (aten binary_cross_entropy / _backward), which is reproduced here.
//   negative entry : q = bce(p, 0) * p^2
//   positive entry : q = bce(p, s) * |s - p|^2
LD_HD float bce_prob(float p, float t, float* dbce) {
  float lp = fmaxf_(logf(p), -100.0f), l1p = fmaxf_(logf(1.0f - p), -100.0f);
  *dbce = (p - t) / fmaxf_((1.0f - p) * p, 1e-12f);
  return -(t * lp + (1.0f - t) * l1p);
}
LD_HD float qfl_prob_neg(float p, float* dq) {
  float db;
  float bce = bce_prob(p, 0.0f, &db);
  *dq = db * p * p + bce * 2.0f * p;
  return bce * p * p;
}
LD_HD float qfl_prob_pos(float p, float score, float* dq) {
  float db;
  float bce = bce_prob(p, score, &db);
  float d = score - p;
  *dq = db * d * d - 2.0f * d * bce;
  return bce * d * d;
}

// GIoU loss 1 - GIoU(pred, target) on aligned boxes (iou_loss.py:85-102,
// iou2d_calculator.py:117-177) and d(loss)/d(pred box), taking the same
// sub-gradients autograd takes through clamp(min=0) / max(., eps) / min / max
// (ties in min/max split 0.5/0.5 like torch.maximum's backward).
// Also returns the plain IoU (the QFL quality score, ld_head.py:204-207).
LD_HD float sel_gt(float a, float b) { return a > b ? 1.0f : (a == b ? 0.5f : 0.0f); }
LD_HD float sel_lt(float a, float b) { return a < b ? 1.0f : (a == b ? 0.5f : 0.0f); }

LD_HD float giou_loss_grad(const Box& p, const Box& t, float eps, float* iou_out,
                           float g[4]) {
  float pw = p.x2 - p.x1, ph = p.y2 - p.y1;
  float a1 = pw * ph;
  float a2 = (t.x2 - t.x1) * (t.y2 - t.y1);
  float iw_raw = fminf_(p.x2, t.x2) - fmaxf_(p.x1, t.x1);
  float ih_raw = fminf_(p.y2, t.y2) - fmaxf_(p.y1, t.y1);
  float iw = fmaxf_(iw_raw, 0.0f), ih = fmaxf_(ih_raw, 0.0f);
  float inter = iw * ih;
  float union_raw = a1 + a2 - inter;
  float uni = fmaxf_(union_raw, eps);
  float ew_raw = fmaxf_(p.x2, t.x2) - fminf_(p.x1, t.x1);
  float eh_raw = fmaxf_(p.y2, t.y2) - fminf_(p.y1, t.y1);
  float ew = fmaxf_(ew_raw, 0.0f), eh = fmaxf_(eh_raw, 0.0f);
  float earea_raw = ew * eh;
  float earea = fmaxf_(earea_raw, eps);
  float iou = inter / uni;
  float giou = iou - (earea - uni) / earea;
  *iou_out = iou;
  // giou = I/U - 1 + U/E
  float dg_dI = 1.0f / uni;
  float dg_dU = -inter / (uni * uni) + 1.0f / earea;
  float dg_dE = -uni / (earea * earea);
  float u_live = union_raw > eps ? 1.0f : 0.0f;
  float e_live = earea_raw > eps ? 1.0f : 0.0f;
  float gI = dg_dI - dg_dU * u_live;
  float gA1 = dg_dU * u_live;
  float gE = dg_dE * e_live;
  float g_iw = gI * ih * (iw_raw >= 0.0f ? 1.0f : 0.0f);
  float g_ih = gI * iw * (ih_raw >= 0.0f ? 1.0f : 0.0f);
  float g_ew = gE * eh * (ew_raw >= 0.0f ? 1.0f : 0.0f);
  float g_eh = gE * ew * (eh_raw >= 0.0f ? 1.0f : 0.0f);
  // d giou / d p, negated for the loss
  g[0] = -(gA1 * (-ph) - g_iw * sel_gt(p.x1, t.x1) - g_ew * sel_lt(p.x1, t.x1));
  g[1] = -(gA1 * (-pw) - g_ih * sel_gt(p.y1, t.y1) - g_eh * sel_lt(p.y1, t.y1));
  g[2] = -(gA1 * ph + g_iw * sel_lt(p.x2, t.x2) + g_ew * sel_gt(p.x2, t.x2));
  g[3] = -(gA1 * pw + g_ih * sel_lt(p.y2, t.y2) + g_eh * sel_gt(p.y2, t.y2));
  return 1.0f - giou;
}

// IoU loss -log(clamp(IoU, min=eps)) (linear: 1 - clamp(IoU, min=eps)) on
// aligned boxes (iou_loss.py:14-36) and d(loss)/d(pred box).  The IoU is
// bbox_overlaps' own (union = max(., 1e-6), iou2d_calculator.py:111-171);
// `eps` is the module's and only clamps: no gradient below it (clamp's backward
// passes at equality).  *iou_out is the unclamped IoU.
LD_HD float iou_loss_grad(const Box& p, const Box& t, float eps, bool linear,
                          float* iou_out, float g[4]) {
  float pw = p.x2 - p.x1, ph = p.y2 - p.y1;
  float a1 = pw * ph;
  float a2 = (t.x2 - t.x1) * (t.y2 - t.y1);
  float iw_raw = fminf_(p.x2, t.x2) - fmaxf_(p.x1, t.x1);
  float ih_raw = fminf_(p.y2, t.y2) - fmaxf_(p.y1, t.y1);
  float iw = fmaxf_(iw_raw, 0.0f), ih = fmaxf_(ih_raw, 0.0f);
  float inter = iw * ih;
  float union_raw = a1 + a2 - inter;
  float uni = fmaxf_(union_raw, 1e-6f);
  float iou = inter / uni;
  *iou_out = iou;
  float ic = fmaxf_(iou, eps);
  // d loss / d iou
  float k = iou >= eps ? (linear ? -1.0f : -1.0f / ic) : 0.0f;
  float dU = -inter / (uni * uni) * sel_gt(union_raw, 1e-6f);
  float gI = k * (1.0f / uni - dU);
  float gA1 = k * dU;
  float g_iw = gI * ih * (iw_raw >= 0.0f ? 1.0f : 0.0f);
  float g_ih = gI * iw * (ih_raw >= 0.0f ? 1.0f : 0.0f);
  g[0] = gA1 * (-ph) - g_iw * sel_gt(p.x1, t.x1);
  g[1] = gA1 * (-pw) - g_ih * sel_gt(p.y1, t.y1);
  g[2] = gA1 * ph + g_iw * sel_lt(p.x2, t.x2);
  g[3] = gA1 * pw + g_ih * sel_lt(p.y2, t.y2);
  return linear ? 1.0f - ic : -logf(ic);
}

// DIoU loss 1 - (IoU - rho^2 / c^2) and CIoU loss 1 - (IoU - (rho^2 / c^2 +
// v^2 / (1 - IoU + v))) on aligned boxes (iou_loss.py:107-157, :162-219) and
// d(loss)/d(pred box).  The conventions are the reference's own and differ from
// bbox_overlaps': union = ap + ag - overlap + eps and c^2 = cw^2 + ch^2 + eps
// are ADDITIVE; CIoU's heights are (y2 - y1) + eps; v = 4/pi^2 (atan(w2/h2) -
// atan(w1/h1))^2 carries a gradient, and so does the IoU inside v's
// denominator (no no_grad there).  Sub-gradients as in giou_loss_grad.
// *iou_out is bbox_overlaps' IoU (the QFL quality score), not the additive one.
LD_HD float dciou_loss_grad_(const Box& p, const Box& t, float eps, bool ciou,
                             float* iou_out, float g[4]) {
  float pw = p.x2 - p.x1, ph = p.y2 - p.y1;
  float tw = t.x2 - t.x1, th = t.y2 - t.y1;
  float iw_raw = fminf_(p.x2, t.x2) - fmaxf_(p.x1, t.x1);
  float ih_raw = fminf_(p.y2, t.y2) - fmaxf_(p.y1, t.y1);
  float iw = fmaxf_(iw_raw, 0.0f), ih = fmaxf_(ih_raw, 0.0f);
  float inter = iw * ih;
  float union_raw = pw * ph + tw * th - inter;
  float uni = union_raw + eps;
  float iou = inter / uni;
  *iou_out = inter / fmaxf_(union_raw, 1e-6f);
  float cw_raw = fmaxf_(p.x2, t.x2) - fminf_(p.x1, t.x1);
  float ch_raw = fmaxf_(p.y2, t.y2) - fminf_(p.y1, t.y1);
  float cw = fmaxf_(cw_raw, 0.0f), ch = fmaxf_(ch_raw, 0.0f);
  float c2 = cw * cw + ch * ch + eps;
  float lx = (t.x1 + t.x2) - (p.x1 + p.x2);
  float ly = (t.y1 + t.y2) - (p.y1 + p.y2);
  float rho2 = (lx * lx) / 4.0f + (ly * ly) / 4.0f;
  float pen = rho2 / c2;
  // k_iou = d loss / d iou; g_w, g_h = d loss / d (pred width, pred height)
  float k_iou = -1.0f, g_w = 0.0f, g_h = 0.0f;
  if (ciou) {
    const float factor = (float)(4.0 / (M_PI * M_PI));
    float h1 = ph + eps, h2 = th + eps;
    float r1 = pw / h1;
    float d = atanf(tw / h2) - atanf(r1);
    float v = factor * (d * d);
    float den = 1.0f - iou + v;
    // den == 0 only for a perfect box (iou == 1 once fp32 drops the additive eps
    // of the union, and v == 0): q = v^2 / den and its derivatives are 0 there,
    // as in exact arithmetic.  The reference's fp32 evaluates 0 / 0 = NaN at such
    // a box; float64 gives 0 (tests/test_gpu_loss_edges.py, box_ties_ciou).
    const bool live = den > 0.0f;
    float vd2 = live ? (v * v) / (den * den) : 0.0f;
    pen = pen + (live ? (v * v) / den : 0.0f);
    k_iou = -1.0f + vd2;
    // d q / d v * d v / d r1, q = v^2 / den
    float gr1 = ((live ? 2.0f * v / den : 0.0f) - vd2) *
                (-(factor * 2.0f * d) / (1.0f + r1 * r1));
    g_w = gr1 / h1;
    g_h = -gr1 * r1 / h1;
  }
  float dU = -inter / (uni * uni);
  float gI = k_iou * (1.0f / uni - dU);
  float gA1 = k_iou * dU;
  float g_iw = gI * ih * (iw_raw >= 0.0f ? 1.0f : 0.0f);
  float g_ih = gI * iw * (ih_raw >= 0.0f ? 1.0f : 0.0f);
  float gc = -rho2 / (c2 * c2);
  float g_cw = gc * 2.0f * cw * (cw_raw >= 0.0f ? 1.0f : 0.0f);
  float g_ch = gc * 2.0f * ch * (ch_raw >= 0.0f ? 1.0f : 0.0f);
  float g_lx = -lx / (2.0f * c2), g_ly = -ly / (2.0f * c2);
  g[0] = gA1 * (-ph) - g_iw * sel_gt(p.x1, t.x1) + g_lx - g_cw * sel_lt(p.x1, t.x1) - g_w;
  g[1] = gA1 * (-pw) - g_ih * sel_gt(p.y1, t.y1) + g_ly - g_ch * sel_lt(p.y1, t.y1) - g_h;
  g[2] = gA1 * ph + g_iw * sel_lt(p.x2, t.x2) + g_lx + g_cw * sel_gt(p.x2, t.x2) + g_w;
  g[3] = gA1 * pw + g_ih * sel_lt(p.y2, t.y2) + g_ly + g_ch * sel_gt(p.y2, t.y2) + g_h;
  return 1.0f - (iou - pen);
}
LD_HD float diou_loss_grad(const Box& p, const Box& t, float eps, float* iou_out,
                           float g[4]) {
  return dciou_loss_grad_(p, t, eps, false, iou_out, g);
}
LD_HD float ciou_loss_grad(const Box& p, const Box& t, float eps, float* iou_out,
                           float g[4]) {
  return dciou_loss_grad_(p, t, eps, true, iou_out, g);
}

// One 17-bin side of the LD regression distribution.
// Inputs: student logits s[17], teacher logits t[17].
//   kl    = T^2/K * sum_k pt_k (log pt_k - log ps_k),  p = softmax(./T)
//           (kd_loss.py:27-36; K = 17 because of .mean(1))
//   dkl_k = T/K * (ps_k - pt_k)
// Outputs are accumulated by the caller with its own weights.
struct SideKL {
  float kl;
  float lse_s, lse_t;  // log-sum-exp of s/T and t/T (max-shifted form folded in)
};

// a * b - c * d for the KL gradient direction ps - pt of kl_rows_inplace:
// fma(a, b, -(c * d)), one rounding fewer than two products -- except where
// (a, b) == (c, d).  There the difference is exactly 0 and the fma would return
// the rounding residual of c * d (about 1e-8 of p): a student row that equals its
// teacher's gets exactly zero, as kl_rows gives it
// (tests/test_gpu_loss_edges.py, student_is_teacher).  Every other input keeps
// the fma's bits.
LD_HD float diff_of_products_(float a, float b, float c, float d) {
  return (a == c && b == d) ? 0.0f : fmaf(a, b, -(c * d));
}

template <int K>
LD_HD float kl_rows(const float* s, const float* t, float invT, float T,
                    float* ps_minus_pt /* [K] out: ps_k - pt_k */) {
  float ms = s[0], mt = t[0];
#pragma unroll
  for (int k = 1; k < K; ++k) {
    ms = fmaxf_(ms, s[k]);
    mt = fmaxf_(mt, t[k]);
  }
  float es[K], et[K];
  float zs = 0.0f, zt = 0.0f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    es[k] = expf((s[k] - ms) * invT);
    et[k] = expf((t[k] - mt) * invT);
    zs += es[k];
    zt += et[k];
  }
  float rzs = 1.0f / zs, rzt = 1.0f / zt;
  float lzs = logf(zs), lzt = logf(zt);
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float pt = et[k] * rzt;
    float ps = es[k] * rzs;
    // log pt - log ps
    float d = ((t[k] - mt) * invT - lzt) - ((s[k] - ms) * invT - lzs);
    acc += pt * d;
    ps_minus_pt[k] = ps - pt;
  }
  return acc * (T * T) / (float)K;
}

// Register-lean form of kl_rows for the dense sweep (round 3): the same KL
// (kd_loss.py:27-36) with the row statistics folded so that nothing but the two
// logit rows stays live --
//   kl = T^2/K * [ 1/(T z_t) * sum_k e_t,k ((t_k - m_t) - (s_k - m_s)) + log z_s - log z_t ]
// (sum_k pt_k = 1 moves the two log-sum-exp terms out of the sum).  On return
// s[k] = ps_k - pt_k (the gradient direction) and t[k] = e_t,k; 34 live values
// instead of kl_rows' 85.  FAST: exp / reciprocal through the hardware
// v_exp_f32 / v_rcp_f32 (1 ulp) instead of the correctly rounded library forms.
#if defined(__HIP_DEVICE_COMPILE__)
LD_HD float fast_exp2_(float x) { return __builtin_amdgcn_exp2f(x); }
LD_HD float fast_rcp_(float x) { return __builtin_amdgcn_rcpf(x); }
#else
LD_HD float fast_exp2_(float x) { return exp2f(x); }
LD_HD float fast_rcp_(float x) { return 1.0f / x; }
#endif

template <int K, bool FAST>
LD_HD float kl_rows_inplace(float* s, float* t, float invT, float T) {
  float ms = s[0], mt = t[0];
#pragma unroll
  for (int k = 1; k < K; ++k) {
    ms = fmaxf_(ms, s[k]);
    mt = fmaxf_(mt, t[k]);
  }
  const float c = FAST ? invT * 1.44269504088896341f : invT;
  float zs = 0.0f, zt = 0.0f, acc = 0.0f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float ds = s[k] - ms, dt = t[k] - mt;
    const float es = FAST ? fast_exp2_(ds * c) : expf(ds * c);
    const float et = FAST ? fast_exp2_(dt * c) : expf(dt * c);
    zs += es;
    zt += et;
    acc = fmaf(et, dt - ds, acc);
    s[k] = es;
    t[k] = et;
  }
  const float rzs = FAST ? fast_rcp_(zs) : 1.0f / zs;
  const float rzt = FAST ? fast_rcp_(zt) : 1.0f / zt;
  const float kl = (acc * rzt * invT + (logf(zs) - logf(zt))) * ((T * T) / (float)K);
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = diff_of_products_(s[k], rzs, t[k], rzt);
  return kl;
}

// Softmax over one 17-bin side + its expectation (Integral, gfl_head.py:32-44).
template <int K>
LD_HD float softmax_expect(const float* s, float* p /* [K] out */) {
  float m = s[0];
#pragma unroll
  for (int k = 1; k < K; ++k) m = fmaxf_(m, s[k]);
  float z = 0.0f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    p[k] = expf(s[k] - m);
    z += p[k];
  }
  float rz = 1.0f / z, e = 0.0f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    p[k] *= rz;
    e += p[k] * (float)k;
  }
  return e;
}

// Distribution focal loss of one side given its softmax p and log-sum-exp
// pieces (gfocal_loss.py:53-74): y in [0, reg_max - 0.1].
//   loss = CE(s, yl) * (yl + 1 - y) + CE(s, yl + 1) * (y - yl)
//   dloss/ds_k = p_k - wl [k == yl] - wr [k == yl + 1]      (wl + wr = 1)
template <int K>
LD_HD float dfl_side(const float* s, const float* p, float y, float* wl_out,
                     float* wr_out, int* yl_out) {
  int yl = (int)y;  // label.long(): truncation, y >= 0
  float wl = (float)(yl + 1) - y;
  float wr = y - (float)yl;
  // log softmax at yl and yl+1:  s_k - m - log z  ==  log p_k
  float m = s[0];
#pragma unroll
  for (int k = 1; k < K; ++k) m = fmaxf_(m, s[k]);
  float z = 0.0f;
#pragma unroll
  for (int k = 0; k < K; ++k) z += expf(s[k] - m);
  float lz = logf(z);
  float ll = 0.0f, lr = 0.0f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float lp = s[k] - m - lz;
    ll = (k == yl) ? lp : ll;
    lr = (k == yl + 1) ? lp : lr;
  }
  *wl_out = wl;
  *wr_out = wr;
  *yl_out = yl;
  (void)p;
  return -ll * wl - lr * wr;
}

// softmax_expect + dfl_side fused and IN PLACE (the same op sequence, so the same
// bits): on return s[k] = softmax(s)_k, *e_out = the Integral expectation, and
// the DFL value of target y is returned.  34 -> 17 live values for the dense
// sweep's rare positive anchors.
template <int K>
LD_HD float softmax_dfl_inplace(float* s, float y, float* e_out, float* wl_out,
                                float* wr_out, int* yl_out) {
  const int yl = (int)y;
  const float wl = (float)(yl + 1) - y, wr = y - (float)yl;
  float m = s[0];
#pragma unroll
  for (int k = 1; k < K; ++k) m = fmaxf_(m, s[k]);
  float z = 0.0f, sl = 0.0f, sr = 0.0f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    sl = (k == yl) ? s[k] : sl;
    sr = (k == yl + 1) ? s[k] : sr;
    s[k] = expf(s[k] - m);
    z += s[k];
  }
  const float lz = logf(z), rz = 1.0f / z;
  float e = 0.0f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    s[k] *= rz;
    e += s[k] * (float)k;
  }
  // yl + 1 <= K - 1 (y <= reg_max - 0.1); a bin outside [0, K) contributes
  // log p = 0 exactly as dfl_side's unmatched select does
  const float ll = (yl >= 0 && yl < K) ? sl - m - lz : 0.0f;
  const float lr = (yl + 1 >= 0 && yl + 1 < K) ? sr - m - lz : 0.0f;
  *e_out = e;
  *wl_out = wl;
  *wr_out = wr;
  *yl_out = yl;
  return -ll * wl - lr * wr;
}

// bbox2distance clamp (core/bbox/transforms.py:171-180), max_dis = reg_max,
// eps = 0.1
LD_HD float clamp_dist(float d, float reg_max) {
  return fminf_(fmaxf_(d, 0.0f), reg_max - 0.1f);
}

// ---- DeltaXYWHBBoxCoder (core/bbox/coder/delta_xywh_bbox_coder.py) ----------
// bbox2delta, :87-130: deltas of `gt` about `roi`, in the reference's op order.
LD_HD void bbox2delta(const Box& roi, const Box& gt, const float* means,
                      const float* stds, float* d /* [4] out */) {
  const float px = (roi.x1 + roi.x2) * 0.5f, py = (roi.y1 + roi.y2) * 0.5f;
  const float pw = roi.x2 - roi.x1, ph = roi.y2 - roi.y1;
  const float gx = (gt.x1 + gt.x2) * 0.5f, gy = (gt.y1 + gt.y2) * 0.5f;
  const float gw = gt.x2 - gt.x1, gh = gt.y2 - gt.y1;
  d[0] = ((gx - px) / pw - means[0]) / stds[0];
  d[1] = ((gy - py) / ph - means[1]) / stds[1];
  d[2] = (logf(gw / pw) - means[2]) / stds[2];
  d[3] = (logf(gh / ph) - means[3]) / stds[3];
}

// delta2bbox, :133-220 without the max_shape clip: denormalise, clamp dw / dh at
// +-max_ratio = |log(wh_ratio_clip)|, shift the centre, scale the size.  `jac`
// (nullable, [4]): d centre_x / d d0, d centre_y / d d1, d half_w / d d2,
// d half_h / d d3 -- the last two are 0 where the clamp cut (torch.clamp passes
// the gradient on the closed interval [-max_ratio, max_ratio]).
LD_HD Box delta2bbox(const Box& roi, const float* d, const float* means,
                     const float* stds, float max_ratio, float* jac) {
  const float dx = d[0] * stds[0] + means[0], dy = d[1] * stds[1] + means[1];
  const float dw0 = d[2] * stds[2] + means[2], dh0 = d[3] * stds[3] + means[3];
  const float dw = fminf_(fmaxf_(dw0, -max_ratio), max_ratio);
  const float dh = fminf_(fmaxf_(dh0, -max_ratio), max_ratio);
  const float px = (roi.x1 + roi.x2) * 0.5f, py = (roi.y1 + roi.y2) * 0.5f;
  const float pw = roi.x2 - roi.x1, ph = roi.y2 - roi.y1;
  const float gw = pw * expf(dw), gh = ph * expf(dh);
  const float gx = px + pw * dx, gy = py + ph * dy;
  if (jac) {
    jac[0] = pw * stds[0];
    jac[1] = ph * stds[1];
    jac[2] = (dw0 < -max_ratio || dw0 > max_ratio) ? 0.0f : 0.5f * gw * stds[2];
    jac[3] = (dh0 < -max_ratio || dh0 > max_ratio) ? 0.0f : 0.5f * gh * stds[3];
  }
  return Box{gx - gw * 0.5f, gy - gh * 0.5f, gx + gw * 0.5f, gy + gh * 0.5f};
}

// the clip of :222-235: x to [0, w], y to [0, h]
LD_HD Box clip_box(const Box& b, float h, float w) {
  return Box{fminf_(fmaxf_(b.x1, 0.0f), w), fminf_(fmaxf_(b.y1, 0.0f), h),
             fminf_(fmaxf_(b.x2, 0.0f), w), fminf_(fmaxf_(b.y2, 0.0f), h)};
}

// d loss / d delta[k] from d loss / d (x1, y1, x2, y2) of the decoded box
LD_HD void delta2bbox_grad(const float* g /* [4] */, const float* jac, float* gd) {
  gd[0] = (g[0] + g[2]) * jac[0];
  gd[1] = (g[1] + g[3]) * jac[1];
  gd[2] = (g[2] - g[0]) * jac[2];
  gd[3] = (g[3] - g[1]) * jac[3];
}

// l1_loss / smooth_l1_loss element, losses/smooth_l1_loss.py:9-56; d = pred -
// target.  Returns the loss, writes its derivative (sign(0) = 0 as torch.abs).
LD_HD float l1_elem(float d, float* dl) {
  *dl = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
  return fabsf(d);
}
LD_HD float smooth_l1_elem(float d, float beta, float* dl) {
  const float a = fabsf(d);
  if (a < beta) {
    *dl = d / beta;
    return 0.5f * a * a / beta;
  }
  *dl = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
  return a - 0.5f * beta;
}

}  // namespace ld
