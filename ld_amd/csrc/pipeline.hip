// Device input pipeline for gfx950: what the
// reference's train_pipeline does per image on CPU workers
//   Resize(img_scale=(1333, 800), keep_ratio=True) -> RandomFlip ->
//   Normalize(mean, std, to_rgb=True) -> Pad(size_divisor=32) -> collate
//   (configs/ld/ld_r18_gflv1_r101_fpn_coco_1x.py:66-77,
//    mmdet/datasets/pipelines/transforms.py:203-233,416-450,524-580)
// as ONE launch for a whole batch: decoded uint8 HWC images (BGR, as
// cv2.imread / LoadImageFromFile deliver them) already on the device ->
// the padded fp32 NCHW batch tensor the detector consumes.  At 2 workers per
// GPU (data.workers_per_gpu=2) the CPU pipeline cannot feed an MI355X at the
// measured step rate; this kernel is HBM-bound (3 bytes in, 12 bytes out per
// pixel: 2 x 800 x 1344 x 15 B = 32 MB -> a few microseconds).
//
// Arithmetic restated from the published behaviour of the libraries the
// reference calls (absent from the checkout: mmcv.imrescale -> cv2.resize
// INTER_LINEAR on 8-bit data, mmcv.imflip, mmcv.imnormalize):
//   * bilinear with pixel-centre alignment, source index clamped at the
//     borders, 11-bit fixed-point coefficients and a rounded 8-bit result
//     (cv2's INTER_RESIZE_COEF_BITS = 11 path; the result is uint8 BEFORE the
//     normalisation, as in the reference);
//   * horizontal flip of the resized image; BGR -> RGB; (v - mean) * (1 / std)
//     in fp32; zeros in the padding.
// Parity status: UNPINNED against cv2 itself (checked bit-exactly against the
// numpy restatement in oracle/pipeline_oracle.py).
#include <hip/hip_runtime.h>

#include "ld_launch.h"

#include "../../include/ld_hip.h"

namespace {

constexpr int kCoefBits = 11, kCoefOne = 1 << kCoefBits;

__device__ __forceinline__ void lin_coef(int d, double scale, int ssize, int& s0,
                                         int& s1, int& a0, int& a1) {
  // cv2 resize (linear): fx = (d + 0.5) * scale - 0.5
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) {
    f = 0.0f;
    s = 0;
  }
  if (s >= ssize - 1) {
    f = 0.0f;
    s = ssize - 1;
  }
  s0 = s;
  s1 = min(s + 1, ssize - 1);
  // saturate_cast<short>(x * 2048): round to nearest even like cvRound
  a0 = (int)rintf((1.0f - f) * (float)kCoefOne);
  a1 = (int)rintf(f * (float)kCoefOne);
}

__global__ __launch_bounds__(256) void preprocess_kernel(
    const ld_image_t* __restrict__ imgs, int Hpad, int Wpad, float mean0, float mean1,
    float mean2, float inv0, float inv1, float inv2, int to_rgb,
    float* __restrict__ out) {
  const int n = blockIdx.z;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= Wpad || y >= Hpad) return;
  const ld_image_t im = imgs[n];
  const size_t plane = (size_t)Hpad * Wpad;
  float* o = out + (size_t)n * 3 * plane + (size_t)y * Wpad + x;
  if (y >= im.new_h || x >= im.new_w) {  // Pad(size_divisor) / collate: zeros
    o[0] = 0.0f;
    o[plane] = 0.0f;
    o[2 * plane] = 0.0f;
    return;
  }
  const int xr = im.flip ? im.new_w - 1 - x : x;  // flip AFTER the resize
  int sx0, sx1, ax0, ax1, sy0, sy1, ay0, ay1;
  lin_coef(xr, (double)im.src_w / (double)im.new_w, im.src_w, sx0, sx1, ax0, ax1);
  lin_coef(y, (double)im.src_h / (double)im.new_h, im.src_h, sy0, sy1, ay0, ay1);
  const unsigned char* r0 = im.data + ((size_t)sy0 * im.src_w) * 3;
  const unsigned char* r1 = im.data + ((size_t)sy1 * im.src_w) * 3;
  const float mean[3] = {mean0, mean1, mean2}, inv[3] = {inv0, inv1, inv2};
#pragma unroll
  for (int c = 0; c < 3; ++c) {  // c = output channel
    const int cs = to_rgb ? 2 - c : c;  // source (BGR) channel
    const int h0 = r0[sx0 * 3 + cs] * ax0 + r0[sx1 * 3 + cs] * ax1;
    const int h1 = r1[sx0 * 3 + cs] * ax0 + r1[sx1 * 3 + cs] * ax1;
    // FixedPtCast<int, uchar, 2 * 11>: (v + (1 << 21)) >> 22
    int v = (h0 * ay0 + h1 * ay1 + (1 << (2 * kCoefBits - 1))) >> (2 * kCoefBits);
    v = min(max(v, 0), 255);
    o[(size_t)c * plane] = ((float)v - mean[c]) * inv[c];
  }
}

// The train-time augmentations in the same launch (ld_hip.h, ld_image_aug_t):
// every output pixel walks back through crop -> resize -> window -> canvas to
// at most four source bytes per channel; nothing intermediate is stored.
// Same 64 x 4 mapping: a wavefront writes 64 consecutive floats of one row per
// plane, and reads a contiguous (scale x 192 byte) run of one source row.
__global__ __launch_bounds__(256) void preprocess_aug_kernel(
    const ld_image_aug_t* __restrict__ imgs, int Hpad, int Wpad, float mean0,
    float mean1, float mean2, float inv0, float inv1, float inv2, float pad0,
    float pad1, float pad2, int to_rgb, float* __restrict__ out) {
  const int n = blockIdx.z;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= Wpad || y >= Hpad) return;
  const ld_image_aug_t im = imgs[n];
  const size_t plane = (size_t)Hpad * Wpad;
  float* o = out + (size_t)n * 3 * plane + (size_t)y * Wpad + x;
  if (y >= im.out_h || x >= im.out_w) {  // Pad(size / size_divisor, pad_val)
    o[0] = pad0;
    o[plane] = pad1;
    o[2 * plane] = pad2;
    return;
  }
  // flip within the crop, then the crop offset: resized coordinates
  const int xr = (im.flip ? im.out_w - 1 - x : x) + im.crop_x;
  const int yr = y + im.crop_y;
  int sx0, sx1, ax0, ax1, sy0, sy1, ay0, ay1;  // window coordinates
  lin_coef(xr, (double)im.win_w / (double)im.new_w, im.win_w, sx0, sx1, ax0, ax1);
  lin_coef(yr, (double)im.win_h / (double)im.new_h, im.win_h, sy0, sy1, ay0, ay1);
  // window -> canvas -> image; a tap outside the image reads the fill
  const int ix0 = im.win_x + sx0 - im.img_left, ix1 = im.win_x + sx1 - im.img_left;
  const int iy0 = im.win_y + sy0 - im.img_top, iy1 = im.win_y + sy1 - im.img_top;
  const bool inx0 = (unsigned)ix0 < (unsigned)im.src_w;
  const bool inx1 = (unsigned)ix1 < (unsigned)im.src_w;
  const bool iny0 = (unsigned)iy0 < (unsigned)im.src_h;
  const bool iny1 = (unsigned)iy1 < (unsigned)im.src_h;
  // rows that are not read keep a valid address (row 0)
  const unsigned char* r0 = im.data + ((size_t)(iny0 ? iy0 : 0) * im.src_w) * 3;
  const unsigned char* r1 = im.data + ((size_t)(iny1 ? iy1 : 0) * im.src_w) * 3;
  const float mean[3] = {mean0, mean1, mean2}, inv[3] = {inv0, inv1, inv2};
#pragma unroll
  for (int c = 0; c < 3; ++c) {  // c = output channel
    const int cs = to_rgb ? 2 - c : c;  // source (BGR) channel
    const int f = im.fill[cs];
    const int p00 = (iny0 && inx0) ? r0[ix0 * 3 + cs] : f;
    const int p01 = (iny0 && inx1) ? r0[ix1 * 3 + cs] : f;
    const int p10 = (iny1 && inx0) ? r1[ix0 * 3 + cs] : f;
    const int p11 = (iny1 && inx1) ? r1[ix1 * 3 + cs] : f;
    const int h0 = p00 * ax0 + p01 * ax1;
    const int h1 = p10 * ax0 + p11 * ax1;
    int v = (h0 * ay0 + h1 * ay1 + (1 << (2 * kCoefBits - 1))) >> (2 * kCoefBits);
    v = min(max(v, 0), 255);
    o[(size_t)c * plane] = ((float)v - mean[c]) * inv[c];
  }
}

// ---- float-image mode (ld_hip.h, ld_image_photo_t) ---------------------------
// LoadImageFromFile(to_float32=True) -> PhotoMetricDistortion in front of the
// steps above.  The distortion is pointwise, so it runs on each of the four
// taps of an output pixel; nothing is stored.  The two colour conversions are
// OpenCV's published float formulas (H in [0, 360), S = diff / (|V| +
// FLT_EPSILON), V the maximum; the branch order for ties and the sector table
// are stated in ld_hip.h), the resize is cv2's float INTER_LINEAR (coefficients
// 1 - f and f, no rounding to 8 bits).  Only correctly rounded fp32 + - * /,
// compares, floors and int conversions (hipcc's default division is the
// correctly rounded one; this file is built with -ffp-contract=off).
// Parity status: UNPINNED against cv2 itself for both conversions and the
// float resize; checked bit for bit against tests/_photometric_oracle.py.
constexpr float kFltEps = 1.1920928955078125e-07f;

__device__ __forceinline__ void lin_coef_f(int d, double scale, int ssize, int& s0,
                                           int& s1, float& a0, float& a1) {
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) {
    f = 0.0f;
    s = 0;
  }
  if (s >= ssize - 1) {
    f = 0.0f;
    s = ssize - 1;
  }
  s0 = s;
  s1 = min(s + 1, ssize - 1);
  a0 = 1.0f - f;
  a1 = f;
}

__device__ __forceinline__ float sel3(float x0, float x1, float x2, int k) {
  return k == 0 ? x0 : (k == 1 ? x1 : x2);
}

// the chain of one pixel, in place: x0, x1, x2 = B, G, R
__device__ __forceinline__ void photo_chain(const ld_image_photo_t& im, float& x0,
                                            float& x1, float& x2) {
  if (im.do_brightness) {
    x0 += im.delta;
    x1 += im.delta;
    x2 += im.delta;
  }
  if (im.do_contrast && im.contrast_mode == 1) {
    x0 *= im.alpha;
    x1 *= im.alpha;
    x2 *= im.alpha;
  }
  if (im.do_hsv) {
    const float b = x0, g = x1, r = x2;
    float v = fmaxf(fmaxf(r, g), b);
    const float vmin = fminf(fminf(r, g), b);
    const float diff = v - vmin;
    float s = diff / (fabsf(v) + kFltEps);
    const float k = 60.0f / (diff + kFltEps);
    float h;
    if (v == r)
      h = (g - b) * k;
    else if (v == g)
      h = (b - r) * k + 120.0f;
    else
      h = (r - g) * k + 240.0f;
    if (h < 0.0f) h += 360.0f;
    if (im.do_saturation) s *= im.saturation;
    if (im.do_hue) {
      h += im.hue;
      if (h > 360.0f) h -= 360.0f;
      if (h < 0.0f) h += 360.0f;
    }
    if (s == 0.0f) {
      x0 = x1 = x2 = v;
    } else {
      h *= 6.0f / 360.0f;  // one fp32 constant, as OpenCV's hscale
      if (h < 0.0f)
        h += 6.0f;
      else if (h >= 6.0f)
        h -= 6.0f;
      int sector = (int)floorf(h);
      h -= (float)sector;
      if ((unsigned)sector >= 6u) {
        sector = 0;
        h = 0.0f;
      }
      const float t0 = v;
      const float t1 = v * (1.0f - s);
      const float t2 = v * (1.0f - s * h);
      const float t3 = v * (1.0f - s * (1.0f - h));
      switch (sector) {  // (B, G, R) = tab[sector_data[sector][0 .. 2]]
        case 0: x0 = t1; x1 = t3; x2 = t0; break;
        case 1: x0 = t1; x1 = t0; x2 = t2; break;
        case 2: x0 = t3; x1 = t0; x2 = t1; break;
        case 3: x0 = t0; x1 = t2; x2 = t1; break;
        case 4: x0 = t0; x1 = t1; x2 = t3; break;
        default: x0 = t2; x1 = t1; x2 = t0; break;
      }
    }
  }
  if (im.do_contrast && im.contrast_mode == 0) {
    x0 *= im.alpha;
    x1 *= im.alpha;
    x2 *= im.alpha;
  }
  const float y0 = sel3(x0, x1, x2, im.perm[0]);
  const float y1 = sel3(x0, x1, x2, im.perm[1]);
  const float y2 = sel3(x0, x1, x2, im.perm[2]);
  x0 = y0;
  x1 = y1;
  x2 = y2;
}

// one tap: the distorted image pixel, or the canvas fill as it is
__device__ __forceinline__ void photo_tap(const ld_image_photo_t& im,
                                          const unsigned char* row, int ix, bool in,
                                          float (&p)[3]) {
  if (in) {
    const unsigned char* s = row + (size_t)ix * 3;
    p[0] = (float)s[0];
    p[1] = (float)s[1];
    p[2] = (float)s[2];
    photo_chain(im, p[0], p[1], p[2]);
  } else {
    p[0] = im.fill[0];
    p[1] = im.fill[1];
    p[2] = im.fill[2];
  }
}

// Same 64 x 4 mapping and launch shape as the two kernels above; the
// photometric scalars are uniform per image (blockIdx.z), so every branch of
// the chain but the pixel's own (tie order, sector) is uniform per block.
__global__ __launch_bounds__(256) void preprocess_photo_kernel(
    const ld_image_photo_t* __restrict__ imgs, int Hpad, int Wpad, float mean0,
    float mean1, float mean2, float inv0, float inv1, float inv2, float pad0,
    float pad1, float pad2, int to_rgb, float* __restrict__ out) {
  const int n = blockIdx.z;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= Wpad || y >= Hpad) return;
  const ld_image_photo_t im = imgs[n];
  const size_t plane = (size_t)Hpad * Wpad;
  float* o = out + (size_t)n * 3 * plane + (size_t)y * Wpad + x;
  if (y >= im.out_h || x >= im.out_w) {  // Pad(size / size_divisor, pad_val)
    o[0] = pad0;
    o[plane] = pad1;
    o[2 * plane] = pad2;
    return;
  }
  const int xr = (im.flip ? im.out_w - 1 - x : x) + im.crop_x;
  const int yr = y + im.crop_y;
  int sx0, sx1, sy0, sy1;  // window coordinates
  float ax0, ax1, ay0, ay1;
  lin_coef_f(xr, (double)im.win_w / (double)im.new_w, im.win_w, sx0, sx1, ax0, ax1);
  lin_coef_f(yr, (double)im.win_h / (double)im.new_h, im.win_h, sy0, sy1, ay0, ay1);
  // window -> canvas -> image; a tap outside the image reads the fill
  const int ix0 = im.win_x + sx0 - im.img_left, ix1 = im.win_x + sx1 - im.img_left;
  const int iy0 = im.win_y + sy0 - im.img_top, iy1 = im.win_y + sy1 - im.img_top;
  const bool inx0 = (unsigned)ix0 < (unsigned)im.src_w;
  const bool inx1 = (unsigned)ix1 < (unsigned)im.src_w;
  const bool iny0 = (unsigned)iy0 < (unsigned)im.src_h;
  const bool iny1 = (unsigned)iy1 < (unsigned)im.src_h;
  // rows that are not read keep a valid address (row 0)
  const unsigned char* r0 = im.data + ((size_t)(iny0 ? iy0 : 0) * im.src_w) * 3;
  const unsigned char* r1 = im.data + ((size_t)(iny1 ? iy1 : 0) * im.src_w) * 3;
  float p00[3], p01[3], p10[3], p11[3];
  photo_tap(im, r0, ix0, iny0 && inx0, p00);
  photo_tap(im, r0, ix1, iny0 && inx1, p01);
  photo_tap(im, r1, ix0, iny1 && inx0, p10);
  photo_tap(im, r1, ix1, iny1 && inx1, p11);
  const float mean[3] = {mean0, mean1, mean2}, inv[3] = {inv0, inv1, inv2};
#pragma unroll
  for (int c = 0; c < 3; ++c) {  // c = output channel
    const int cs = to_rgb ? 2 - c : c;  // source (BGR) channel
    const float h0 = p00[cs] * ax0 + p01[cs] * ax1;  // horizontal pass
    const float h1 = p10[cs] * ax0 + p11[cs] * ax1;
    const float v = h0 * ay0 + h1 * ay1;  // vertical pass
    o[(size_t)c * plane] = (v - mean[c]) * inv[c];
  }
}

}  // namespace

extern "C" int ld_preprocess_batch_photo(const ld_image_photo_t* imgs, int N, int Hpad,
                                         int Wpad, const float* mean,
                                         const float* std_inv, const float* pad_val,
                                         int to_rgb, float* out, ld_stream_t stream) {
  if (!imgs || !mean || !std_inv || !pad_val || !out || N < 1 || Hpad < 1 || Wpad < 1)
    return LD_EINVAL;
  LD_LAUNCH(preprocess_photo_kernel, dim3((Wpad + 63) / 64, (Hpad + 3) / 4, N),
                     dim3(256), 0, (hipStream_t)stream, imgs, Hpad, Wpad, mean[0],
                     mean[1], mean[2], std_inv[0], std_inv[1], std_inv[2], pad_val[0],
                     pad_val[1], pad_val[2], to_rgb, out);
  return (int)hipGetLastError();
}

extern "C" int ld_preprocess_batch_aug(const ld_image_aug_t* imgs, int N, int Hpad,
                                       int Wpad, const float* mean,
                                       const float* std_inv, const float* pad_val,
                                       int to_rgb, float* out, ld_stream_t stream) {
  if (!imgs || !mean || !std_inv || !pad_val || !out || N < 1 || Hpad < 1 || Wpad < 1)
    return LD_EINVAL;
  LD_LAUNCH(preprocess_aug_kernel, dim3((Wpad + 63) / 64, (Hpad + 3) / 4, N),
                     dim3(256), 0, (hipStream_t)stream, imgs, Hpad, Wpad, mean[0],
                     mean[1], mean[2], std_inv[0], std_inv[1], std_inv[2], pad_val[0],
                     pad_val[1], pad_val[2], to_rgb, out);
  return (int)hipGetLastError();
}

extern "C" int ld_preprocess_batch(const ld_image_t* imgs, int N, int Hpad, int Wpad,
                                   const float* mean, const float* std_inv, int to_rgb,
                                   float* out, ld_stream_t stream) {
  if (!imgs || !mean || !std_inv || !out || N < 1 || Hpad < 1 || Wpad < 1)
    return LD_EINVAL;
  LD_LAUNCH(preprocess_kernel, dim3((Wpad + 63) / 64, (Hpad + 3) / 4, N),
                     dim3(256), 0, (hipStream_t)stream, imgs, Hpad, Wpad, mean[0],
                     mean[1], mean[2], std_inv[0], std_inv[1], std_inv[2], to_rgb, out);
  return (int)hipGetLastError();
}
