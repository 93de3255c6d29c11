// The fp32 IoU of the evaluation family (eval.hip, eval_image.hip, recall.hip):
// bbox_overlaps.py in the reference's op order.  Include only from files compiled
// with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace ldeval {

__device__ __forceinline__ float box_area(const float* b) {
  return (b[2] - b[0]) * (b[3] - b[1]);
}

// bbox_overlaps.py: overlap / max(area1 + area2 - overlap, eps); the detection
// is bboxes1 unless the image has fewer GTs than detections, and the sum is
// commutative either way
__device__ __forceinline__ float iou_ref(const float* d, float area_d, const float* g) {
  float area_g = box_area(g);
  float xs = fmaxf(d[0], g[0]), ys = fmaxf(d[1], g[1]);
  float xe = fminf(d[2], g[2]), ye = fminf(d[3], g[3]);
  float ov = fmaxf(xe - xs, 0.0f) * fmaxf(ye - ys, 0.0f);
  float uni = fmaxf(area_d + area_g - ov, 1e-6f);
  return ov / uni;
}

}  // namespace ldeval
