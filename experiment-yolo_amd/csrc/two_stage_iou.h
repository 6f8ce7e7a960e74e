// IoU of the two-stage script, shared by two_stage.hip and two_stage_batch.hip so that the single-image and the batched kernels
// evaluate one expression.  Include after `#pragma clang fp contract(off)`: the operation order is the reference's.
#pragma once
#pragma clang fp contract(off)

// IoU of calculate_iou_tensor (:70-87): 0 for empty intersection or a non-positive area, no epsilon.
static __device__ __forceinline__ float iou_plain(float ax1, float ay1, float ax2, float ay2, float bx1, float by1, float bx2, float by2) {
  const float x1 = fmaxf(ax1, bx1), y1 = fmaxf(ay1, by1), x2 = fminf(ax2, bx2), y2 = fminf(ay2, by2);
  if (x2 <= x1 || y2 <= y1) return 0.f;
  const float inter = (x2 - x1) * (y2 - y1);
  const float a1 = (ax2 - ax1) * (ay2 - ay1), a2 = (bx2 - bx1) * (by2 - by1);
  if (a1 <= 0.f || a2 <= 0.f) return 0.f;
  const float uni = a1 + a2 - inter;
  return uni > 0.f ? inter / uni : 0.f;
}
