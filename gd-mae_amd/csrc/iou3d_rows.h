// 3-D IoU of a box pair and the valid rows of a zero-padded GT table: the ONE definition that roi_targets.hip (one wavefront per RoI, a
// reduction over GT rows) and recall_record.hip (one wavefront per GT row, a reduction over predicted rows) share.
#pragma once
#include "bev_iou.h"

namespace {
// last row of a (G, cols) table with a non-zero entry, -1 when there is none: whole wavefront
__device__ inline int rt_last_nonzero_row(const float* __restrict__ gt, int G, int cols, int lane) {
  int last = -1;
  for (int g = lane; g < G; g += GD_WAVE) {
    bool any = false;
    for (int c = 0; c < cols; ++c) any = any || gt[(size_t)g * cols + c] != 0.f;
    if (any) last = g;
  }
#pragma unroll
  for (int d = GD_WAVE / 2; d > 0; d >>= 1) last = max(last, __shfl_xor(last, d, GD_WAVE));
  return last;
}

// rows 0 .. k of a sample's (G, 8) GT table are valid, k = last row with a non-zero entry (0 when there is none): whole wavefront
__device__ inline int rt_valid_rows(const float* __restrict__ gt, int G, int lane) { return max(rt_last_nonzero_row(gt, G, 8, lane), 0) + 1; }

// the operations of boxes_iou3d_gpu(a, b) on one pair
__device__ inline float rt_iou3d(const float* a, const float* b) {
  const float a_max = a[2] + a[5] / 2, a_min = a[2] - a[5] / 2;
  const float b_max = b[2] + b[5] / 2, b_min = b[2] - b[5] / 2;
  const float oh = fmaxf(fminf(a_max, b_max) - fmaxf(a_min, b_min), 0.f);
  // centres further apart than the half-diagonals (+ 0.1 m, far beyond the 1e-2 margin of the corner test): no crossing, no corner
  // inside the other box, the polygon is empty and bev_overlap returns exactly 0
  const float ra = 0.5f * sqrtf(a[3] * a[3] + a[4] * a[4]), rb = 0.5f * sqrtf(b[3] * b[3] + b[4] * b[4]);
  const float dx = a[0] - b[0], dy = a[1] - b[1], reach = ra + rb + 0.1f;
  const float ov = (dx * dx + dy * dy > reach * reach) ? 0.f : bev_overlap(a, b);
  const float o3 = ov * oh;
  const float va = a[3] * a[4] * a[5], vb = b[3] * b[4] * b[5];
  return o3 / fmaxf(va + vb - o3, 1e-6f);
}
}  // namespace
