// Per-candidate arithmetic of the CenterHead evaluation tail, shared by center_head.hip (k_ch_decode: one thread per top-K cell, rows
// for the op-by-op tail) and center_detect.hip (the batched tail): one definition, so both run the same operations in the same order
// (the build has -ffp-contract=off) and leave the same bits for the same cell.
#pragma once
#include "common.h"

struct ChMaps {
  const float *center, *center_z, *dim, *rot, *vel, *iou;   // (B, 2 | 1 | 3 | 2 | 2 | 1, H, W); vel / iou optional
};
struct ChGeom {
  int H, W;
  float x0, y0, vsx, vsy, stride;
  float lim[6];
  float score_thresh;
  int use_thresh;
};

// One cell `c` (flat index over (class, y, x)) of sample b with heat-map score `score`: box[0 .. 6 | 8], the class inside the head, the
// clamped IoU value q (1 without an iou map).  -> inside the post-centre range and above the score threshold.
__device__ __forceinline__ bool ch_decode_cell(const ChMaps& M, const ChGeom& G, int b, long long c, float score, float* box, int& cls, float& q) {
  const long long hw = (long long)G.H * G.W;
  cls = (int)(c / hw);
  const long long site = c % hw;
  const int y = (int)(site / G.W), x = (int)(site % G.W);
  auto at = [&](const float* m, int ch, int k) { return m[((long long)b * ch + k) * hw + site]; };
  box[0] = (((float)x + at(M.center, 2, 0)) * G.stride) * G.vsx + G.x0;
  box[1] = (((float)y + at(M.center, 2, 1)) * G.stride) * G.vsy + G.y0;
  box[2] = at(M.center_z, 1, 0);
  box[3] = expf(at(M.dim, 3, 0)); box[4] = expf(at(M.dim, 3, 1)); box[5] = expf(at(M.dim, 3, 2));
  box[6] = atan2f(at(M.rot, 2, 1), at(M.rot, 2, 0));                 // rot = [cos, sin]
  if (M.vel) { box[7] = at(M.vel, 2, 0); box[8] = at(M.vel, 2, 1); }
  q = 1.f;
  if (M.iou) q = fminf(fmaxf((at(M.iou, 1, 0) + 1.f) * 0.5f, 0.f), 1.f);
  bool ok = true;
  for (int e = 0; e < 3; ++e) ok = ok && box[e] >= G.lim[e] && box[e] <= G.lim[3 + e];
  if (G.use_thresh) ok = ok && score > G.score_thresh;
  return ok;
}

static inline void ch_fill_geom(ChGeom& G, int H, int W, const float* pc_range, const float* voxel_size, float stride, const float* lim,
                                float score_thresh, int use_thresh) {
  G.H = H; G.W = W;
  G.x0 = pc_range[0]; G.y0 = pc_range[1]; G.vsx = voxel_size[0]; G.vsy = voxel_size[1]; G.stride = stride;
  for (int e = 0; e < 6; ++e) G.lim[e] = lim[e];
  G.score_thresh = score_thresh; G.use_thresh = use_thresh;
}
