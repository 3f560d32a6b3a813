// Per-anchor arithmetic of the anchor head at evaluation, shared by anchor_head.hip (dense decode / selection over stored rows) and
// anchor_head_infer.hip (the same on the logits of its own product): one definition, so both run the same operations in the same
// order (the build has -ffp-contract=off) and agree bit for bit on the same fp32 logits.
// `at(i)`: the i-th value of the group being read (class logits, box codes, direction logits of ONE anchor) as fp32.
#pragma once
#include "common.h"

__device__ __forceinline__ float ah_limit_period(float v, float offset, float period) { return v - floorf(v / period + offset) * period; }

// best class of one anchor: the sigmoid score (or the value itself with normalized = 1) and its 0-based class; ties keep the lowest class
template <typename At>
__device__ __forceinline__ void ah_best_class(const At& at, int C, int normalized, float& best, int& arg) {
  best = -1.f;
  arg = 0;
  for (int c = 0; c < C; ++c) {
    const float x = at(c);
    const float s = normalized ? x : 1.f / (1.f + expf(-x));
    if (c == 0 || s > best) { best = s; arg = c; }
  }
}

// ResidualCoder.decode of one anchor (centre xa / ya, slot = z, dx, dy, dz, rotation) + the direction-bin correction (nb > 0)
template <typename AtBox, typename AtDir>
__device__ __forceinline__ void ah_decode_box(const AtBox& box, const AtDir& dir, int nb, float xa, float ya, const float* __restrict__ s,
                                              float dir_offset, float dir_limit_offset, float* o) {
  const float za = s[0], dxa = s[1], dya = s[2], dza = s[3], ra = s[4];
  const float diag = sqrtf(dxa * dxa + dya * dya);
  o[0] = box(0) * diag + xa;
  o[1] = box(1) * diag + ya;
  o[2] = box(2) * dza + za;
  o[3] = expf(box(3)) * dxa;
  o[4] = expf(box(4)) * dya;
  o[5] = expf(box(5)) * dza;
  o[6] = box(6) + ra;
  if (nb > 0) {
    int best = 0;
    float bv = dir(0);
    for (int d = 1; d < nb; ++d) {
      const float v = dir(d);
      if (v > bv) { bv = v; best = d; }
    }
    const float period = (float)(6.283185307179586 / (double)nb);
    const float rot = ah_limit_period(o[6] - dir_offset, dir_limit_offset, period);
    o[6] = (rot + dir_offset) + period * (float)best;
  }
}
