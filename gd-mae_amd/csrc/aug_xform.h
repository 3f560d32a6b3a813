// World transformation of one point, shared by the two passes of the on-GPU input pipeline (input_pipeline.hip: the SSL
// configuration; gt_sampling.hip: the fine-tune configuration), so that a point goes through the same fp32 operations in both.
// The order of operations and the arithmetic follow the reference: flip, then x' = x c - y s, y' = x s + y c (evaluated as the
// reference's matmul does: products then sum, no FMA contraction), then scale.
#pragma once
#include "common.h"

struct AugParams {   // per frame, fp32: [flip_x, flip_y, cos, sin, scale, angle (fine-tune table only), pad, pad]
  const float* tab;
  const int* frame_off;   // (B + 1) device
  int B;
};

struct AugLoad {
  const float* raw;
  int F;
  AugParams P;
  float xmin, ymin, xmax, ymax;
  __device__ int frame_of(long long i) const {
    int b = 0;
    while (b + 1 < P.B && i >= P.frame_off[b + 1]) ++b;
    return b;
  }
  // t: the frame's row of the table; x, y, z: the raw coordinates in, the transformed ones out
  __device__ static void apply(const float* t, float& x, float& y, float& z) {
    if (t[0] != 0.f) y = -y;          // flip along x: y -> -y
    if (t[1] != 0.f) x = -x;          // flip along y: x -> -x
    const float c = t[2], s = t[3];
    const float xr = __fadd_rn(__fmul_rn(x, c), __fmul_rn(y, -s));
    const float yr = __fadd_rn(__fmul_rn(x, s), __fmul_rn(y, c));
    x = __fmul_rn(xr, t[4]);
    y = __fmul_rn(yr, t[4]);
    z = __fmul_rn(z, t[4]);
  }
  __device__ void xform(long long i, int b, float& x, float& y, float& z) const {
    const float* p = raw + i * F;
    x = p[0];
    y = p[1];
    z = p[2];
    apply(P.tab + b * 8, x, y, z);
  }
  __device__ int operator()(long long i) const {
    float x, y, z;
    xform(i, frame_of(i), x, y, z);
    return (x >= xmin && x <= xmax && y >= ymin && y <= ymax) ? 1 : 0;
  }
};
