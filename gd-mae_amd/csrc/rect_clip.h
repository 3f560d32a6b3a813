// Exact intersection area of two rotated rectangles on plain doubles (cx, cy, dx, dy, angle), and the wave64 reductions of the
// evaluator kernels (csrc/once_eval.hip).  The clipping is the one of csrc/kitti_eval.hip: the subject polygon
// cut by the four edges of the other rectangle in fp64, no vertex sort, no corner margin.  Folding the two files onto this header
// is a follow-up: kitti_eval.hip keeps its own copy so that its compiled code does not move.
#pragma once
#include <limits.h>

#include "common.h"

struct RcPoint {
  double x, y;
};

// corners of (cx, cy, dx, dy, angle) relative to (ox, oy), the angle counter-clockwise.  The sign convention MATTERS for an
// intersection whenever the centres differ (mirroring the angles alone is no mirror image): a caller whose angle turns clockwise
// passes its negative.
__device__ inline void rc_corners(double cx, double cy, double dx, double dy, double angle, double ox, double oy, RcPoint (&c)[4]) {
  const double cs = cos(angle), sn = sin(angle);
  const double hx = 0.5 * dx, hy = 0.5 * dy, px = cx - ox, py = cy - oy;
  const double lx[4] = {-hx, hx, hx, -hx}, ly[4] = {-hy, -hy, hy, hy};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    c[k].x = px + lx[k] * cs - ly[k] * sn;
    c[k].y = py + lx[k] * sn + ly[k] * cs;
  }
}

// a = (ax, ay, adx, ady, aangle), b likewise -> area of the intersection.  Early exit when the circumscribed circles do not meet.
__device__ inline double rc_intersection(double ax, double ay, double adx, double ady, double aang, double bx, double by, double bdx,
                                         double bdy, double bang) {
  const double ra = 0.5 * sqrt(adx * adx + ady * ady), rb = 0.5 * sqrt(bdx * bdx + bdy * bdy);
  const double ox = ax - bx, oy = ay - by, reach = ra + rb + 1e-3;
  if (ox * ox + oy * oy > reach * reach) return 0.0;
  RcPoint clip[4], p[8], q[8];
  rc_corners(bx, by, bdx, bdy, bang, ax, ay, clip);         // coordinates relative to a's centre
  {
    RcPoint ca[4];
    rc_corners(ax, ay, adx, ady, aang, ax, ay, ca);
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = ca[k];
  }
  int n = 4;
  for (int e = 0; e < 4; ++e) {
    const RcPoint p0 = clip[e], p1 = clip[(e + 1) & 3];
    const double ex = p1.x - p0.x, ey = p1.y - p0.y;
    int m = 0;
    for (int k = 0; k < n; ++k) {
      const RcPoint c = p[k], nx = p[k + 1 == n ? 0 : k + 1];
      const double sc = ex * (c.y - p0.y) - ey * (c.x - p0.x), sn = ex * (nx.y - p0.y) - ey * (nx.x - p0.x);
      if (sc >= 0.0 && m < 8) q[m++] = c;
      if ((sc >= 0.0) != (sn >= 0.0) && m < 8) {
        const double t = sc / (sc - sn);
        q[m].x = c.x + t * (nx.x - c.x);
        q[m].y = c.y + t * (nx.y - c.y);
        ++m;
      }
    }
    n = m;
    if (n == 0) return 0.0;
    for (int k = 0; k < n; ++k) p[k] = q[k];
  }
  double s = 0.0;
  for (int k = 0; k < n; ++k) {
    const RcPoint c = p[k], nx = p[k + 1 == n ? 0 : k + 1];
    s += c.x * nx.y - nx.x * c.y;
  }
  return fabs(s) * 0.5;
}

// the wavefront's (largest v, lowest index among equal v); idx INT_MAX = none
__device__ inline void rc_wave_argmax(float& v, int& idx) {
#pragma unroll
  for (int d = GD_WAVE / 2; d > 0; d >>= 1) {
    const float ov = __shfl_xor(v, d, GD_WAVE);
    const int oi = __shfl_xor(idx, d, GD_WAVE);
    if (oi != INT_MAX && (idx == INT_MAX || ov > v || (ov == v && oi < idx))) {
      v = ov;
      idx = oi;
    }
  }
}
__device__ inline int rc_wave_min(int v) {
#pragma unroll
  for (int d = GD_WAVE / 2; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d, GD_WAVE));
  return v;
}
__device__ inline int rc_wave_sum(int v) {
#pragma unroll
  for (int d = GD_WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, GD_WAVE);
  return v;
}
