// Rotated bird's-eye-view overlap / IoU of two boxes [x, y, z, dx, dy, dz, heading]: the ONE definition of the arithmetic that
// iou3d_nms.hip (pair matrices, gdmae_nms_bev) and center_detect.hip (the batched CenterHead tail) share, so that both set the same
// suppression bits on the same boxes (the build has -ffp-contract=off).  What the helpers restate of the reference, and why operation
// by operation, is written at the top of iou3d_nms.hip.
#pragma once
#include "common.h"

namespace {
constexpr float kEps = 1e-8f;
constexpr float kMargin = 1e-2f;

struct P2 {
  float x, y;
};
__device__ inline float cross3(const P2& a, const P2& b, const P2& o) { return (a.x - o.x) * (b.y - o.y) - (b.x - o.x) * (a.y - o.y); }

__device__ inline void box_corners(const float* b, P2 (&c)[5]) {
  const float hx = b[3] * 0.5f, hy = b[4] * 0.5f;
  const float cs = cosf(b[6]), sn = sinf(b[6]);
  const float lx[4] = {-hx, hx, hx, -hx}, ly[4] = {-hy, -hy, hy, hy};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // rotate the axis-aligned corner about the centre (the reference builds the absolute corner first, then rotates the
    // difference to the centre: identical arithmetic)
    const float px = (b[0] + lx[k]) - b[0], py = (b[1] + ly[k]) - b[1];
    c[k].x = px * cs + py * (-sn) + b[0];
    c[k].y = px * sn + py * cs + b[1];
  }
  c[4] = c[0];
}

__device__ inline bool inside_with_margin(const float* b, const P2& p) {
  const float cs = cosf(-b[6]), sn = sinf(-b[6]);
  const float rx = (p.x - b[0]) * cs + (p.y - b[1]) * (-sn);
  const float ry = (p.x - b[0]) * sn + (p.y - b[1]) * cs;
  return fabsf(rx) < b[3] * 0.5f + kMargin && fabsf(ry) < b[4] * 0.5f + kMargin;
}

// proper crossing of segments p0-p1 and q0-q1
__device__ inline bool seg_cross(const P2& p1, const P2& p0, const P2& q1, const P2& q0, P2& out) {
  const bool rect = fminf(p0.x, p1.x) <= fmaxf(q0.x, q1.x) && fminf(q0.x, q1.x) <= fmaxf(p0.x, p1.x) &&
                    fminf(p0.y, p1.y) <= fmaxf(q0.y, q1.y) && fminf(q0.y, q1.y) <= fmaxf(p0.y, p1.y);
  if (!rect) return false;
  const float s1 = cross3(q0, p1, p0), s2 = cross3(p1, q1, p0), s3 = cross3(p0, q1, q0), s4 = cross3(q1, p1, q0);
  if (!(s1 * s2 > 0.f && s3 * s4 > 0.f)) return false;
  const float s5 = cross3(q1, p1, p0);
  if (fabsf(s5 - s1) > kEps) {
    out.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
    out.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
  } else {
    const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
    const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
    const float D = a0 * b1 - a1 * b0;
    out.x = (b0 * c1 - b1 * c0) / D;
    out.y = (a1 * c0 - a0 * c1) / D;
  }
  return true;
}

__device__ inline float bev_overlap(const float* a, const float* b) {
  P2 ca[5], cb[5];
  box_corners(a, ca);
  box_corners(b, cb);
  P2 pts[24];
  int n = 0;
  float sx = 0.f, sy = 0.f;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      P2 x;
      if (seg_cross(ca[i + 1], ca[i], cb[j + 1], cb[j], x)) {
        sx += x.x; sy += x.y;
        pts[n++] = x;
      }
    }
  for (int k = 0; k < 4; ++k) {
    if (inside_with_margin(a, cb[k])) { sx += cb[k].x; sy += cb[k].y; pts[n++] = cb[k]; }
    if (inside_with_margin(b, ca[k])) { sx += ca[k].x; sy += ca[k].y; pts[n++] = ca[k]; }
  }
  if (n < 3) return 0.f;
  const float mx = sx / n, my = sy / n;
  float ang[24];
  for (int i = 0; i < n; ++i) ang[i] = atan2f(pts[i].y - my, pts[i].x - mx);
  // ascending angle (stable exchange sort, n <= 24)
  for (int j = 0; j < n - 1; ++j)
    for (int i = 0; i < n - j - 1; ++i)
      if (ang[i] > ang[i + 1]) {
        const float t = ang[i]; ang[i] = ang[i + 1]; ang[i + 1] = t;
        const P2 q = pts[i]; pts[i] = pts[i + 1]; pts[i + 1] = q;
      }
  float area = 0.f;
  for (int k = 0; k < n - 1; ++k) {
    const float ux = pts[k].x - pts[0].x, uy = pts[k].y - pts[0].y, vx = pts[k + 1].x - pts[0].x, vy = pts[k + 1].y - pts[0].y;
    area += ux * vy - uy * vx;
  }
  return fabsf(area) * 0.5f;
}

__device__ inline float bev_iou(const float* a, const float* b) {
  const float ov = bev_overlap(a, b);
  return ov / fmaxf(a[3] * a[4] + b[3] * b[4] - ov, kEps);
}
__device__ inline float axis_iou(const float* a, const float* b) {
  const float l = fmaxf(a[0] - a[3] * 0.5f, b[0] - b[3] * 0.5f), r = fminf(a[0] + a[3] * 0.5f, b[0] + b[3] * 0.5f);
  const float t = fmaxf(a[1] - a[4] * 0.5f, b[1] - b[4] * 0.5f), bo = fminf(a[1] + a[4] * 0.5f, b[1] + b[4] * 0.5f);
  const float inter = fmaxf(r - l, 0.f) * fmaxf(bo - t, 0.f);
  return inter / fmaxf(a[3] * a[4] + b[3] * b[4] - inter, kEps);
}
}  // namespace
