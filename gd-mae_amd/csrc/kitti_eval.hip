// The official KITTI AP statistics on the device (reference pcdet/datasets/kitti/kitti_object_eval_python/eval.py: calculate_iou_partly,
// compute_statistics_jit, get_thresholds, fused_compute_statistics).  The reference runs one greedy matching per frame for
// every (class, difficulty, overlap set, metric) = "combo" and, in the second pass, for each of up to 41 score thresholds, in numba
// loops on the CPU.  All of these matchings are independent; here they are wavefronts.
//   k_ke_overlaps    one workgroup per frame, a thread per (GT row, detection) pair: image IoU, rotated BEV IoU and 3-D IoU, stored
//                    GT-major ((G_f, D_f): the matching kernels stride the detections over the lanes), and per detection the largest
//                    criterion-0 image overlap with the frame's DontCare boxes.  fp32 inputs, fp64 arithmetic, fp32 results.  The
//                    rotated intersection is a convex clipping WITHOUT the 1e-2 m corner margin of bev_iou.h (that margin costs
//                    1.4e-2 of overlap on nearly aligned pairs, the normal case of an evaluator).
//   k_ke_match1      one wavefront per (frame, combo): compute_statistics_jit(compute_fp=False).  The GT rows in order; per row the
//                    lanes stride the detections and reduce (highest score, lowest index) by wave64 shuffles; the assigned flags are
//                    one 16-bit mask per lane (detection = lane + 64 * bit).  Writes every slot of matched (combo, NG): the true
//                    positive's score, -inf elsewhere.
//   (the caller orders every row of `matched` descending)
//   k_ke_thresholds  one wavefront per combo counts the matched scores, lane 0 runs get_thresholds in fp64 (sequential by nature).
//   k_ke_match2      one wavefront per (chunk of kKeFrames frames, combo): compute_statistics_jit(compute_fp=True) for every frame of
//                    the chunk and every threshold; lane t keeps the chunk's tp / fp / fn / similarity of threshold t.
//   k_ke_reduce      one thread per (combo, threshold) adds the chunks in order.
// No atomics anywhere: the result does not depend on scheduling.
#include <limits.h>

#include "common.h"

namespace {
constexpr int kKeFrames = 8;          // frames per wavefront of the second pass (the unit of the fixed-order similarity sum)
constexpr int kKeMaxRows = 1024;      // detections / GT rows per frame: 16 mask bits per lane
constexpr int kKeMaxCombos = 108;     // 6 classes x 3 difficulties x 2 overlap sets x 3 metrics
constexpr int kKePts = 41;

struct KeArgs {
  int F, K, NG, ND;
  long long NP;
  const int *gt_off, *dt_off, *dc_off;
  const long long* pair_off;
  const float *gt_box, *gt_geo, *gt_alpha, *dt_box, *dt_geo, *dt_alpha, *dt_score, *dc_box;
  const signed char *ign_gt, *ign_dt;
  const int *combo_cl, *combo_metric, *combo_ngt;
  const double* combo_min;
};

struct D2 {
  double x, y;
};

// corners of the rectangle [x, z, l, w, ry] of a [x, y, z, l, h, w, ry] row relative to (ox, oy), in counter-clockwise order.
// rotation_y turns clockwise in the (x, z) plane (the reference's rbbox_to_corners): the rotation is by -ry.  The sign matters: two
// boxes displaced along their length under one convention are displaced across their width under the other.
__device__ inline void ke_corners(const float* b, double ox, double oy, D2 (&c)[4]) {
  const double cs = cos((double)b[6]), sn = -sin((double)b[6]);
  const double hx = 0.5 * (double)b[3], hy = 0.5 * (double)b[5], cx = (double)b[0] - ox, cy = (double)b[2] - oy;
  const double lx[4] = {-hx, hx, hx, -hx}, ly[4] = {-hy, -hy, hy, hy};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    c[k].x = cx + lx[k] * cs - ly[k] * sn;
    c[k].y = cy + lx[k] * sn + ly[k] * cs;
  }
}

// area of the intersection of the two rectangles: the subject polygon clipped by the four edges of the other (no margin)
__device__ inline double ke_rect_intersection(const float* a, const float* b) {
  const double ra = 0.5 * sqrt((double)a[3] * a[3] + (double)a[5] * a[5]), rb = 0.5 * sqrt((double)b[3] * b[3] + (double)b[5] * b[5]);
  const double dx = (double)a[0] - (double)b[0], dy = (double)a[2] - (double)b[2], reach = ra + rb + 1e-3;
  if (dx * dx + dy * dy > reach * reach) return 0.0;       // the circumscribed circles do not meet: the intersection is empty
  D2 clip[4], p[8], q[8];
  ke_corners(b, (double)a[0], (double)a[2], clip);          // coordinates relative to a's centre
  {
    D2 ca[4];
    ke_corners(a, (double)a[0], (double)a[2], ca);
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = ca[k];
  }
  int n = 4;
  for (int e = 0; e < 4; ++e) {
    const D2 p0 = clip[e], p1 = clip[(e + 1) & 3];
    const double ex = p1.x - p0.x, ey = p1.y - p0.y;
    int m = 0;
    for (int k = 0; k < n; ++k) {
      const D2 c = p[k], nx = p[k + 1 == n ? 0 : k + 1];
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
    const D2 c = p[k], nx = p[k + 1 == n ? 0 : k + 1];
    s += c.x * nx.y - nx.x * c.y;
  }
  return fabs(s) * 0.5;
}

// image overlap of boxes [x1, y1, x2, y2]: criterion -1 (IoU) or 0 (divided by the area of a)
__device__ inline double ke_image_overlap(const float* a, const float* b, bool iou) {
  const double iw = fmin((double)a[2], (double)b[2]) - fmax((double)a[0], (double)b[0]);
  if (!(iw > 0.0)) return 0.0;
  const double ih = fmin((double)a[3], (double)b[3]) - fmax((double)a[1], (double)b[1]);
  if (!(ih > 0.0)) return 0.0;
  const double aa = ((double)a[2] - (double)a[0]) * ((double)a[3] - (double)a[1]);
  const double ua = iou ? aa + ((double)b[2] - (double)b[0]) * ((double)b[3] - (double)b[1]) - iw * ih : aa;
  return iw * ih / ua;
}

__global__ __launch_bounds__(256) void k_ke_overlaps(KeArgs A, float* __restrict__ overlaps, float* __restrict__ dc_max) {
  const int f = blockIdx.x;
  const int g0 = A.gt_off[f], G = A.gt_off[f + 1] - g0, d0 = A.dt_off[f], D = A.dt_off[f + 1] - d0;
  const int c0 = A.dc_off[f], NC = A.dc_off[f + 1] - c0;
  const long long base = A.pair_off[f];
  for (int i = threadIdx.x; i < G * D; i += 256) {
    const int g = i / D, j = i - g * D;
    const float* gb = A.gt_geo + (size_t)(g0 + g) * 7;
    const float* db = A.dt_geo + (size_t)(d0 + j) * 7;
    overlaps[base + i] = (float)ke_image_overlap(A.dt_box + (size_t)(d0 + j) * 4, A.gt_box + (size_t)(g0 + g) * 4, true);
    const double inter = ke_rect_intersection(db, gb);
    double bev = 0.0, d3 = 0.0;
    if (inter > 0.0) {
      bev = inter / ((double)db[3] * db[5] + (double)gb[3] * gb[5] - inter);
      const double ih = fmin((double)db[1], (double)gb[1]) - fmax((double)db[1] - (double)db[4], (double)gb[1] - (double)gb[4]);
      if (ih > 0.0) {
        const double inc = ih * inter;
        d3 = inc / ((double)db[3] * db[4] * db[5] + (double)gb[3] * gb[4] * gb[5] - inc);
      }
    }
    overlaps[A.NP + base + i] = (float)bev;
    overlaps[2 * A.NP + base + i] = (float)d3;
  }
  for (int j = threadIdx.x; j < D; j += 256) {
    double best = 0.0;
    for (int c = 0; c < NC; ++c) best = fmax(best, ke_image_overlap(A.dt_box + (size_t)(d0 + j) * 4, A.dc_box + (size_t)(c0 + c) * 4, false));
    dc_max[d0 + j] = (float)best;
  }
}

// the wavefront's (largest v, lowest index among equal v); idx INT_MAX = none
__device__ inline void ke_argmax(float& v, int& idx) {
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
__device__ inline int ke_wave_min(int v) {
#pragma unroll
  for (int d = GD_WAVE / 2; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d, GD_WAVE));
  return v;
}
__device__ inline int ke_wave_sum(int v) {
#pragma unroll
  for (int d = GD_WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, GD_WAVE);
  return v;
}

__global__ __launch_bounds__(256) void k_ke_match1(KeArgs A, const float* __restrict__ overlaps, float* __restrict__ matched) {
  const int f = blockIdx.x, lane = threadIdx.x & (GD_WAVE - 1), k = blockIdx.y * (256 / GD_WAVE) + threadIdx.x / GD_WAVE;
  if (k >= A.K) return;                                      // whole wavefronts leave together
  const int g0 = A.gt_off[f], G = A.gt_off[f + 1] - g0, d0 = A.dt_off[f], D = A.dt_off[f + 1] - d0;
  const int cl = A.combo_cl[k];
  const double min_ov = A.combo_min[k];
  const float* ov = overlaps + (size_t)A.combo_metric[k] * A.NP + A.pair_off[f];
  const signed char* ig = A.ign_gt + (size_t)cl * A.NG + g0;
  const signed char* id = A.ign_dt + (size_t)cl * A.ND + d0;
  const float* sc = A.dt_score + d0;
  const int nI = (D + GD_WAVE - 1) / GD_WAVE;
  unsigned live = 0, assigned = 0;
  for (int i = 0; i < nI; ++i) {
    const int j = lane + GD_WAVE * i;
    if (j < D && id[j] != -1) live |= 1u << i;
  }
  for (int g = 0; g < G; ++g) {
    float out = -INFINITY;
    const int ign_g = ig[g];
    if (ign_g != -1) {
      float bs = -10000000.f;                                // the reference's NO_DETECTION: a score at or below it never matches
      int bj = INT_MAX;
      const unsigned m = live & ~assigned;
      for (int i = 0; i < nI; ++i)
        if ((m >> i) & 1u) {
          const int j = lane + GD_WAVE * i;
          if ((double)ov[(size_t)g * D + j] > min_ov && sc[j] > bs) {
            bs = sc[j];
            bj = j;
          }
        }
      ke_argmax(bs, bj);
      if (bj != INT_MAX) {
        if (lane == (bj & (GD_WAVE - 1))) assigned |= 1u << (bj / GD_WAVE);
        if (!(ign_g == 1 || id[bj] == 1)) out = bs;
      }
    }
    if (lane == 0) matched[(size_t)k * A.NG + g0 + g] = out;
  }
}

__global__ __launch_bounds__(GD_WAVE) void k_ke_thresholds(KeArgs A, const float* __restrict__ sorted, float* __restrict__ thresholds,
                                                           int* __restrict__ n_thresholds) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const float* row = sorted + (size_t)k * A.NG;
  int n = 0;
  for (int i = lane; i < A.NG; i += GD_WAVE) n += row[i] > -INFINITY ? 1 : 0;
  n = ke_wave_sum(n);
  int nt = 0;
  if (lane == 0) {
    const double num_gt = (double)A.combo_ngt[k];
    double cur = 0.0;
    for (int i = 0; i < n && nt < kKePts; ++i) {
      const double l = (double)(i + 1) / num_gt;
      const double r = i < n - 1 ? (double)(i + 2) / num_gt : l;
      if ((r - cur) < (cur - l) && i < n - 1) continue;
      thresholds[k * kKePts + nt++] = row[i];
      cur += 1 / 40.0;
    }
    n_thresholds[k] = nt;
  }
  nt = __shfl(nt, 0, GD_WAVE);
  if (lane >= nt && lane < kKePts) thresholds[k * kKePts + lane] = 0.f;
}

__global__ __launch_bounds__(256) void k_ke_match2(KeArgs A, const float* __restrict__ overlaps, const float* __restrict__ dc_max,
                                                   const float* __restrict__ thresholds, const int* __restrict__ n_thresholds,
                                                   int compute_aos, int* __restrict__ part_i, double* __restrict__ part_s) {
  const int chunk = blockIdx.x, lane = threadIdx.x & (GD_WAVE - 1), k = blockIdx.y * (256 / GD_WAVE) + threadIdx.x / GD_WAVE;
  if (k >= A.K) return;
  const int cl = A.combo_cl[k], metric = A.combo_metric[k], nt = n_thresholds[k];
  const double min_ov = A.combo_min[k];
  int acc_tp = 0, acc_fp = 0, acc_fn = 0;
  double acc_sim = 0.0;
  for (int f = chunk * kKeFrames; f < min((chunk + 1) * kKeFrames, A.F); ++f) {
    const int g0 = A.gt_off[f], G = A.gt_off[f + 1] - g0, d0 = A.dt_off[f], D = A.dt_off[f + 1] - d0;
    const float* ov = overlaps + (size_t)metric * A.NP + A.pair_off[f];
    const signed char* ig = A.ign_gt + (size_t)cl * A.NG + g0;
    const signed char* id = A.ign_dt + (size_t)cl * A.ND + d0;
    const float* sc = A.dt_score + d0;
    const int nI = (D + GD_WAVE - 1) / GD_WAVE;
    unsigned live0 = 0, live1 = 0, stuff = 0;               // ignored_det 0 / 1; over a DontCare box (metric 0)
    for (int i = 0; i < nI; ++i) {
      const int j = lane + GD_WAVE * i;
      if (j < D) {
        if (id[j] == 0) live0 |= 1u << i;
        if (id[j] == 1) live1 |= 1u << i;
        if (metric == 0 && (double)dc_max[d0 + j] > min_ov) stuff |= 1u << i;
      }
    }
    for (int t = 0; t < nt; ++t) {
      const float thr = thresholds[k * kKePts + t];
      unsigned keep = 0, assigned = 0;
      for (int i = 0; i < nI; ++i) {
        const int j = lane + GD_WAVE * i;
        if (j < D && !(sc[j] < thr)) keep |= 1u << i;
      }
      const unsigned c0 = live0 & keep, c1 = live1 & keep;
      int tp = 0, fn = 0;
      double sim = 0.0;
      for (int g = 0; g < G; ++g) {
        const int ign_g = ig[g];
        if (ign_g == -1) continue;
        // a non-ignored detection with the largest overlap (lowest index among equals) wins; without one, the first ignored detection
        float bo = -1.f;
        int bj = INT_MAX;
        unsigned m = c0 & ~assigned;
        for (int i = 0; i < nI; ++i)
          if ((m >> i) & 1u) {
            const int j = lane + GD_WAVE * i;
            const float o = ov[(size_t)g * D + j];
            if ((double)o > min_ov && o > bo) {
              bo = o;
              bj = j;
            }
          }
        ke_argmax(bo, bj);
        bool ignored_pick = false;
        if (bj == INT_MAX) {
          m = c1 & ~assigned;
          for (int i = 0; i < nI && bj == INT_MAX; ++i)
            if ((m >> i) & 1u) {
              const int j = lane + GD_WAVE * i;
              if ((double)ov[(size_t)g * D + j] > min_ov) bj = j;
            }
          bj = ke_wave_min(bj);
          ignored_pick = true;
        }
        if (bj == INT_MAX) {
          if (ign_g == 0) ++fn;
        } else {
          if (lane == (bj & (GD_WAVE - 1))) assigned |= 1u << (bj / GD_WAVE);
          if (!(ign_g == 1 || ignored_pick)) {
            ++tp;
            if (compute_aos && metric == 0) sim += (1.0 + cos((double)A.gt_alpha[g0 + g] - (double)A.dt_alpha[d0 + bj])) / 2.0;
          }
        }
      }
      const int fp = ke_wave_sum(__popc(c0 & ~assigned & ~stuff));
      if (lane == t) {
        acc_tp += tp;
        acc_fp += fp;
        acc_fn += fn;
        acc_sim += sim;
      }
    }
  }
  if (lane < kKePts) {
    const size_t o = ((size_t)chunk * A.K + k) * kKePts + lane;
    part_i[o * 3 + 0] = acc_tp;
    part_i[o * 3 + 1] = acc_fp;
    part_i[o * 3 + 2] = acc_fn;
    part_s[o] = acc_sim;
  }
}

__global__ __launch_bounds__(256) void k_ke_reduce(int n_chunks, int K, const int* __restrict__ part_i, const double* __restrict__ part_s,
                                                   long long* __restrict__ pr_counts, double* __restrict__ pr_sim) {
  const int i = blockIdx.x * 256 + threadIdx.x;              // (combo, threshold)
  if (i >= K * kKePts) return;
  long long tp = 0, fp = 0, fn = 0;
  double sim = 0.0;
  for (int c = 0; c < n_chunks; ++c) {
    const size_t o = (size_t)c * K * kKePts + i;
    tp += part_i[o * 3 + 0];
    fp += part_i[o * 3 + 1];
    fn += part_i[o * 3 + 2];
    sim += part_s[o];
  }
  pr_counts[i * 3 + 0] = tp;
  pr_counts[i * 3 + 1] = fp;
  pr_counts[i * 3 + 2] = fn;
  pr_sim[i] = sim;
}

size_t ke_part_i_bytes(int n_frames, int n_combos) { return gd_align((size_t)gd_div_up(n_frames, kKeFrames) * n_combos * kKePts * 3 * sizeof(int)); }
size_t ke_part_s_bytes(int n_frames, int n_combos) { return gd_align((size_t)gd_div_up(n_frames, kKeFrames) * n_combos * kKePts * sizeof(double)); }
}  // namespace

extern "C" int gdmae_kitti_eval_frames_per_chunk() { return kKeFrames; }

extern "C" size_t gdmae_kitti_eval_workspace_bytes(int n_frames, int n_combos) {
  if (n_frames < 0 || n_combos < 0) return 0;
  return ke_part_i_bytes(n_frames, n_combos) + ke_part_s_bytes(n_frames, n_combos);
}

extern "C" int gdmae_kitti_eval(int stages, int n_frames, int n_combos, const int* host_gt_off, const int* host_dt_off, const int* host_dc_off,
                                const int* gt_off, const int* dt_off, const int* dc_off, const long long* pair_off, const float* gt_box,
                                const float* gt_geo, const float* gt_alpha, const float* dt_box, const float* dt_geo, const float* dt_alpha,
                                const float* dt_score, const float* dc_box, const signed char* ignored_gt, const signed char* ignored_dt,
                                const int* combo_cl, const int* combo_metric, const double* combo_min_overlap, const int* combo_num_gt,
                                int compute_aos, float* overlaps, float* dc_max, float* matched, const float* sorted_scores,
                                float* thresholds, int* n_thresholds, long long* pr_counts, double* pr_sim, void* workspace,
                                size_t workspace_bytes, void* stream) {
  GD_REQUIRE(stages == 1 || stages == 2, "kitti_eval: stages is 1 (overlaps, first pass) or 2 (thresholds, second pass)");
  GD_REQUIRE(n_frames >= 1, "kitti_eval: negative or zero frame count");
  GD_REQUIRE(n_combos >= 1 && n_combos <= kKeMaxCombos, "kitti_eval: 1 .. 108 (class, difficulty, overlap set, metric) combinations");
  GD_REQUIRE(host_gt_off && host_dt_off && host_dc_off, "kitti_eval: the host copies of the frame offsets are required");
  GD_REQUIRE(host_gt_off[0] == 0 && host_dt_off[0] == 0 && host_dc_off[0] == 0, "kitti_eval: frame offsets start at 0");
  long long np = 0;
  for (int f = 0; f < n_frames; ++f) {
    const long long g = (long long)host_gt_off[f + 1] - host_gt_off[f], d = (long long)host_dt_off[f + 1] - host_dt_off[f];
    GD_REQUIRE(g >= 0 && d >= 0 && host_dc_off[f + 1] >= host_dc_off[f], "kitti_eval: negative GT, detection or DontCare count in a frame");
    GD_REQUIRE(g <= kKeMaxRows, "kitti_eval: more than 1024 GT rows in a frame");
    GD_REQUIRE(d <= kKeMaxRows, "kitti_eval: more than 1024 detections in a frame");
    np += g * d;
  }
  const size_t need = gdmae_kitti_eval_workspace_bytes(n_frames, n_combos);
  GD_REQUIRE(stages == 1 || (workspace && workspace_bytes >= need), "kitti_eval: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  KeArgs A;
  A.F = n_frames; A.K = n_combos; A.NG = host_gt_off[n_frames]; A.ND = host_dt_off[n_frames]; A.NP = np;
  A.gt_off = gt_off; A.dt_off = dt_off; A.dc_off = dc_off; A.pair_off = pair_off;
  A.gt_box = gt_box; A.gt_geo = gt_geo; A.gt_alpha = gt_alpha; A.dt_box = dt_box; A.dt_geo = dt_geo; A.dt_alpha = dt_alpha;
  A.dt_score = dt_score; A.dc_box = dc_box; A.ign_gt = ignored_gt; A.ign_dt = ignored_dt;
  A.combo_cl = combo_cl; A.combo_metric = combo_metric; A.combo_ngt = combo_num_gt; A.combo_min = combo_min_overlap;
  const int wg_combos = gd_div_up(n_combos, 256 / GD_WAVE);
  if (stages == 1) {
    hipLaunchKernelGGL(k_ke_overlaps, dim3(n_frames), dim3(256), 0, st, A, overlaps, dc_max);
    GD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ke_match1, dim3(n_frames, wg_combos), dim3(256), 0, st, A, (const float*)overlaps, matched);
    GD_LAUNCH_CHECK();
    return 0;
  }
  const int n_chunks = gd_div_up(n_frames, kKeFrames);
  int* part_i = (int*)workspace;
  double* part_s = (double*)((char*)workspace + ke_part_i_bytes(n_frames, n_combos));
  hipLaunchKernelGGL(k_ke_thresholds, dim3(n_combos), dim3(GD_WAVE), 0, st, A, sorted_scores, thresholds, n_thresholds);
  GD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ke_match2, dim3(n_chunks, wg_combos), dim3(256), 0, st, A, (const float*)overlaps, (const float*)dc_max,
                     (const float*)thresholds, (const int*)n_thresholds, compute_aos, part_i, part_s);
  GD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ke_reduce, dim3(gd_div_up(n_combos * kKePts, 256)), dim3(256), 0, st, n_chunks, n_combos, (const int*)part_i,
                     (const double*)part_s, pr_counts, pr_sim);
  GD_LAUNCH_CHECK();
  return 0;
}
