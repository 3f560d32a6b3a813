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
// No atomics anywhere: the result does not depend on scheduling.  The bodies of the two passes and of the reduce are those of
// csrc/eval_match.h, shared with csrc/once_eval.hip; the rotated intersection is csrc/rect_clip.h.
#include "common.h"
#include "eval_match.h"
#include "rect_clip.h"

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
    // rotation_y turns CLOCKWISE in the (x, z) plane (the reference's rbbox_to_corners): the rotation is by -ry.  The sign matters: two
    // boxes displaced along their length under one convention are displaced across their width under the other.
    const double inter = rc_intersection((double)db[0], (double)db[2], (double)db[3], (double)db[5], -(double)db[6], (double)gb[0],
                                         (double)gb[2], (double)gb[3], (double)gb[5], -(double)gb[6]);
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

// (frame f, combo k): the metric's overlap plane, the class's flag rows, the scores
__device__ inline EmView ke_view(const KeArgs& A, const float* overlaps, int f, int k) {
  const int g0 = A.gt_off[f], d0 = A.dt_off[f], cl = A.combo_cl[k];
  return {overlaps + (size_t)A.combo_metric[k] * A.NP + A.pair_off[f], A.gt_off[f + 1] - g0, A.dt_off[f + 1] - d0,
          A.ign_gt + (size_t)cl * A.NG + g0, A.ign_dt + (size_t)cl * A.ND + d0, A.dt_score + d0, A.combo_min[k]};
}

__global__ __launch_bounds__(256) void k_ke_match1(KeArgs A, const float* __restrict__ overlaps, float* __restrict__ matched) {
  const int f = blockIdx.x, lane = threadIdx.x & (GD_WAVE - 1), k = blockIdx.y * (256 / GD_WAVE) + threadIdx.x / GD_WAVE;
  if (k >= A.K) return;                                      // whole wavefronts leave together
  // the sentinel is the reference's NO_DETECTION
  em_first_pass(ke_view(A, overlaps, f, k), lane, -10000000.f, matched + (size_t)k * A.NG + A.gt_off[f]);
}

__global__ __launch_bounds__(GD_WAVE) void k_ke_thresholds(KeArgs A, const float* __restrict__ sorted, float* __restrict__ thresholds,
                                                           int* __restrict__ n_thresholds) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const float* row = sorted + (size_t)k * A.NG;
  int n = 0;
  for (int i = lane; i < A.NG; i += GD_WAVE) n += row[i] > -INFINITY ? 1 : 0;
  n = em_wave_sum(n);
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

// the orientation similarity of the true positives of one wavefront: GT rows in order within a (frame, threshold), these sums in
// frame order into the lane's threshold
struct KeSimilarity {
  bool on;                                                   // asked for, and the combo's metric is bbox
  const float *gt_alpha, *dt_alpha;                          // of the frame at hand
  double sim = 0.0, acc = 0.0;
  __device__ void hit(int g, int j) {
    if (on) sim += (1.0 + cos((double)gt_alpha[g] - (double)dt_alpha[j])) / 2.0;
  }
  __device__ void end(bool mine) {
    if (mine) acc += sim;
    sim = 0.0;
  }
};

__global__ __launch_bounds__(256) void k_ke_match2(KeArgs A, const float* __restrict__ overlaps, const float* __restrict__ dc_max,
                                                   const float* __restrict__ thresholds, const int* __restrict__ n_thresholds,
                                                   int compute_aos, int* __restrict__ part_i, double* __restrict__ part_s) {
  const int chunk = blockIdx.x, lane = threadIdx.x & (GD_WAVE - 1), k = blockIdx.y * (256 / GD_WAVE) + threadIdx.x / GD_WAVE;
  if (k >= A.K) return;
  const int metric = A.combo_metric[k], nt = n_thresholds[k];
  EmCounts acc;
  KeSimilarity sim{compute_aos && metric == 0, nullptr, nullptr};
  for (int f = chunk * kKeFrames; f < min((chunk + 1) * kKeFrames, A.F); ++f) {
    const EmView v = ke_view(A, overlaps, f, k);
    const int g0 = A.gt_off[f], d0 = A.dt_off[f];
    unsigned stuff = 0;                                      // over a DontCare box (metric 0): never a false positive
    for (int i = 0; metric == 0 && i * GD_WAVE < v.D; ++i) {
      const int j = lane + GD_WAVE * i;
      if (j < v.D && (double)dc_max[d0 + j] > v.min_ov) stuff |= 1u << i;
    }
    sim.gt_alpha = A.gt_alpha + g0, sim.dt_alpha = A.dt_alpha + d0;
    em_second_pass<kKePts>(v, lane, k, thresholds, nt, stuff, sim, acc);
  }
  const size_t o = ((size_t)chunk * A.K + k) * kKePts + lane;
  em_store_part<kKePts>(acc, lane, o, part_i);
  if (lane < kKePts) part_s[o] = sim.acc;
}

__global__ __launch_bounds__(256) void k_ke_reduce(int n_chunks, int K, const int* __restrict__ part_i, const double* __restrict__ part_s,
                                                   long long* __restrict__ pr_counts, double* __restrict__ pr_sim) {
  em_reduce<kKePts>(blockIdx.x * 256 + threadIdx.x, n_chunks, K, part_i, part_s, pr_counts, pr_sim);
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
