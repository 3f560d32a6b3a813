// The ONCE AP statistics on the device (reference pcdet/datasets/once/once_eval/evaluation.py: compute_iou3d, filter_data,
// accumulate_scores, get_thresholds, compute_statistics).  The reference runs one greedy matching per frame for every
// (class, distance band) = "combo" and, in the second pass, one more for each of up to num_pr_points + 1 score thresholds, in numba
// loops on the CPU.  All of these matchings are independent; here they are wavefronts, as in csrc/kitti_eval.hip.
//   k_oe_overlaps    one workgroup per frame, a thread per (GT row, prediction) pair: the 3-D IoU of lidar boxes (x, y, z, l, w, h, rot)
//                    with the heading rule, stored GT-major ((G_f, P_f): the matching kernels stride the predictions over the lanes).
//                    fp32 inputs, fp64 arithmetic, fp32 results.  The same launch writes the int8 flags (class, band, row) of both
//                    sides from the name codes, the accept masks and the fp64 distance.
//   k_oe_match1      one wavefront per (frame, combo): accumulate_scores.  The GT rows in order; per row the lanes stride the
//                    predictions and reduce (highest score, lowest index) by wave64 shuffles; the assigned flags are one 16-bit mask per
//                    lane (prediction = lane + 64 * bit).  Writes every slot of matched (combo, NG): the true positive's score, -inf
//                    elsewhere.
//   (the caller orders every row of `matched` descending)
//   k_oe_thresholds  one wavefront per combo counts the matched scores and the flag-0 GT rows, lane 0 runs get_thresholds in fp64.
//   k_oe_match2      one wavefront per (chunk of kOeFrames frames, combo): compute_statistics for every frame of the chunk and every
//                    threshold; lane t keeps the chunk's tp / fp / fn of threshold t.
//   k_oe_reduce      one thread per (combo, threshold) adds the chunks in order.
// No atomics anywhere: the result does not depend on scheduling.  The bodies of the two passes and of the reduce are those of
// csrc/eval_match.h, shared with csrc/kitti_eval.hip; the rotated intersection is csrc/rect_clip.h.
#include "common.h"
#include "eval_match.h"
#include "rect_clip.h"

namespace {
constexpr int kOeFrames = 8;          // frames per wavefront of the second pass
constexpr int kOeMaxRows = 1024;      // predictions / GT rows per frame: 16 mask bits per lane
constexpr int kOeMaxClasses = 32;
constexpr int kOePts = 64;            // threshold slots per combo: num_pr_points + 1 <= 64, one lane each
constexpr int kOeMaxPrPoints = kOePts - 1;

struct OeArgs {
  int F, C, B, K, NG, ND, mode, npp, heading;
  const int *gt_off, *pd_off;
  const long long* pair_off;
  const float *gt_box, *pd_box, *pd_score;
  const int *gt_code, *pd_code;
  const unsigned* accept;
  const double* iou_thr;
  const signed char *flag_gt, *flag_pd;
};

// distance band of a row: 0 below 30 m, 1 below 50 m, 2 from 50 m, 3 in none (a distance that is not a number)
__device__ inline int oe_band_of(const float* b) {
  const double x = (double)b[0], y = (double)b[1], z = (double)b[2];
  const double dist = sqrt(x * x + y * y + z * z);
  return dist < 30.0 ? 0 : (dist >= 30.0 && dist < 50.0) ? 1 : dist >= 50.0 ? 2 : 3;
}

__device__ inline void oe_write_flags(const OeArgs& A, const float* box, int code, signed char* flags, size_t n_rows, size_t row) {
  const int band = oe_band_of(box);
  for (int c = 0; c < A.C; ++c) {
    const bool accepted = (A.accept[c] >> (code & 31)) & 1u;
    for (int b = 0; b < A.B; ++b) {
      const bool inside = A.mode == 0 || (A.mode == 1 ? band == b : (b == 0 || band == b - 1));
      // the reference's filter_data writes the band after the class: a row outside the band is 1 whatever its class
      flags[((size_t)c * A.B + b) * n_rows + row] = inside ? (accepted ? 0 : -1) : 1;
    }
  }
}

__device__ inline float oe_iou3d(const float* g, const float* p, int heading) {
  if (heading) {
    double d = fabs((double)g[6] - (double)p[6]);
    if (d >= M_PI) d = 2 * M_PI - d;                         // literally the reference: nothing wraps beyond 2 pi
    if (d > M_PI / 2) return 0.f;
  }
  const double gz = (double)g[2], gh = (double)g[5], pz = (double)p[2], ph = (double)p[5];
  const double ih = fmin(gz + gh * 0.5, pz + ph * 0.5) - fmax(gz - gh * 0.5, pz - ph * 0.5);
  if (!(ih > 0.0)) return 0.f;
  // rot turns CLOCKWISE in (x, y), as the reference's rbbox_to_corners has it: two boxes displaced along their length under one
  // convention are displaced across their width under the other
  const double inter = rc_intersection((double)g[0], (double)g[1], (double)g[3], (double)g[4], -(double)g[6], (double)p[0], (double)p[1],
                                       (double)p[3], (double)p[4], -(double)p[6]);
  if (!(inter > 0.0)) return 0.f;
  const double i3 = inter * ih;
  const double uni = (double)g[3] * (double)g[4] * (double)g[5] + (double)p[3] * (double)p[4] * (double)p[5] - i3;
  if (uni == 0.0) return 0.f;                                // the reference's 0 / 0: never above a threshold
  return (float)(i3 / uni);
}

__global__ __launch_bounds__(256) void k_oe_overlaps(OeArgs A, float* __restrict__ overlaps, signed char* __restrict__ flag_gt,
                                                     signed char* __restrict__ flag_pd) {
  const int f = blockIdx.x;
  const int g0 = A.gt_off[f], G = A.gt_off[f + 1] - g0, d0 = A.pd_off[f], D = A.pd_off[f + 1] - d0;
  const long long base = A.pair_off[f];
  for (int i = threadIdx.x; i < G * D; i += 256) {
    const int g = i / D, j = i - g * D;
    overlaps[base + i] = oe_iou3d(A.gt_box + (size_t)(g0 + g) * 7, A.pd_box + (size_t)(d0 + j) * 7, A.heading);
  }
  for (int g = threadIdx.x; g < G; g += 256) oe_write_flags(A, A.gt_box + (size_t)(g0 + g) * 7, A.gt_code[g0 + g], flag_gt, A.NG, g0 + g);
  for (int j = threadIdx.x; j < D; j += 256) oe_write_flags(A, A.pd_box + (size_t)(d0 + j) * 7, A.pd_code[d0 + j], flag_pd, A.ND, d0 + j);
}

// (frame f, combo k): the one overlap plane, the combo's flag rows, the scores
__device__ inline EmView oe_view(const OeArgs& A, const float* overlaps, int f, int k) {
  const int g0 = A.gt_off[f], d0 = A.pd_off[f];
  return {overlaps + A.pair_off[f], A.gt_off[f + 1] - g0, A.pd_off[f + 1] - d0, A.flag_gt + (size_t)k * A.NG + g0,
          A.flag_pd + (size_t)k * A.ND + d0, A.pd_score + d0, A.iou_thr[k / A.B]};
}

__global__ __launch_bounds__(256) void k_oe_match1(OeArgs A, const float* __restrict__ overlaps, float* __restrict__ matched) {
  const int f = blockIdx.x, lane = threadIdx.x & (GD_WAVE - 1), k = blockIdx.y * (256 / GD_WAVE) + threadIdx.x / GD_WAVE;
  if (k >= A.K) return;                                      // whole wavefronts leave together
  em_first_pass(oe_view(A, overlaps, f, k), lane, -1.f, matched + (size_t)k * A.NG + A.gt_off[f]);      // -1: the reference's sentinel
}

__global__ __launch_bounds__(GD_WAVE) void k_oe_thresholds(OeArgs A, const float* __restrict__ sorted, int* __restrict__ num_valid,
                                                           float* __restrict__ thresholds, int* __restrict__ n_thresholds) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const float* row = sorted + (size_t)k * A.NG;
  const signed char* ig = A.flag_gt + (size_t)k * A.NG;
  int n = 0, nv = 0;
  for (int i = lane; i < A.NG; i += GD_WAVE) {
    n += row[i] > -INFINITY ? 1 : 0;
    nv += ig[i] == 0 ? 1 : 0;
  }
  n = em_wave_sum(n);
  nv = em_wave_sum(nv);
  if (nv == 0) n = 0;                                        // no true positive without a valid GT row
  int nt = 0;
  if (lane == 0) {
    const double num_gt = (double)nv, step = 1.0 / (double)A.npp, eps = 1e-6;
    double level = 0.0;
    for (int i = 0; i < n && nt < 2 * kOePts; ++i) {
      const double l = (double)(i + 1) / num_gt;
      const double r = i < n - 1 ? (double)(i + 2) / num_gt : l;
      if (r + l < 2 * level && i < n - 1) continue;
      const float s = row[i];
      if (nt < kOePts) thresholds[k * kOePts + nt] = s;
      ++nt;
      level += step;
      while (r + l + eps > 2 * level && nt < 2 * kOePts) {   // the count is at most num_pr_points + 1; the caller checks it
        if (nt < kOePts) thresholds[k * kOePts + nt] = s;
        ++nt;
        level += step;
      }
    }
    n_thresholds[k] = nt;
    num_valid[k] = nv;
  }
  nt = __shfl(nt, 0, GD_WAVE);
  if (lane >= nt) thresholds[k * kOePts + lane] = 0.f;
}

__global__ __launch_bounds__(256) void k_oe_match2(OeArgs A, const float* __restrict__ overlaps, const float* __restrict__ thresholds,
                                                   const int* __restrict__ n_thresholds, int* __restrict__ part) {
  const int chunk = blockIdx.x, lane = threadIdx.x & (GD_WAVE - 1), k = blockIdx.y * (256 / GD_WAVE) + threadIdx.x / GD_WAVE;
  if (k >= A.K) return;
  const int nt = min(n_thresholds[k], kOePts);
  EmCounts acc;
  EmNoHook none;
  for (int f = chunk * kOeFrames; f < min((chunk + 1) * kOeFrames, A.F); ++f)
    em_second_pass<kOePts>(oe_view(A, overlaps, f, k), lane, k, thresholds, nt, 0u, none, acc);
  em_store_part<kOePts>(acc, lane, ((size_t)chunk * A.K + k) * kOePts + lane, part);
}

__global__ __launch_bounds__(256) void k_oe_reduce(int n_chunks, int K, const int* __restrict__ part, long long* __restrict__ counts) {
  em_reduce<kOePts>(blockIdx.x * 256 + threadIdx.x, n_chunks, K, part, nullptr, counts, nullptr);
}

int oe_host_bands(int mode) { return mode == 0 ? 1 : mode == 1 ? 3 : 4; }
}  // namespace

extern "C" int gdmae_once_eval_frames_per_chunk() { return kOeFrames; }

extern "C" size_t gdmae_once_eval_workspace_bytes(int n_frames, int n_combos) {
  if (n_frames < 0 || n_combos < 0) return 0;
  return gd_align((size_t)gd_div_up(n_frames, kOeFrames) * n_combos * kOePts * 3 * sizeof(int));
}

extern "C" int gdmae_once_eval(int stages, int n_frames, int n_classes, int difficulty_mode, int num_pr_points, int with_heading,
                               const int* host_gt_off, const int* host_pred_off, const int* gt_off, const int* pred_off,
                               const long long* pair_off, const float* gt_box, const float* pred_box, const float* pred_score,
                               const int* gt_code, const int* pred_code, const unsigned* accept, const double* iou_threshold,
                               float* overlaps, signed char* flag_gt, signed char* flag_pred, float* matched, const float* sorted_scores,
                               int* num_valid, float* thresholds, int* n_thresholds, long long* counts, void* workspace,
                               size_t workspace_bytes, void* stream) {
  GD_REQUIRE(stages == 1 || stages == 2, "once_eval: stages is 1 (overlaps, flags, first pass) or 2 (thresholds, second pass)");
  GD_REQUIRE(n_frames >= 1, "once_eval: negative or zero frame count");
  GD_REQUIRE(n_classes >= 1 && n_classes <= kOeMaxClasses, "once_eval: 1 .. 32 evaluated classes");
  GD_REQUIRE(difficulty_mode >= 0 && difficulty_mode <= 2, "once_eval: difficulty_mode is 0 (Overall), 1 (Distance) or 2 (Overall&Distance)");
  GD_REQUIRE(num_pr_points >= 1 && num_pr_points <= kOeMaxPrPoints, "once_eval: num_pr_points outside 1 .. 63");
  GD_REQUIRE(host_gt_off && host_pred_off, "once_eval: the host copies of the frame offsets are required");
  GD_REQUIRE(host_gt_off[0] == 0 && host_pred_off[0] == 0, "once_eval: frame offsets start at 0");
  for (int f = 0; f < n_frames; ++f) {
    const long long g = (long long)host_gt_off[f + 1] - host_gt_off[f], d = (long long)host_pred_off[f + 1] - host_pred_off[f];
    GD_REQUIRE(g >= 0 && d >= 0, "once_eval: negative GT or prediction count in a frame");
    GD_REQUIRE(g <= kOeMaxRows, "once_eval: more than 1024 GT rows in a frame");
    GD_REQUIRE(d <= kOeMaxRows, "once_eval: more than 1024 predictions in a frame");
  }
  const int n_bands = oe_host_bands(difficulty_mode), n_combos = n_classes * n_bands;
  const size_t need = gdmae_once_eval_workspace_bytes(n_frames, n_combos);
  GD_REQUIRE(stages == 1 || (workspace && workspace_bytes >= need), "once_eval: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  OeArgs A;
  A.F = n_frames; A.C = n_classes; A.B = n_bands; A.K = n_combos; A.NG = host_gt_off[n_frames]; A.ND = host_pred_off[n_frames];
  A.mode = difficulty_mode; A.npp = num_pr_points; A.heading = with_heading ? 1 : 0;
  A.gt_off = gt_off; A.pd_off = pred_off; A.pair_off = pair_off; A.gt_box = gt_box; A.pd_box = pred_box; A.pd_score = pred_score;
  A.gt_code = gt_code; A.pd_code = pred_code; A.accept = accept; A.iou_thr = iou_threshold; A.flag_gt = flag_gt; A.flag_pd = flag_pred;
  const int wg_combos = gd_div_up(n_combos, 256 / GD_WAVE);
  if (stages == 1) {
    hipLaunchKernelGGL(k_oe_overlaps, dim3(n_frames), dim3(256), 0, st, A, overlaps, flag_gt, flag_pred);
    GD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_oe_match1, dim3(n_frames, wg_combos), dim3(256), 0, st, A, (const float*)overlaps, matched);
    GD_LAUNCH_CHECK();
    return 0;
  }
  const int n_chunks = gd_div_up(n_frames, kOeFrames);
  int* part = (int*)workspace;
  hipLaunchKernelGGL(k_oe_thresholds, dim3(n_combos), dim3(GD_WAVE), 0, st, A, sorted_scores, num_valid, thresholds, n_thresholds);
  GD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_oe_match2, dim3(n_chunks, wg_combos), dim3(256), 0, st, A, (const float*)overlaps, (const float*)thresholds,
                     (const int*)n_thresholds, part);
  GD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_oe_reduce, dim3(gd_div_up(n_combos * kOePts, 256)), dim3(256), 0, st, n_chunks, n_combos, (const int*)part, counts);
  GD_LAUNCH_CHECK();
  return 0;
}
