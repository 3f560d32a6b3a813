// Recall record of an evaluation step for the whole batch (reference Detector3DTemplate.generate_recall_record,
// detector3d_template.py:318-358): how many GT boxes have a predicted box (and a RoI) with 3-D IoU above each threshold.  The reference
// trims the GT rows with nonzero + int(), builds two pair matrices per sample and reads two counts per threshold on the host; here two
// launches add to a device record that is never read here.  The mirror image of k_rt_match (roi_targets.hip).
//   k_rr_best    one wavefront per (GT row, sample): the lanes agree on the sample's valid-row count, stride the predicted rows and the
//                RoI rows, give overlap 0 to pairs whose centres are further apart than the two half-diagonals (+ slack: bev_overlap is
//                exactly 0 there) and reduce the largest IoU by wave64 shuffles.  IoU = the operations of boxes_iou3d_gpu(pred, gt).
//   k_rr_count   one workgroup: a wavefront per sample in turn counts its valid rows and the rows above each threshold, the four
//                wavefronts meet in LDS and one thread per counter adds its figure (stream order makes the read-modify-write safe).
// No atomics: the result does not depend on scheduling.
#include "iou3d_rows.h"

namespace {
constexpr int kRrMaxT = 8;

struct RrThresh {
  float t[kRrMaxT];
};

// largest IoU of box b (as the second argument) over rows 0 .. n - 1 of a (n, cols) table; every lane returns the wavefront's maximum
__device__ inline float rr_best(const float* __restrict__ rows, int n, int cols, const float* gb, int lane) {
  float best = 0.f;                                          // IoU >= 0: "none" and "no overlap" are both 0
  for (int p = lane; p < n; p += GD_WAVE) {
    const float* q = rows + (size_t)p * cols;
    float pb[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) pb[c] = q[c];
    const float v = rt_iou3d(pb, gb);
    if (v > best) best = v;
  }
#pragma unroll
  for (int d = GD_WAVE / 2; d > 0; d >>= 1) best = fmaxf(best, __shfl_xor(best, d, GD_WAVE));
  return best;
}

__device__ inline int rr_rows(const int* __restrict__ num, int b, int n) { return num ? min(max(num[b], 0), n) : n; }

__global__ __launch_bounds__(256) void k_rr_best(const float* __restrict__ pred, const int* __restrict__ pred_num, int n, int pred_cols,
                                                 const float* __restrict__ rois, const int* __restrict__ roi_num, int M, int roi_cols,
                                                 const float* __restrict__ gt, int G, int gt_cols, float* __restrict__ best_iou) {
  const int b = blockIdx.y, lane = threadIdx.x & (GD_WAVE - 1);
  const int g = blockIdx.x * (256 / GD_WAVE) + (threadIdx.x / GD_WAVE);
  if (g >= G) return;                                        // whole wavefronts leave together (g is per wavefront)
  const float* g0 = gt + (size_t)b * G * gt_cols;
  const int nv = rt_last_nonzero_row(g0, G, gt_cols, lane) + 1;
  float v_roi = 0.f, v_pred = 0.f;
  if (g < nv) {                                              // uniform in the wavefront
    float gb[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) gb[c] = g0[(size_t)g * gt_cols + c];
    v_pred = rr_best(pred + (size_t)b * n * pred_cols, rr_rows(pred_num, b, n), pred_cols, gb, lane);
    if (rois) v_roi = rr_best(rois + (size_t)b * M * roi_cols, rr_rows(roi_num, b, M), roi_cols, gb, lane);
  }
  if (lane == 0) {
    best_iou[((size_t)b * G + g) * 2 + 0] = v_roi;
    best_iou[((size_t)b * G + g) * 2 + 1] = v_pred;
  }
}

__global__ __launch_bounds__(256) void k_rr_count(const float* __restrict__ gt, int B, int G, int gt_cols, const float* __restrict__ best_iou,
                                                  int with_rois, int T, RrThresh th, long long* __restrict__ counters) {
  constexpr int kWaves = 256 / GD_WAVE;
  __shared__ int s_cnt[kWaves][1 + 2 * kRrMaxT];
  const int lane = threadIdx.x & (GD_WAVE - 1), w = threadIdx.x / GD_WAVE;
  int cnt[1 + 2 * kRrMaxT];
#pragma unroll
  for (int i = 0; i < 1 + 2 * kRrMaxT; ++i) cnt[i] = 0;
  for (int b = w; b < B; b += kWaves) {
    const int nv = rt_last_nonzero_row(gt + (size_t)b * G * gt_cols, G, gt_cols, lane) + 1;
    if (lane == 0) cnt[0] += nv;
    for (int g = lane; g < nv; g += GD_WAVE) {
      const float v_roi = best_iou[((size_t)b * G + g) * 2 + 0], v_pred = best_iou[((size_t)b * G + g) * 2 + 1];
#pragma unroll
      for (int i = 0; i < kRrMaxT; ++i)
        if (i < T) {
          if (with_rois && v_roi > th.t[i]) cnt[1 + i] += 1;
          if (v_pred > th.t[i]) cnt[1 + kRrMaxT + i] += 1;
        }
    }
  }
#pragma unroll
  for (int i = 0; i < 1 + 2 * kRrMaxT; ++i) {
    int v = cnt[i];
#pragma unroll
    for (int d = GD_WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, GD_WAVE);
    if (lane == 0) s_cnt[w][i] = v;
  }
  __syncthreads();
  const int i = threadIdx.x;
  if (i < 1 + 2 * T) {
    const int src = (i == 0) ? 0 : (i <= T ? i : 1 + kRrMaxT + (i - 1 - T));      // [gt_num, roi_t.., rcnn_t..]
    long long s = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) s += s_cnt[k][src];
    counters[i] += s;
  }
}
}  // namespace

extern "C" int gdmae_recall_record(const float* pred_boxes, const int* pred_num, int batch, int n_pred, int pred_cols, const float* rois,
                                   const int* roi_num, int n_rois, int roi_cols, const float* gt_boxes, int n_gt, int gt_cols,
                                   const float* thresholds, int n_thresh, long long* counters, float* best_iou, void* stream) {
  GD_REQUIRE(n_thresh >= 1 && n_thresh <= kRrMaxT, "recall_record: 1 .. 8 thresholds");
  GD_REQUIRE(batch >= 0 && n_pred >= 0 && n_rois >= 0 && n_gt >= 0, "recall_record: negative batch, predicted-row, RoI-row or GT-row count");
  GD_REQUIRE(batch <= 65535, "recall_record: batch outside 0 .. 65535");
  GD_REQUIRE(pred_cols >= 7 && roi_cols >= 7 && gt_cols >= 7, "recall_record: predicted boxes, RoIs and GT boxes of at least 7 columns");
  if (batch == 0 || n_gt == 0) return 0;                     // no GT row: nothing to add, best_iou has no entry
  hipStream_t st = (hipStream_t)stream;
  RrThresh th;
  for (int i = 0; i < kRrMaxT; ++i) th.t[i] = i < n_thresh ? thresholds[i] : 0.f;
  hipLaunchKernelGGL(k_rr_best, dim3(gd_div_up(n_gt, 256 / GD_WAVE), batch), dim3(256), 0, st, pred_boxes, pred_num, n_pred, pred_cols, rois,
                     roi_num, rois ? n_rois : 0, roi_cols, gt_boxes, n_gt, gt_cols, best_iou);
  GD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_rr_count, dim3(1), dim3(256), 0, st, gt_boxes, batch, n_gt, gt_cols, best_iou, rois ? 1 : 0, n_thresh, th, counters);
  GD_LAUNCH_CHECK();
  return 0;
}
