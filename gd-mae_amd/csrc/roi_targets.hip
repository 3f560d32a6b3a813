// Proposal targets of the second stage for the whole batch (reference ProposalTargetLayer, target_assigner/proposal_target_layer.py:13-230,
// and RoIHeadTemplate.assign_targets, roi_head_template.py:104-127).  The reference loops over the samples and the classes with mask
// gathers, nonzero, .item() and host-drawn permutations between the device calls; here the host draws its uniform numbers up front
// (u_fg per RoI, u_bg per output slot) and two launches decide everything on the device, without a host read.
//   k_rt_match   one wavefront per RoI: the lanes stride the sample's valid GT rows, skip the rows of other classes (by_class), give
//                overlap 0 to pairs whose centres are further apart than the two half-diagonals (+ slack: bev_overlap is exactly 0 there)
//                and reduce (largest IoU, lowest row) by wave64 shuffles.  IoU = the operations of boxes_iou3d_gpu on bev_overlap.
//   k_rt_sample  one 256-thread workgroup per sample: fg / hard / easy lists in RoI order by a packed block scan, the fg selection as a
//                bitonic sort of (u_fg bits, RoI index) keys in LDS, then one thread per output slot draws its RoI and writes its row of
//                every output (copied rows, labels, GT in the RoI's canonical frame).
// Keys are unique (the RoI index is in them) and there are no atomics: the result does not depend on scheduling.
#include "iou3d_rows.h"

namespace {
constexpr int kRtMax = 1024;      // RoIs, GT rows and output slots per sample (LDS lists, 10-bit counters)

struct RtThresh {
  float reg_fg, cls_fg, cls_bg, cls_bg_lo;
};

__global__ __launch_bounds__(256) void k_rt_match(const float* __restrict__ rois, const int* __restrict__ labels, const float* __restrict__ gt, int M,
                                                  int G, int by_class, float* __restrict__ iou_out, int* __restrict__ row_out) {
  const int b = blockIdx.y, lane = threadIdx.x & (GD_WAVE - 1);
  const int r = blockIdx.x * (256 / GD_WAVE) + (threadIdx.x / GD_WAVE);
  if (r >= M) return;                                        // whole wavefronts leave together (r is per wavefront)
  const float* g0 = gt + (size_t)b * G * 8;
  const int nv = rt_valid_rows(g0, G, lane);
  float box[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) box[c] = rois[((size_t)b * M + r) * 7 + c];
  const int lab = labels[(size_t)b * M + r];
  float best = 0.f;                                          // max_overlaps starts at 0
  int row = kRtMax;                                          // no row of the RoI's class seen yet
  for (int g = lane; g < nv; g += GD_WAVE) {
    const float* q = g0 + (size_t)g * 8;
    if (by_class && (int)q[7] != lab) continue;   // .long() of the label column
    float gb[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) gb[c] = q[c];
    const float v = rt_iou3d(box, gb);
    if (row == kRtMax || v > best) { best = v; row = g; }     // rows ascend within a lane: a tie keeps the lower row
  }
#pragma unroll
  for (int d = GD_WAVE / 2; d > 0; d >>= 1) {
    const float ob = __shfl_xor(best, d, GD_WAVE);
    const int orow = __shfl_xor(row, d, GD_WAVE);
    if (ob > best || (ob == best && orow < row)) { best = ob; row = orow; }
  }
  if (lane == 0) {
    iou_out[(size_t)b * M + r] = (row == kRtMax) ? 0.f : best;
    row_out[(size_t)b * M + r] = (row == kRtMax) ? 0 : row;   // a class without GT: row 0, overlap 0
  }
}

__device__ inline float rt_limit_period(float v, float period) { return v - floorf(v / period + 0.5f) * period; }
// list element of a uniform number: min(int(u n), n - 1), the product in fp32; u outside [0, 1) cannot leave the list
__device__ inline int rt_draw(float u, int n) { return max(min((int)(u * (float)n), n - 1), 0); }

struct RtOut {
  float* rois;        // (B, R, 7)
  float* scores;      // (B, R)
  int* labels;        // (B, R)
  int* indices;       // (B, R)
  float* iou;         // (B, R)
  float* gt_src;      // (B, R, 8)
  float* gt_ct;       // (B, R, 8)
  int* reg_valid;     // (B, R)
  float* cls_labels;  // (B, R)
};

__global__ __launch_bounds__(256) void k_rt_sample(const float* __restrict__ rois, const float* __restrict__ scores, const int* __restrict__ labels,
                                                   const float* __restrict__ gt, const float* __restrict__ u_fg, const float* __restrict__ u_bg,
                                                   const int* __restrict__ hard_quota, const float* __restrict__ iou, const int* __restrict__ row,
                                                   int M, int G, int N, int R, int fg_per_image, RtThresh T, int cls_type, RtOut O) {
  __shared__ unsigned long long keys[kRtMax];
  __shared__ unsigned short l_fg[kRtMax], l_hard[kRtMax], l_easy[kRtMax];
  __shared__ unsigned long long s_scan[256 / GD_WAVE + 1];
  const int b = blockIdx.x, t = threadIdx.x;
  const size_t base = (size_t)b * M;
  const float fg_thresh = fminf(T.reg_fg, T.cls_fg);
  // ---- the three lists in RoI order: counters packed 21 bits apart, one block scan per 256 RoIs
  unsigned long long carry = 0ull;
  for (int i0 = 0; i0 < N; i0 += 256) {
    const int i = i0 + t;
    unsigned long long flag = 0ull, key = ~0ull;
    bool fg = false, hard = false, easy = false;
    if (i < M) {
      const float v = iou[base + i];
      fg = v >= fg_thresh;
      easy = v < T.cls_bg_lo;
      hard = v < T.reg_fg && v >= T.cls_bg_lo;
      flag = (fg ? 1ull : 0ull) | (hard ? 1ull << 21 : 0ull) | (easy ? 1ull << 42 : 0ull);
      if (fg) key = ((unsigned long long)__float_as_uint(u_fg[base + i]) << 32) | (unsigned long long)i;   // u >= 0: the bits order like the value
    }
    keys[i] = key;
    unsigned long long tot;
    const unsigned long long ex = carry + gd_block_exclusive_scan<unsigned long long, 256>(flag, tot, s_scan);
    if (fg) l_fg[ex & 0x1FFFFF] = (unsigned short)i;
    if (hard) l_hard[(ex >> 21) & 0x1FFFFF] = (unsigned short)i;
    if (easy) l_easy[(ex >> 42) & 0x1FFFFF] = (unsigned short)i;
    carry += tot;
  }
  const int n_fg = (int)(carry & 0x1FFFFF), n_hard = (int)((carry >> 21) & 0x1FFFFF), n_easy = (int)((carry >> 42) & 0x1FFFFF);
  __syncthreads();
  // ---- fg without replacement: ascending (key, index); bitonic sort of N (power of two >= M) keys
  for (int k = 2; k <= N; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = t; p < (N >> 1); p += 256) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const int l = i + j;
        const unsigned long long x = keys[i], y = keys[l];
        const bool up = (i & k) == 0;
        if ((x > y) == up) { keys[i] = y; keys[l] = x; }
      }
      __syncthreads();
    }
  const int n_bg = n_hard + n_easy;
  const int f = (n_bg == 0) ? 0 : min(fg_per_image, n_fg);            // slots filled without replacement
  const int nb = R - f;
  int h = 0;                                                            // bg slots f .. f + h - 1 draw from the hard list
  if (n_hard > 0 && n_easy > 0) h = min(hard_quota[nb], n_hard);
  else if (n_hard > 0) h = nb;
  const float* gt_b = gt + (size_t)b * G * 8;
  for (int j = t; j < R; j += 256) {
    const float u = u_bg[(size_t)b * R + j];
    int src;
    if (j < f) {
      src = (int)(keys[j] & 0xFFFFFFFFull);
    } else if (n_bg == 0) {
      src = (n_fg > 0) ? l_fg[rt_draw(u, n_fg)] : 0;      // n_fg == 0 too: only with NaN overlaps; RoI 0
    } else if (j - f < h) {
      src = l_hard[rt_draw(u, n_hard)];
    } else {
      src = l_easy[rt_draw(u, n_easy)];
    }
    const size_t o = (size_t)b * R + j;
    float roi[7], g[8];
#pragma unroll
    for (int c = 0; c < 7; ++c) { roi[c] = rois[(base + src) * 7 + c]; O.rois[o * 7 + c] = roi[c]; }
    const float v = iou[base + src];
    const float* q = gt_b + (size_t)row[base + src] * 8;
#pragma unroll
    for (int c = 0; c < 8; ++c) { g[c] = q[c]; O.gt_src[o * 8 + c] = g[c]; }
    O.scores[o] = scores[base + src];
    O.labels[o] = labels[base + src];
    O.indices[o] = src;
    O.iou[o] = v;
    O.reg_valid[o] = v > T.reg_fg ? 1 : 0;
    float cl;
    if (cls_type == 1) {                                               // 'cls': 1 / 0, -1 strictly between the two thresholds
      cl = v > T.cls_fg ? 1.f : 0.f;
      if (v > T.cls_bg && v < T.cls_fg) cl = -1.f;
    } else {                                                           // 'roi_iou'
      cl = v > T.cls_fg ? 1.f : (v < T.cls_bg ? 0.f : (v - T.cls_bg) / (T.cls_fg - T.cls_bg));
    }
    O.cls_labels[o] = cl;
    // canonical frame of the RoI (assign_targets): shift, heading relative to the RoI's wrapped heading, rotate by -heading, wrap to pi
    const float ry = rt_limit_period(roi[6], 6.283185307179586f);
    const float x = g[0] - roi[0], y = g[1] - roi[1], z = g[2] - roi[2];
    const float hd = g[6] - ry;
    const float ca = cosf(-ry), sa = sinf(-ry);
    O.gt_ct[o * 8 + 0] = x * ca + y * (-sa);
    O.gt_ct[o * 8 + 1] = x * sa + y * ca;
    O.gt_ct[o * 8 + 2] = z;
    O.gt_ct[o * 8 + 3] = g[3];
    O.gt_ct[o * 8 + 4] = g[4];
    O.gt_ct[o * 8 + 5] = g[5];
    O.gt_ct[o * 8 + 6] = rt_limit_period(hd, 3.141592653589793f);
    O.gt_ct[o * 8 + 7] = g[7];
  }
}
}  // namespace

extern "C" size_t gdmae_roi_targets_workspace_bytes(int batch, int n_rois) {
  const size_t n = (size_t)(batch > 0 ? batch : 0) * (size_t)(n_rois > 0 ? n_rois : 0);
  return gd_align(n * sizeof(float)) + gd_align(n * sizeof(int));
}

extern "C" int gdmae_roi_targets(const float* rois, const float* roi_scores, const int* roi_labels, int batch, int n_rois, int roi_cols,
                                 const float* gt_boxes, int n_gt, const float* u_fg, const float* u_bg, const int* hard_quota,
                                 int rois_per_image, int fg_per_image, float reg_fg_thresh, float cls_fg_thresh, float cls_bg_thresh,
                                 float cls_bg_thresh_lo, int by_class, int cls_score_type, float* out_rois, float* out_roi_scores,
                                 int* out_roi_labels, int* out_roi_indices, float* out_gt_iou, float* out_gt_src, float* out_gt_of_rois,
                                 int* out_reg_valid, float* out_cls_labels, void* workspace, size_t workspace_bytes, void* stream) {
  GD_REQUIRE(roi_cols == 7, "roi_targets: RoIs of 7 columns only");
  GD_REQUIRE(n_rois >= 1 && n_rois <= kRtMax, "roi_targets: 1 .. 1024 RoIs per sample (the lists and the sort live in LDS)");
  GD_REQUIRE(n_gt >= 1 && n_gt <= kRtMax, "roi_targets: 1 .. 1024 GT rows per sample");
  GD_REQUIRE(rois_per_image >= 1 && rois_per_image <= kRtMax, "roi_targets: 1 .. 1024 RoIs sampled per sample (ROI_PER_IMAGE)");
  GD_REQUIRE(fg_per_image >= 0 && fg_per_image <= rois_per_image, "roi_targets: fg_per_image outside 0 .. ROI_PER_IMAGE");
  GD_REQUIRE(cls_score_type == 0 || cls_score_type == 1, "roi_targets: cls_score_type is 0 (roi_iou) or 1 (cls)");
  GD_REQUIRE(batch >= 0 && batch <= 65535, "roi_targets: batch outside 0 .. 65535");
  if (batch == 0) return 0;
  GD_REQUIRE(workspace_bytes >= gdmae_roi_targets_workspace_bytes(batch, n_rois), "roi_targets: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  GdArena A(workspace, workspace_bytes);
  float* iou = A.take<float>((size_t)batch * n_rois);
  int* row = A.take<int>((size_t)batch * n_rois);
  hipLaunchKernelGGL(k_rt_match, dim3(gd_div_up(n_rois, 256 / GD_WAVE), batch), dim3(256), 0, st, rois, roi_labels, gt_boxes, n_rois, n_gt,
                     by_class ? 1 : 0, iou, row);
  GD_LAUNCH_CHECK();
  int N = 256;                                   // every thread of the scan loop owns a key slot
  while (N < n_rois) N <<= 1;
  const RtThresh T{reg_fg_thresh, cls_fg_thresh, cls_bg_thresh, cls_bg_thresh_lo};
  const RtOut O{out_rois, out_roi_scores, out_roi_labels, out_roi_indices, out_gt_iou, out_gt_src, out_gt_of_rois, out_reg_valid, out_cls_labels};
  hipLaunchKernelGGL(k_rt_sample, dim3(batch), dim3(256), 0, st, rois, roi_scores, roi_labels, gt_boxes, u_fg, u_bg, hard_quota, iou, row, n_rois,
                     n_gt, N, rois_per_image, fg_per_image, T, cls_score_type, O);
  GD_LAUNCH_CHECK();
  return 0;
}
