// Rotated bird's-eye-view overlap / IoU and rotated NMS for the evaluation side of the fine-tune detector (SURVEY next
// row f4; reference pcdet/ops/iou3d_nms/src/iou3d_nms_kernel.cu:236-414 `boxes_overlap_kernel`, `boxes_iou_bev_kernel`,
// `nms_kernel`, `nms_normal_kernel`, and the host loop of iou3d_nms.cpp that walks the suppression masks).
//
// Overlap of two rotated rectangles, as the reference defines it: the intersection polygon is assembled from (a) the proper
// crossings of the 4 x 4 edge pairs and (b) the corners of either box that lie inside the other one WITH A 1e-2 MARGIN
// (so boxes that merely touch within a centimetre already report a sliver of overlap); the points are ordered by angle
// around their centroid and the area is the shoelace sum.  fp32 throughout, like the reference.
//
// Stated plainly: the device helpers of bev_iou.h (cross3, box_corners, inside_with_margin, seg_cross, bev_overlap) RESTATE
// iou3d_nms_kernel.cu:38-235 operation by operation - same intermediate quantities, same order of the fp32 operations, the same
// angular sort.  That is deliberate and it is the parity contract of this file: evaluation numbers (which box survives NMS at a
// threshold, an IoU that lands on either side of a matching threshold) depend on the last bits of this arithmetic and on the
// 1e-2 margin rule, so a geometrically equivalent formulation (e.g. Sutherland-Hodgman clipping) would NOT reproduce them.  What
// is pinned, and how: closed-form intersection areas (tests/test_iou3d_nms.py KNOWN_OVERLAPS: axis-aligned, 90 / 45 degree
// turns, containment, a corner triangle, disjoint) for both the CPU restatement (oracle/iou3d_oracle.py) and these kernels, an
// independent exact float64 clipping away from the margin cases, and kernel == oracle to 2e-5 on random boxes.  The reference
// holds no vectors for it and its CPU twin does not compile here (<cuda.h>), so "matches the reference's own output" stays
// unpinned.  The NMS half (mask words + a one-wavefront device scan, no host round trip) is this build's own design.
//
// NMS: boxes arrive sorted by score.  k_nms_masks: one thread per (box i, 64-box column block) builds the 64-bit word of
// the later boxes j > i with IoU > threshold; k_nms_scan: ONE wavefront walks the boxes in order with the "removed" bit set
// in LDS (lane = one 64-bit word of the row being OR-ed in) and writes the kept indices and their count - the reference
// copies the masks to the host and scans them there; here nothing leaves the device.
#include "bev_iou.h"

namespace {

// mode 0: overlap area, 1: IoU
__global__ __launch_bounds__(256) void k_bev_pairs(const float* __restrict__ A, int n, const float* __restrict__ B, int m, int mode,
                                                   float* __restrict__ out) {
  const long long total = (long long)n * m;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const float* a = A + (i / m) * 7;
    const float* b = B + (i % m) * 7;
    out[i] = mode ? bev_iou(a, b) : bev_overlap(a, b);
  }
}

// mask[i][cb] bit j: box (64 cb + j) > i overlaps box i beyond the threshold
__global__ __launch_bounds__(64) void k_nms_masks(const float* __restrict__ boxes, int n, float thresh, int rotated,
                                                  unsigned long long* __restrict__ mask, int words) {
  __shared__ float cols[64 * 7];
  const int rb = blockIdx.y, cb = blockIdx.x, t = threadIdx.x;
  const int cn = min(64, n - cb * 64), rn = min(64, n - rb * 64);
  if (t < cn)
    for (int e = 0; e < 7; ++e) cols[t * 7 + e] = boxes[(long long)(cb * 64 + t) * 7 + e];
  __syncthreads();
  if (t >= rn) return;
  const int i = rb * 64 + t;
  unsigned long long w = 0ull;
  if (cb >= rb) {
    const float* bi = boxes + (long long)i * 7;
    const int start = cb == rb ? t + 1 : 0;
    for (int j = start; j < cn; ++j) {
      const float v = rotated ? bev_iou(bi, cols + j * 7) : axis_iou(bi, cols + j * 7);
      if (v > thresh) w |= 1ull << j;
    }
  }
  mask[(long long)i * words + cb] = w;
}

// one wavefront: sequential scan in score order; removed bits live in LDS (words <= 4096 / 64 * ... = n / 64)
__global__ __launch_bounds__(64) void k_nms_scan(const unsigned long long* __restrict__ mask, int n, int words, long long* __restrict__ keep,
                                                 int* __restrict__ n_keep) {
  extern __shared__ unsigned long long removed[];
  const int lane = threadIdx.x;
  for (int w = lane; w < words; w += 64) removed[w] = 0ull;
  __syncthreads();
  int cnt = 0;
  for (int i = 0; i < n; ++i) {
    const bool dead = (removed[i >> 6] >> (i & 63)) & 1ull;     // uniform across the wavefront
    if (!dead) {
      if (lane == 0) keep[cnt] = i;
      ++cnt;
      for (int w = lane; w < words; w += 64) removed[w] |= mask[(long long)i * words + w];
    }
    __syncthreads();
  }
  if (lane == 0) *n_keep = cnt;
}
}  // namespace

// boxes (n, 7) / (m, 7) fp32 device [x, y, z, dx, dy, dz, heading]; out (n, m): mode 0 = BEV overlap area, 1 = BEV IoU
extern "C" int gdmae_boxes_bev_pairs(const float* boxes_a, int n, const float* boxes_b, int m, int mode, float* out, void* stream) {
  if (n <= 0 || m <= 0) return 0;
  long long g = ((long long)n * m + 255) / 256;
  if (g > 65535) g = 65535;
  hipLaunchKernelGGL(k_bev_pairs, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, boxes_a, n, boxes_b, m, mode, out);
  GD_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t gdmae_nms_workspace_bytes(int n) {
  const size_t words = (size_t)(n + 63) / 64;
  return gd_align((size_t)(n > 0 ? n : 1) * words * sizeof(unsigned long long));
}

// boxes (n, 7) sorted by descending score; keep (n) int64 receives the kept indices in order, n_keep (device int) their count.
// rotated: 1 = rotated BEV IoU (reference nms_gpu), 0 = axis-aligned IoU ignoring the heading (reference nms_normal_gpu).
extern "C" int gdmae_nms_bev(const float* boxes, int n, float thresh, int rotated, long long* keep, int* n_keep, void* workspace,
                             void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (n <= 0) {
    GD_CHECK(hipMemsetAsync(n_keep, 0, sizeof(int), st));
    return 0;
  }
  const int words = (n + 63) / 64;
  GD_REQUIRE((size_t)words * 8 <= 60 * 1024, "nms_bev: too many boxes for the in-LDS bit set");
  unsigned long long* mask = (unsigned long long*)workspace;
  hipLaunchKernelGGL(k_nms_masks, dim3(words, words), dim3(64), 0, st, boxes, n, thresh, rotated, mask, words);
  GD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_nms_scan, dim3(1), dim3(64), (size_t)words * 8, st, (const unsigned long long*)mask, n, words, keep, n_keep);
  GD_LAUNCH_CHECK();
  return 0;
}
