// Anchor head of the KITTI fine-tune config on the GPU (reference pcdet/models/dense_heads/anchor_head_template.py:88-266,
// target_assigner/axis_aligned_target_assigner.py:36-210, utils/box_utils.py:249-298, utils/box_coder_utils.py:14-78,
// utils/loss_utils.py:10-140 / 213-238, model_utils/model_nms_utils.py:6-25).
//
// The reference assigns targets in a Python loop over samples x anchor classes (~25 small launches and several host reads per
// iteration, 48 iterations at the config's batch of 16) and evaluates the three losses as ~60 elementwise passes over
// (B, 321408, .) tensors.  Here:
//   gdmae_anchor_targets   3 launches for all samples and classes: k_ah_prepare (per (sample, class): ordered compaction of the
//                          class's ground-truth boxes + their nearest axis-aligned rectangles), k_ah_colmax (best IoU per ground
//                          truth: LDS maxima per workgroup, then an atomic max on the bit patterns - IoU >= 0, so integer order is
//                          float order and the result does not depend on arrival order), k_ah_assign (labels, matched box,
//                          regression targets, direction bins, positive counts).
//   gdmae_anchor_loss_fwd  focal + smooth-L1 + direction cross-entropy in ONE pass over the head's output rows, per-workgroup
//                          partials finished in a fixed order (bit-repeatable); gdmae_anchor_loss_bwd writes the whole gradient row.
//   gdmae_anchor_decode    ResidualCoder.decode + direction-bin correction for all B x A anchors in one launch.
//   gdmae_anchor_select    best-class sigmoid score / label per anchor and an ordered compaction of the anchors at or above the
//                          score threshold: one workgroup per sample scans its anchors in order (deterministic output).
// Anchor geometry comes from small tables filled from the generated anchor tensor (the framework path's bits), not 7 floats per
// anchor.  The IoU arithmetic restates box_utils.py:249-269 operation by operation; the build has -ffp-contract=off.
// Anchor index: a = (y * W + x) * K + k, k = the anchor slot of a location (class-major, then size, then rotation).
#include "anchor_decode.h"
#include "common.h"

namespace {
constexpr int kMaxGt = 512;       // ground-truth rows per sample the LDS copies are sized for
constexpr int kMaxCls = 8;
constexpr int kMaxSlots = 32;
constexpr int kMaxBins = 8;

__device__ __forceinline__ float ah_iou(float ax1, float ay1, float ax2, float ay2, float area_a, float4 g, float area_g) {
  const float x_min = fmaxf(ax1, g.x), x_max = fminf(ax2, g.z);
  const float y_min = fmaxf(ay1, g.y), y_max = fminf(ay2, g.w);
  const float x_len = fmaxf(x_max - x_min, 0.f), y_len = fmaxf(y_max - y_min, 0.f);
  const float inter = x_len * y_len;
  return inter / fmaxf(area_a + area_g - inter, 1e-6f);
}

// workspace layout as ah_ws() places it (not the field order of AhWs): rect[B][n_cls][n_max] float4 | row[B][n_cls][n_max] int | cls[..] int | colmax[..] uint | n_gt[B][n_cls] int
struct AhWs {
  int* n_gt;
  float4* rect;
  int* row;
  int* cls;
  unsigned* colmax;
};
__host__ __device__ inline AhWs ah_ws(void* ws, int B, int n_cls, int n_max) {
  AhWs w;
  char* p = (char*)ws;
  w.rect = (float4*)p; p += (size_t)B * n_cls * n_max * sizeof(float4);
  w.row = (int*)p; p += (size_t)B * n_cls * n_max * sizeof(int);
  w.cls = (int*)p; p += (size_t)B * n_cls * n_max * sizeof(int);
  w.colmax = (unsigned*)p; p += (size_t)B * n_cls * n_max * sizeof(unsigned);
  w.n_gt = (int*)p;
  return w;
}

struct AhNames { int idx[kMaxCls]; };     // anchor class -> index of its name in the detector's class list (-1: not there)

// one wave per (sample, anchor class)
__global__ __launch_bounds__(64) void k_ah_prepare(const float* __restrict__ gt, int n_max, int box_dim, int n_cls, int n_names, AhNames names,
                                                   AhWs w, int* __restrict__ npos) {
  const int b = blockIdx.x / n_cls, c = blockIdx.x % n_cls, lane = threadIdx.x;
  const float* g = gt + (long long)b * n_max * box_dim;
  if (c == 0 && lane == 0) npos[b] = 0;
  // trailing rows whose box sums to zero are padding; row 0 always stays (axis_aligned_target_assigner.py:53-57)
  int last = 0;
  for (int i = lane; i < n_max; i += 64) {
    float s = 0.f;
    for (int e = 0; e < box_dim - 1; ++e) s += g[(long long)i * box_dim + e];
    if (s != 0.f) last = i;
  }
  for (int d = 32; d > 0; d >>= 1) last = max(last, __shfl_xor(last, d));
  const long long o = ((long long)b * n_cls + c) * n_max;
  int base = 0;
  for (int i0 = 0; i0 <= last; i0 += 64) {
    const int i = i0 + lane;
    bool own = false;
    int cv = 0;
    if (i <= last) {
      cv = (int)g[(long long)i * box_dim + box_dim - 1];
      // class value cv names class_names[cv - 1] with Python's negative indexing: 0 selects the last name
      if (cv >= 0 && cv <= n_names) own = ((cv - 1 + n_names) % n_names) == names.idx[c];
    }
    const unsigned long long m = __ballot(own);
    const int k = base + __popcll(m & ((1ull << lane) - 1ull));
    base += __popcll(m);
    if (own) {
      const float* bx = g + (long long)i * box_dim;
      const float pi = 3.14159265358979323846f;
      const float rot = fabsf(ah_limit_period(bx[6], 0.5f, pi));
      const bool keep = rot < 0.78539816339744830962f;
      const float dx = keep ? bx[3] : bx[4], dy = keep ? bx[4] : bx[3];
      w.rect[o + k] = make_float4(bx[0] - dx / 2.f, bx[1] - dy / 2.f, bx[0] + dx / 2.f, bx[1] + dy / 2.f);
      w.row[o + k] = i;
      w.cls[o + k] = cv;
      w.colmax[o + k] = 0u;
    }
  }
  if (lane == 0) w.n_gt[b * n_cls + c] = base;
}

struct AhGeom {
  int H, W, K, n_cls, n_max;
  const int* slot_cls;      // (K)
  const float* xr;          // (K, W, 2) x1, x2
  const float* yr;          // (K, H, 2) y1, y2
  const float* xc;          // (W)
  const float* yc;          // (H)
  const float* slot;        // (K, 5) z, dx, dy, dz, rotation
};

// grid (ceil(A / 256), B): best IoU of every ground truth over the anchors of its class
__global__ __launch_bounds__(256) void k_ah_colmax(AhGeom G, AhWs w) {
  __shared__ float4 s_rect[kMaxGt];
  __shared__ unsigned s_max[kMaxGt];
  __shared__ int s_off[kMaxCls + 1];
  const int b = blockIdx.y;
  if (threadIdx.x == 0) {
    int o = 0;
    for (int c = 0; c < G.n_cls; ++c) { s_off[c] = o; o += w.n_gt[b * G.n_cls + c]; }
    s_off[G.n_cls] = o;
  }
  __syncthreads();
  const int total = s_off[G.n_cls];
  if (total == 0) return;
  for (int c = 0; c < G.n_cls; ++c) {
    const long long o = ((long long)b * G.n_cls + c) * G.n_max;
    for (int i = threadIdx.x; i < s_off[c + 1] - s_off[c]; i += 256) { s_rect[s_off[c] + i] = w.rect[o + i]; s_max[s_off[c] + i] = 0u; }
  }
  __syncthreads();
  const long long A = (long long)G.H * G.W * G.K;
  const long long a = blockIdx.x * 256ll + threadIdx.x;
  if (a < A) {
    const int k = (int)(a % G.K);
    const long long loc = a / G.K;
    const int x = (int)(loc % G.W), y = (int)(loc / G.W);
    const int c = G.slot_cls[k];
    const float ax1 = G.xr[((long long)k * G.W + x) * 2], ax2 = G.xr[((long long)k * G.W + x) * 2 + 1];
    const float ay1 = G.yr[((long long)k * G.H + y) * 2], ay2 = G.yr[((long long)k * G.H + y) * 2 + 1];
    const float area_a = (ax2 - ax1) * (ay2 - ay1);
    for (int j = s_off[c]; j < s_off[c + 1]; ++j) {
      const float4 g = s_rect[j];
      const float iou = ah_iou(ax1, ay1, ax2, ay2, area_a, g, (g.z - g.x) * (g.w - g.y));
      if (iou > 0.f) atomicMax(&s_max[j], __float_as_uint(iou));
    }
  }
  __syncthreads();
  for (int c = 0; c < G.n_cls; ++c) {
    const long long o = ((long long)b * G.n_cls + c) * G.n_max;
    for (int i = threadIdx.x; i < s_off[c + 1] - s_off[c]; i += 256) {
      const unsigned v = s_max[s_off[c] + i];
      if (v) atomicMax(&w.colmax[o + i], v);
    }
  }
}

struct AhThr { float matched[kMaxCls], unmatched[kMaxCls]; };

__global__ __launch_bounds__(256) void k_ah_assign(AhGeom G, AhWs w, const float* __restrict__ gt, int gt_rows, int box_dim, AhThr T,
                                                   float dir_offset, int num_bins, int* __restrict__ labels, int* __restrict__ gt_ids,
                                                   float* __restrict__ reg, int* __restrict__ bins, int* __restrict__ npos) {
  __shared__ float4 s_rect[kMaxGt];
  __shared__ float s_max[kMaxGt];
  __shared__ int s_off[kMaxCls + 1];
  __shared__ int s_pos;
  const int b = blockIdx.y;
  if (threadIdx.x == 0) {
    int o = 0;
    for (int c = 0; c < G.n_cls; ++c) { s_off[c] = o; o += w.n_gt[b * G.n_cls + c]; }
    s_off[G.n_cls] = o;
    s_pos = 0;
  }
  __syncthreads();
  for (int c = 0; c < G.n_cls; ++c) {
    const long long o = ((long long)b * G.n_cls + c) * G.n_max;
    for (int i = threadIdx.x; i < s_off[c + 1] - s_off[c]; i += 256) {
      s_rect[s_off[c] + i] = w.rect[o + i];
      const float m = __uint_as_float(w.colmax[o + i]);
      s_max[s_off[c] + i] = m == 0.f ? -1.f : m;            // a ground truth no anchor overlaps force-matches nothing
    }
  }
  __syncthreads();
  const long long A = (long long)G.H * G.W * G.K;
  const long long a = blockIdx.x * 256ll + threadIdx.x;
  if (a < A) {
    const int k = (int)(a % G.K);
    const long long loc = a / G.K;
    const int x = (int)(loc % G.W), y = (int)(loc / G.W);
    const int c = G.slot_cls[k];
    const int j0 = s_off[c], n = s_off[c + 1] - s_off[c];
    int label = 0, gid = -1, bin = -1;
    float t[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (n > 0) {
      const float ax1 = G.xr[((long long)k * G.W + x) * 2], ax2 = G.xr[((long long)k * G.W + x) * 2 + 1];
      const float ay1 = G.yr[((long long)k * G.H + y) * 2], ay2 = G.yr[((long long)k * G.H + y) * 2 + 1];
      const float area_a = (ax2 - ax1) * (ay2 - ay1);
      float best = -1.f;
      int arg = 0;
      bool force = false;
      for (int j = 0; j < n; ++j) {
        const float4 g = s_rect[j0 + j];
        const float iou = ah_iou(ax1, ay1, ax2, ay2, area_a, g, (g.z - g.x) * (g.w - g.y));
        if (iou > best) { best = iou; arg = j; }             // ties: the lowest index (argmax on the CPU)
        force = force || iou == s_max[j0 + j];
      }
      const long long o = ((long long)b * G.n_cls + c) * G.n_max + arg;
      const int cls = w.cls[o];
      label = -1;
      if (force) { label = cls; gid = arg; }
      if (best >= T.matched[c]) { label = cls; gid = arg; }
      const bool fg = label > 0;                              // taken BEFORE the background pass, as the reference does
      if (best < T.unmatched[c]) label = 0;
      if (force) label = cls;
      if (fg) {
        const int row = w.row[o];
        gid = row;
        const float* bx = gt + ((long long)b * gt_rows + row) * box_dim;
        const float* s = G.slot + k * 5;
        const float xa = G.xc[x], ya = G.yc[y], za = s[0];
        const float dxa = fmaxf(s[1], 1e-5f), dya = fmaxf(s[2], 1e-5f), dza = fmaxf(s[3], 1e-5f), ra = s[4];
        const float dxg = fmaxf(bx[3], 1e-5f), dyg = fmaxf(bx[4], 1e-5f), dzg = fmaxf(bx[5], 1e-5f);
        const float diag = sqrtf(dxa * dxa + dya * dya);
        t[0] = (bx[0] - xa) / diag;
        t[1] = (bx[1] - ya) / diag;
        t[2] = (bx[2] - za) / dza;
        t[3] = logf(dxg / dxa); t[4] = logf(dyg / dya); t[5] = logf(dzg / dza);
        t[6] = bx[6] - ra;
        const float two_pi = 6.283185307179586f;
        const float off = ah_limit_period((t[6] + ra) - dir_offset, 0.f, two_pi);
        const float per = (float)(6.283185307179586 / (double)num_bins);
        bin = (int)floorf(off / per);
        bin = bin < 0 ? 0 : (bin > num_bins - 1 ? num_bins - 1 : bin);
      } else {
        gid = -1;
      }
    }
    labels[(long long)b * A + a] = label;
    gt_ids[(long long)b * A + a] = gid;
    bins[(long long)b * A + a] = bin;
    float* r = reg + ((long long)b * A + a) * 7;
#pragma unroll
    for (int e = 0; e < 7; ++e) r[e] = t[e];
    if (label > 0) atomicAdd(&s_pos, 1);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_pos) atomicAdd(&npos[b], s_pos);
}
}  // namespace

extern "C" size_t gdmae_anchor_targets_workspace_bytes(int B, int n_cls, int n_max) {
  const size_t per = (size_t)B * n_cls * (n_max < 1 ? 1 : n_max);
  return gd_align(per * (sizeof(float4) + 3 * sizeof(int)) + (size_t)B * n_cls * sizeof(int));
}

// gt_boxes (B, n_max, box_dim) fp32 device, class in the last column.  Tables (device): slot_cls (K) int, xr (K, W, 2), yr (K, H, 2),
// xc (W), yc (H), slot (K, 5).  Host arrays: name_idx (n_cls), matched / unmatched (n_cls).  Outputs (device, fully written):
// labels / gt_ids / dir_bins (B, A) int32, reg_targets (B, A, 7) fp32, num_pos (B) int32, A = H W K.
extern "C" int gdmae_anchor_targets(const float* gt_boxes, int B, int n_max, int box_dim, int H, int W, int K, int n_cls, int n_names,
                                    const int* name_idx, const int* slot_cls, const float* xr, const float* yr, const float* xc, const float* yc,
                                    const float* slot, const float* matched, const float* unmatched, float dir_offset, int num_bins,
                                    int* labels, int* gt_ids, float* reg_targets, int* dir_bins, int* num_pos, void* workspace, void* stream) {
  GD_REQUIRE(B >= 1 && n_max >= 1 && n_max <= kMaxGt && box_dim >= 8 && H >= 1 && W >= 1 && K >= 1 && K <= kMaxSlots && n_cls >= 1 &&
             n_cls <= kMaxCls && n_names >= 1 && num_bins >= 1 && num_bins <= kMaxBins, "anchor_targets: bad sizes (n_max <= 512, <= 8 classes)");
  for (int c = 0; c < n_cls; ++c)
    for (int d = 0; d < c; ++d)       // a ground-truth row then belongs to one anchor class at most: <= n_max rectangles per sample in LDS
      GD_REQUIRE(name_idx[c] < 0 || name_idx[c] != name_idx[d], "anchor_targets: two anchor classes with one class name");
  hipStream_t st = (hipStream_t)stream;
  AhWs w = ah_ws(workspace, B, n_cls, n_max);
  AhNames names;
  AhThr T;
  for (int c = 0; c < kMaxCls; ++c) {
    names.idx[c] = c < n_cls ? name_idx[c] : -1;
    T.matched[c] = c < n_cls ? matched[c] : 0.f;
    T.unmatched[c] = c < n_cls ? unmatched[c] : 0.f;
  }
  AhGeom G{H, W, K, n_cls, n_max, slot_cls, xr, yr, xc, yc, slot};
  const long long A = (long long)H * W * K;
  hipLaunchKernelGGL(k_ah_prepare, dim3(B * n_cls), dim3(64), 0, st, gt_boxes, n_max, box_dim, n_cls, n_names, names, w, num_pos);
  GD_LAUNCH_CHECK();
  const dim3 grid((unsigned)gd_div_up(A, 256), B);
  hipLaunchKernelGGL(k_ah_colmax, grid, dim3(256), 0, st, G, w);
  GD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ah_assign, grid, dim3(256), 0, st, G, w, gt_boxes, n_max, box_dim, T, dir_offset, num_bins, labels, gt_ids, reg_targets,
                     dir_bins, num_pos);
  GD_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Losses.  rows: (B * n_loc, ld) head output, columns [cls K*C | box K*7 | dir K*nb | padding], bf16 or fp32.
//   cls: sigmoid focal loss (alpha 0.25, gamma 2) x [label >= 0] / max(#pos_b, 1), one-hot target = label - 1 for label > 0
//   loc: smooth-L1 (beta 1/9) of code_weight * (pred - target), the angle as sin(pred) cos(tgt) - cos(pred) sin(tgt); positives only
//   dir: cross-entropy of the direction bins; positives only.          scale[3] = LOSS_WEIGHTS / B
// ------------------------------------------------------------------------------------------------
namespace {
struct AlArgs {
  const void* rows;
  int bf16, ld, B, n_loc, K, C, nb;
  const int* labels;
  const float* reg;
  const int* bins;
  const int* npos;
  float cw[7];
  float scale[3];
};
__device__ __forceinline__ float al_at(const AlArgs& A, long long o) {
  return A.bf16 ? __uint_as_float(((unsigned)((const unsigned short*)A.rows)[o]) << 16) : ((const float*)A.rows)[o];
}
constexpr float kBeta = (float)(1.0 / 9.0);
constexpr float kHalfBeta = (float)(0.5 * (1.0 / 9.0));

// one anchor: the three loss terms (already weighted by 1 / max(#pos, 1)), and with WANT_GRAD the 3 + 7 + nb gradients (unscaled by g)
template <bool WANT_GRAD>
__device__ __forceinline__ void al_anchor(const AlArgs& A, long long e, float* loss3, float* gc, float* gb, float* gd) {
  const long long per_b = (long long)A.n_loc * A.K;
  const int b = (int)(e / per_b);
  const long long site = e / A.K;                 // b * n_loc + loc
  const int k = (int)(e % A.K);
  const int label = A.labels[e];
  const int np = A.npos[b];
  const float wn = 1.f / fmaxf((float)np, 1.f);
  const long long r0 = site * A.ld;
  // classification
  const float wc = label >= 0 ? wn : 0.f;
  for (int c = 0; c < A.C; ++c) {
    if (WANT_GRAD) gc[c] = 0.f;
    if (label < 0) continue;
    const float x = al_at(A, r0 + k * A.C + c);
    const float t = (label > 0 && (A.C == 1 || c == label - 1)) ? 1.f : 0.f;
    const float p = 1.f / (1.f + expf(-x));
    const float aw = t * 0.25f + (1.f - t) * 0.75f;
    const float pt = t * (1.f - p) + (1.f - t) * p;
    const float bce = fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
    loss3[0] += aw * (pt * pt) * bce * wc;
    if (WANT_GRAD) {
      const float dpt = (1.f - 2.f * t) * p * (1.f - p);
      gc[c] = aw * (2.f * pt * dpt * bce + pt * pt * (p - t)) * wc;
    }
  }
  if (WANT_GRAD) {
#pragma unroll
    for (int i = 0; i < 7; ++i) gb[i] = 0.f;
    for (int d = 0; d < A.nb; ++d) gd[d] = 0.f;
  }
  if (label <= 0) return;
  // localisation
  const long long box0 = r0 + A.K * A.C + k * 7;
  const float* tg = A.reg + e * 7;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const float pr = al_at(A, box0 + i);
    float tv = tg[i];
    float pv = pr, dpv = 1.f;
    if (i == 6) {
      pv = sinf(pr) * cosf(tv);
      const float tv2 = cosf(pr) * sinf(tv);
      dpv = cosf(pr) * cosf(tv) + sinf(pr) * sinf(tv);
      tv = tv2;
    }
    if (tv != tv) continue;                        // NaN targets are ignored
    const float diff = (pv - tv) * A.cw[i];
    const float n = fabsf(diff);
    loss3[1] += (n < kBeta ? 0.5f * (n * n) / kBeta : n - kHalfBeta) * wn;
    if (WANT_GRAD) gb[i] = (n < kBeta ? diff / kBeta : (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f))) * A.cw[i] * dpv * wn;
  }
  // direction
  if (A.nb > 0) {
    const long long d0 = r0 + A.K * (A.C + 7) + k * A.nb;
    const int bin = A.bins[e];
    float v[kMaxBins], m = -INFINITY;
    for (int d = 0; d < A.nb; ++d) { v[d] = al_at(A, d0 + d); m = fmaxf(m, v[d]); }
    float s = 0.f;
    for (int d = 0; d < A.nb; ++d) s += expf(v[d] - m);
    const float lse = m + logf(s);
    if (bin >= 0 && bin < A.nb) {
      loss3[2] += (lse - v[bin]) * wn;
      if (WANT_GRAD)
        for (int d = 0; d < A.nb; ++d) gd[d] = (expf(v[d] - lse) - (d == bin ? 1.f : 0.f)) * wn;
    }
  }
}

__global__ __launch_bounds__(256) void k_al_fwd(AlArgs A, float* __restrict__ part) {
  const long long total = (long long)A.B * A.n_loc * A.K;
  float l[3] = {0.f, 0.f, 0.f};
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (long long)gridDim.x * 256) al_anchor<false>(A, e, l, nullptr, nullptr, nullptr);
  __shared__ float sh[3][256];
  sh[0][threadIdx.x] = l[0]; sh[1][threadIdx.x] = l[1]; sh[2][threadIdx.x] = l[2];
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) {
#pragma unroll
      for (int k = 0; k < 3; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + d];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) part[(long long)blockIdx.x * 3 + threadIdx.x] = sh[threadIdx.x][0];
}
__global__ __launch_bounds__(256) void k_al_finish(const float* __restrict__ part, int nblk, float s0, float s1, float s2, float* __restrict__ out) {
  __shared__ double sh[3][256];
  double a[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nblk; i += 256)
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] += (double)part[(long long)i * 3 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) sh[k][threadIdx.x] = a[k];
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) {
#pragma unroll
      for (int k = 0; k < 3; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + d];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)(sh[0][0] * (double)s0);
    out[1] = (float)(sh[1][0] * (double)s1);
    out[2] = (float)(sh[2][0] * (double)s2);
    out[3] = out[0] + (out[1] + out[2]);
  }
}
__global__ __launch_bounds__(256) void k_al_bwd(AlArgs A, const float* __restrict__ g3, void* __restrict__ drows) {
  const long long total = (long long)A.B * A.n_loc * A.K;
  const float g0 = g3[0] * A.scale[0], g1 = g3[1] * A.scale[1], g2 = g3[2] * A.scale[2];
  const int used = A.K * (A.C + 7 + A.nb);
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    float l[3], gc[kMaxCls], gb[7], gd[kMaxBins];
    al_anchor<true>(A, e, l, gc, gb, gd);
    const long long site = e / A.K;
    const int k = (int)(e % A.K);
    const long long r0 = site * A.ld;
    auto put = [&](long long o, float v) {
      if (A.bf16) ((unsigned short*)drows)[o] = gd_to_bf16(v);
      else ((float*)drows)[o] = v;
    };
    for (int c = 0; c < A.C; ++c) put(r0 + k * A.C + c, gc[c] * g0);
#pragma unroll
    for (int i = 0; i < 7; ++i) put(r0 + A.K * A.C + k * 7 + i, gb[i] * g1);
    for (int d = 0; d < A.nb; ++d) put(r0 + A.K * (A.C + 7) + k * A.nb + d, gd[d] * g2);
    if (k == 0)
      for (int p = used; p < A.ld; ++p) put(r0 + p, 0.f);          // the padding columns of the row product
  }
}
inline int al_fill(AlArgs& A, const void* rows, int bf16, int ld, int B, int n_loc, int K, int C, int nb, const int* labels, const float* reg,
                   const int* bins, const int* npos, const float* cw, const float* scale) {
  GD_REQUIRE(rows && labels && reg && npos && B >= 1 && n_loc >= 1 && K >= 1 && C >= 1 && C <= kMaxCls && nb >= 0 && nb <= kMaxBins &&
             ld >= K * (C + 7 + nb) && (nb == 0 || bins), "anchor_loss: bad arguments");
  A.rows = rows; A.bf16 = bf16; A.ld = ld; A.B = B; A.n_loc = n_loc; A.K = K; A.C = C; A.nb = nb;
  A.labels = labels; A.reg = reg; A.bins = bins; A.npos = npos;
  for (int i = 0; i < 7; ++i) A.cw[i] = cw[i];
  for (int i = 0; i < 3; ++i) A.scale[i] = scale[i];
  return 0;
}
}  // namespace

extern "C" int gdmae_anchor_loss_rows(void) { return 1024; }
// out4 = {cls, loc, dir, cls + (loc + dir)} (each x scale); partials: gdmae_anchor_loss_rows() * 3 floats
extern "C" int gdmae_anchor_loss_fwd(const void* rows, int rows_bf16, int ld, int B, int n_loc, int K, int C, int nb, const int* labels,
                                     const float* reg_targets, const int* dir_bins, const int* num_pos, const float* code_weights /* host [7] */,
                                     const float* scale /* host [3] */, float* partials, float* out4, void* stream) {
  AlArgs A;
  if (int rc = al_fill(A, rows, rows_bf16, ld, B, n_loc, K, C, nb, labels, reg_targets, dir_bins, num_pos, code_weights, scale)) return rc;
  GD_REQUIRE(partials && out4, "anchor_loss_fwd: bad arguments");
  const long long total = (long long)B * n_loc * K;
  const int nblk = (int)(gd_div_up(total, 256) > 1024 ? 1024 : gd_div_up(total, 256));
  hipLaunchKernelGGL(k_al_fwd, dim3(nblk), dim3(256), 0, (hipStream_t)stream, A, partials);
  GD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_al_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partials, nblk, scale[0], scale[1], scale[2], out4);
  GD_LAUNCH_CHECK();
  return 0;
}
// drows: (B * n_loc, ld) in the rows' type, every element written; grad3 (device): the gradients of the three losses
extern "C" int gdmae_anchor_loss_bwd(const void* rows, int rows_bf16, int ld, int B, int n_loc, int K, int C, int nb, const int* labels,
                                     const float* reg_targets, const int* dir_bins, const int* num_pos, const float* code_weights,
                                     const float* scale, const float* grad3, void* drows, void* stream) {
  AlArgs A;
  if (int rc = al_fill(A, rows, rows_bf16, ld, B, n_loc, K, C, nb, labels, reg_targets, dir_bins, num_pos, code_weights, scale)) return rc;
  GD_REQUIRE(grad3 && drows, "anchor_loss_bwd: bad arguments");
  const long long total = (long long)B * n_loc * K;
  long long g = gd_div_up(total, 256);
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(k_al_bwd, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, A, grad3, drows);
  GD_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// generate_predicted_boxes (anchor_head_template.py:224-266) for all B x A anchors in one launch
// ------------------------------------------------------------------------------------------------
namespace {
struct AdArgs {
  const void* rows;
  int bf16, ld, B, H, W, K, C, nb;
  const float *xc, *yc, *slot;
  float dir_offset, dir_limit_offset;
  float* cls_out;
  float* boxes;
};
__global__ __launch_bounds__(256) void k_ah_decode(AdArgs D) {
  const long long A = (long long)D.H * D.W * D.K;
  const long long e = blockIdx.x * 256ll + threadIdx.x;
  if (e >= (long long)D.B * A) return;
  const long long a = e % A;
  const int k = (int)(a % D.K);
  const long long loc = a / D.K;
  const int x = (int)(loc % D.W), y = (int)(loc / D.W);
  const long long r0 = (e / D.K) * D.ld;
  auto at = [&](long long o) {
    return D.bf16 ? __uint_as_float(((unsigned)((const unsigned short*)D.rows)[o]) << 16) : ((const float*)D.rows)[o];
  };
  for (int c = 0; c < D.C; ++c) D.cls_out[e * D.C + c] = at(r0 + k * D.C + c);
  const long long b0 = r0 + D.K * D.C + k * 7;
  const long long d0 = r0 + D.K * (D.C + 7) + k * D.nb;
  float o[7];
  ah_decode_box([&](int i) { return at(b0 + i); }, [&](int d) { return at(d0 + d); }, D.nb, D.xc[x], D.yc[y], D.slot + k * 5, D.dir_offset,
                D.dir_limit_offset, o);
#pragma unroll
  for (int i = 0; i < 7; ++i) D.boxes[e * 7 + i] = o[i];
}
}  // namespace
// cls_out (B, A, C) fp32: the class logits in anchor order; boxes (B, A, 7) fp32
extern "C" int gdmae_anchor_decode(const void* rows, int rows_bf16, int ld, int B, int H, int W, int K, int C, int nb, const float* xc,
                                   const float* yc, const float* slot, float dir_offset, float dir_limit_offset, float* cls_out, float* boxes,
                                   void* stream) {
  GD_REQUIRE(rows && B >= 1 && H >= 1 && W >= 1 && K >= 1 && C >= 1 && nb >= 0 && ld >= K * (C + 7 + nb) && cls_out && boxes,
             "anchor_decode: bad arguments");
  AdArgs D{rows, rows_bf16, ld, B, H, W, K, C, nb, xc, yc, slot, dir_offset, dir_limit_offset, cls_out, boxes};
  hipLaunchKernelGGL(k_ah_decode, dim3((unsigned)gd_div_up((long long)B * H * W * K, 256)), dim3(256), 0, (hipStream_t)stream, D);
  GD_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Score selection in front of the class-agnostic NMS (detector3d_template.py:269-274, model_nms_utils.py:8-11)
// ------------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(1024) void k_ah_select(const float* __restrict__ cls, int n, int C, int normalized, float thresh,
                                                    int* __restrict__ idx, float* __restrict__ score, int* __restrict__ label,
                                                    int* __restrict__ count) {
  __shared__ int s_wave[16];
  __shared__ int s_base;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* p = cls + (long long)b * n * C;
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + tid;
    float best = -1.f;
    int arg = 0;
    bool ok = false;
    if (i < n) {
      const float* q = p + (long long)i * C;
      ah_best_class([&](int c) { return q[c]; }, C, normalized, best, arg);
      ok = best >= thresh;
    }
    const unsigned long long m = __ballot(ok);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int off = s_base;
    for (int w = 0; w < wave; ++w) off += s_wave[w];
    if (ok) {
      const long long o = (long long)b * n + off + __popcll(m & ((1ull << lane) - 1ull));
      idx[o] = i; score[o] = best; label[o] = arg + 1;
    }
    __syncthreads();
    if (tid == 0) {
      int t = 0;
      for (int w = 0; w < 16; ++w) t += s_wave[w];
      s_base += t;
    }
    __syncthreads();
  }
  if (tid == 0) count[b] = s_base;
}
}  // namespace
// cls (B, n, C) fp32 logits (or scores with normalized = 1).  -> per sample the count[b] anchors with best-class score >= thresh, in
// anchor order: idx / label (1-based class) int32 and score fp32, each (B, n) with the first count[b] entries of a row written.
extern "C" int gdmae_anchor_select(const float* cls, int B, int n, int C, int normalized, float thresh, int* idx, float* score, int* label,
                                   int* count, void* stream) {
  GD_REQUIRE(cls && B >= 1 && n >= 1 && C >= 1 && idx && score && label && count, "anchor_select: bad arguments");
  hipLaunchKernelGGL(k_ah_select, dim3(B), dim3(1024), 0, (hipStream_t)stream, cls, n, C, normalized, thresh, idx, score, label, count);
  GD_LAUNCH_CHECK();
  return 0;
}
