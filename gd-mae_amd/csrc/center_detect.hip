// CenterHead evaluation tail for the WHOLE batch in three launches: head maps + the top-K cells of every sample -> final
// boxes of all samples and classes, padded to a shape that depends on the config only, nothing read on the host.  It reproduces
// `CenterHead.generate_predicted_boxes` for one head sample by sample (that path: one decode launch, then per sample - and per class
// with multi_class_nms - a mask gather, a nonzero, a sort, a two-launch NMS and a host read of the kept count).
//
//   k_cd_sort   one 256-thread workgroup per sample: decode every candidate (ch_decode_cell, the arithmetic of k_ch_decode), rectify
//               the score, form 64-bit keys (class | ~score bits | top-K position), bitonic-sort <= 1024 of them in LDS, keep the
//               pre_max best per class and write the sorted boxes / scores / labels and n[b] to the workspace.
//   k_cd_masks  (words, words, B) grid of 64-thread blocks, as k_nms_masks: the suppression words of the same-class pairs (bev_iou of
//               bev_iou.h, the class's threshold).  Blocks below the diagonal, beyond n[b] or without a same-class pair do no pair work.
//   k_cd_scan   one wavefront per sample: the sequential scan of k_nms_scan with the removed bits in LDS, the mask rows staged 64 at a
//               time through LDS (one load latency per 64 boxes instead of one per kept box), kept boxes counted per class against
//               post_max; then the compacted rows, the zero padding and count[b] in parallel.
//
// Order of the valid candidates: (class ascending when class-aware, rectified score descending, top-K position ascending); all of it
// is in the key, so the sort has no ties and the result does not depend on scheduling.  No atomics.
#include "bev_iou.h"
#include "center_decode.h"

namespace {
constexpr int kMaxK = 1024, kMaxC = 8;
constexpr unsigned long long kInvalid = ~0ull;

struct CdClasses {
  float thresh[kMaxC], rectifier[kMaxC];
  int pre_max[kMaxC], post_max[kMaxC], to_global[kMaxC];
  int C, class_aware;
};
struct CdWork {
  float* boxes;                // (B, K, box_dim) sorted candidates that entered the NMS
  float* score;                // (B, K)
  int* label;                  // (B, K) global class, 0-based
  int* n;                      // (B)
  unsigned long long* mask;    // (B, K, words)
};

__device__ __forceinline__ int cd_key_class(unsigned long long k) { return (int)(k >> 42); }

// N: power of two >= K (sorted in LDS), 256 threads
__global__ __launch_bounds__(256) void k_cd_sort(const long long* __restrict__ cell, const float* __restrict__ score, ChMaps M, ChGeom G, int K,
                                                 int N, int box_dim, CdClasses P, CdWork Wk) {
  __shared__ unsigned long long keys[kMaxK];
  __shared__ int s_start[kMaxC], s_end[kMaxC];
  const int b = blockIdx.x, t = threadIdx.x;
  const long long row = (long long)b * K;
  if (t < kMaxC) { s_start[t] = 0; s_end[t] = 0; }
  for (int i = t; i < N; i += 256) {
    unsigned long long key = kInvalid;
    if (i < K) {
      float box[9], q;
      int cls;
      const float s = score[row + i];
      bool ok = ch_decode_cell(M, G, b, cell[row + i], s, box, cls, q);
      ok = ok && cls >= 0 && cls < P.C;
      if (ok) {
        const int g = P.to_global[cls];
        float r = s;
        if (P.class_aware) {
          const float a = P.rectifier[g];
          r = powf(s, 1.f - a) * powf(q, a);
        }
        const unsigned long long sc = P.class_aware ? (unsigned long long)g : 0ull;
        key = (sc << 42) | ((unsigned long long)(~__float_as_uint(r)) << 10) | (unsigned long long)i;
      }
    }
    keys[i] = key;
  }
  __syncthreads();
  // bitonic sort, ascending: N / 2 compare-exchanges per step on 256 threads
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
  // class segments of the sorted list (the classes ascend): first and one-past-last position of every class
  for (int p = t; p < N; p += 256) {
    const unsigned long long key = keys[p];
    if (key == kInvalid) continue;
    const int c = cd_key_class(key);
    if (p == 0 || cd_key_class(keys[p - 1]) != c) s_start[c] = p;
    if (p + 1 == N || keys[p + 1] == kInvalid || cd_key_class(keys[p + 1]) != c) s_end[c] = p + 1;
  }
  __syncthreads();
  int off[kMaxC], total = 0;
#pragma unroll
  for (int c = 0; c < kMaxC; ++c) {
    off[c] = total;
    const int cnt = s_end[c] - s_start[c];
    total += cnt < P.pre_max[c] ? cnt : P.pre_max[c];
  }
  if (t == 0) Wk.n[b] = total;
  for (int p = t; p < N; p += 256) {
    const unsigned long long key = keys[p];
    if (key == kInvalid) continue;
    const int c = cd_key_class(key);
    const int rank = p - s_start[c];
    if (rank >= P.pre_max[c]) continue;
    int o = 0;
#pragma unroll
    for (int e = 0; e < kMaxC; ++e) o = e == c ? off[e] : o;
    const int dst = o + rank;                                        // < total <= K
    const int i = (int)(key & 1023ull);
    float box[9], q;
    int cls;
    ch_decode_cell(M, G, b, cell[row + i], score[row + i], box, cls, q);      // the same bits as in the first pass
    for (int e = 0; e < box_dim; ++e) Wk.boxes[(row + dst) * box_dim + e] = box[e];
    Wk.score[row + dst] = __uint_as_float(~(unsigned)(key >> 10));
    Wk.label[row + dst] = P.to_global[cls];
  }
}

// mask[b][i][cb] bit j: box (64 cb + j) > i of the same class overlaps box i beyond the class's threshold
__global__ __launch_bounds__(64) void k_cd_masks(int K, int words, int box_dim, CdClasses P, CdWork Wk) {
  __shared__ float cols[64 * 7];
  __shared__ int colc[64];
  const int b = blockIdx.z, rb = blockIdx.y, cb = blockIdx.x, t = threadIdx.x;
  const int n = Wk.n[b];
  const int nw = (n + 63) >> 6;
  if (rb >= nw || cb >= nw || cb < rb) return;                       // uniform: the scan reads words [row >> 6, nw) of rows < n only
  const long long row = (long long)b * K;
  const int cn = min(64, n - cb * 64), rn = min(64, n - rb * 64);
  const int* lab = Wk.label + row;
  unsigned long long* out = Wk.mask + ((row + rb * 64 + t) * words + cb);
  // the classes ascend along the list: no same-class pair when the last row class is below the first column class
  if (P.class_aware && cb > rb && lab[rb * 64 + rn - 1] < lab[cb * 64]) {
    if (t < rn) *out = 0ull;
    return;
  }
  if (t < cn) {
    const float* src = Wk.boxes + (row + cb * 64 + t) * box_dim;
    for (int e = 0; e < 7; ++e) cols[t * 7 + e] = src[e];
    colc[t] = P.class_aware ? lab[cb * 64 + t] : 0;
  }
  __syncthreads();
  if (t >= rn) return;
  const int i = rb * 64 + t;
  float bi[7];
  for (int e = 0; e < 7; ++e) bi[e] = Wk.boxes[(row + i) * box_dim + e];
  const int ci = P.class_aware ? lab[i] : 0;
  float thr = P.thresh[0];
#pragma unroll
  for (int e = 1; e < kMaxC; ++e) thr = e == ci ? P.thresh[e] : thr;
  const float hi = 0.5f * sqrtf(bi[3] * bi[3] + bi[4] * bi[4]);
  unsigned long long w = 0ull;
  for (int j = cb == rb ? t + 1 : 0; j < cn; ++j) {
    if (colc[j] != ci) continue;
    const float* bj = cols + j * 7;
    // exact pre-reject: every point of the intersection polygon is an edge crossing or a corner of one box within the other's
    // extent + 1e-2 (bev_iou.h), so centres farther apart than the half-diagonals + 0.05 give no point, an overlap of 0 and a bit
    // of 0 for any threshold >= 0.  (inf / NaN sizes compare false and take the full test.)
    const float dx = bi[0] - bj[0], dy = bi[1] - bj[1];
    const float reach = hi + 0.5f * sqrtf(bj[3] * bj[3] + bj[4] * bj[4]) + 0.05f;
    if (dx * dx + dy * dy > reach * reach) continue;
    if (bev_iou(bi, bj) > thr) w |= 1ull << j;
  }
  *out = w;
}

__global__ __launch_bounds__(64) void k_cd_scan(int K, int words, int box_dim, int n_out, CdClasses P, CdWork Wk, float* __restrict__ boxes,
                                                float* __restrict__ scores, long long* __restrict__ labels, int* __restrict__ count) {
  __shared__ unsigned long long removed[kMaxK / 64];
  __shared__ unsigned long long tile[64][kMaxK / 64 + 1];
  __shared__ int tcls[64];
  __shared__ int kept[kMaxK];
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long row = (long long)b * K;
  const int n = Wk.n[b];
  const int nw = (n + 63) >> 6;
  if (lane < kMaxK / 64) removed[lane] = 0ull;
  int cnt = 0;
  int left[kMaxC];                                                   // boxes a class may still emit (uniform)
#pragma unroll
  for (int c = 0; c < kMaxC; ++c) left[c] = P.post_max[c];
  for (int tb = 0; tb < nw; ++tb) {
    const int nwc = nw - tb, rn = min(64, n - tb * 64);
    __syncthreads();
    for (int e = lane; e < rn * nwc; e += 64) {
      const int r = e / nwc, w = tb + e % nwc;
      tile[r][w] = Wk.mask[(row + tb * 64 + r) * words + w];
    }
    if (lane < rn) tcls[lane] = P.class_aware ? Wk.label[row + tb * 64 + lane] : 0;
    __syncthreads();
    for (int r = 0; r < rn; ++r) {
      const int i = tb * 64 + r;
      const bool dead = (removed[tb] >> r) & 1ull;                   // uniform across the wavefront
      if (!dead) {
        const int c = tcls[r];
        int room = 0;
#pragma unroll
        for (int e = 0; e < kMaxC; ++e) room = e == c ? left[e] : room;
        if (room > 0 && cnt < n_out) {
          if (lane == 0) kept[cnt] = i;
          ++cnt;
#pragma unroll
          for (int e = 0; e < kMaxC; ++e) left[e] -= e == c ? 1 : 0;
          if (lane >= tb && lane < nw) removed[lane] |= tile[r][lane];
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();
  // rows below cnt: the kept boxes in scan order (class by class, descending score); the rest zero
  for (int k = lane; k < n_out; k += 64) {
    const long long o = (long long)b * n_out + k;
    if (k < cnt) {
      const long long s = row + kept[k];
      for (int e = 0; e < box_dim; ++e) boxes[o * box_dim + e] = Wk.boxes[s * box_dim + e];
      scores[o] = Wk.score[s];
      labels[o] = (long long)Wk.label[s] + 1;
    } else {
      for (int e = 0; e < box_dim; ++e) boxes[o * box_dim + e] = 0.f;
      scores[o] = 0.f;
      labels[o] = 0;
    }
  }
  if (lane == 0) count[b] = cnt;
}

size_t cd_layout(int B, int K, int box_dim, void* ws, CdWork* Wk) {
  const size_t words = (size_t)(K + 63) / 64, rows = (size_t)B * K;
  GdArena A(ws, ~(size_t)0);
  float* boxes = A.take<float>(rows * box_dim);
  float* score = A.take<float>(rows);
  int* label = A.take<int>(rows);
  int* n = A.take<int>((size_t)B);
  unsigned long long* mask = A.take<unsigned long long>(rows * words);
  if (Wk) *Wk = CdWork{boxes, score, label, n, mask};
  return A.off;
}
}  // namespace

extern "C" size_t gdmae_center_head_detect_workspace_bytes(int B, int K, int box_dim) {
  if (B < 1 || K < 1 || K > kMaxK || box_dim < 7 || box_dim > 9) return 0;
  return cd_layout(B, K, box_dim, nullptr, nullptr);
}

// see include/gdmae_hip.h
extern "C" int gdmae_center_head_detect(const long long* cell, const float* score, const float* center, const float* center_z, const float* dim,
                                        const float* rot, const float* vel, const float* iou, int B, int K, int H, int W, const float* pc_range,
                                        const float* voxel_size, float feature_map_stride, const float* post_center_limit_range,
                                        float score_thresh, int use_score_thresh, int C, const float* thresh, const int* pre_max,
                                        const int* post_max, const float* rectifier, const int* to_global, int class_aware, int n_out,
                                        float* boxes, float* scores, long long* labels, int* count, void* workspace, void* stream) {
  GD_REQUIRE(B >= 1 && K >= 1 && H >= 1 && W >= 1, "center_head_detect: bad sizes");
  GD_REQUIRE(K <= kMaxK, "center_head_detect: more than 1024 candidates per sample (the sort and the bit set live in LDS)");
  GD_REQUIRE(C >= 1 && C <= kMaxC, "center_head_detect: 1 to 8 classes");
  GD_REQUIRE(cell && score && center && center_z && dim && rot && thresh && pre_max && post_max && rectifier && to_global && boxes &&
                 scores && labels && count && workspace,
             "center_head_detect: null argument");
  CdClasses P;
  P.C = C;
  P.class_aware = class_aware ? 1 : 0;
  const int slots = P.class_aware ? C : 1;
  long long room = 0;
  unsigned seen = 0u;
  for (int c = 0; c < kMaxC; ++c) {
    const bool on = c < slots;
    if (on) {
      GD_REQUIRE(thresh[c] >= 0.f, "center_head_detect: negative NMS threshold");          // (a NaN is refused as well)
      GD_REQUIRE(pre_max[c] >= 0 && post_max[c] >= 0, "center_head_detect: negative NMS_PRE_MAXSIZE / NMS_POST_MAXSIZE");
      room += post_max[c];
    }
    P.thresh[c] = on ? thresh[c] : 0.f;
    P.rectifier[c] = on && P.class_aware ? rectifier[c] : 0.f;
    P.pre_max[c] = on ? (pre_max[c] < K ? pre_max[c] : K) : 0;
    P.post_max[c] = on ? (post_max[c] < K ? post_max[c] : K) : 0;
    P.to_global[c] = 0;
    if (c < C) {
      GD_REQUIRE(to_global[c] >= 0 && to_global[c] < C && !(seen >> to_global[c] & 1u), "center_head_detect: to_global is no permutation of 0 .. C - 1");
      seen |= 1u << to_global[c];
      P.to_global[c] = to_global[c];
    }
  }
  GD_REQUIRE(n_out == (int)(room < K ? room : K) && n_out >= 1, "center_head_detect: n_out is not min(K, sum of NMS_POST_MAXSIZE)");
  const int box_dim = vel ? 9 : 7;
  CdWork Wk;
  cd_layout(B, K, box_dim, workspace, &Wk);
  ChMaps M{center, center_z, dim, rot, vel, iou};
  ChGeom G;
  ch_fill_geom(G, H, W, pc_range, voxel_size, feature_map_stride, post_center_limit_range, score_thresh, use_score_thresh);
  int N = 2;
  while (N < K) N <<= 1;
  const int words = (K + 63) / 64;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_cd_sort, dim3(B), dim3(256), 0, st, cell, score, M, G, K, N, box_dim, P, Wk);
  GD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cd_masks, dim3(words, words, B), dim3(64), 0, st, K, words, box_dim, P, Wk);
  GD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cd_scan, dim3(B), dim3(64), 0, st, K, words, box_dim, n_out, P, Wk, boxes, scores, labels, count);
  GD_LAUNCH_CHECK();
  return 0;
}
