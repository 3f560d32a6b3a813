// Fine-tune mode of the on-GPU input pipeline: the reference's per-frame chain
//   gt_sampling                                      pcdet/datasets/augmentor/database_sampler.py:214-258 (collision rule :242-251,
//                                                    paste and remove :161-212; in-box test roiaware_pool3d.cpp:128-140)
//   random_world_flip / _rotation / _scaling         augmentor/data_augmentor.py:55-143, with gt_boxes in the dict
//   heading limit_period, class column               data_augmentor.py:246-249, dataset.py:138-144
//   mask_points_and_boxes_outside_range              processor/data_processor.py:77-88, box_utils.py:28-72
//   collate_batch                                    dataset.py:181-192
// as two launches per batch.  The random decisions (which database entries, flips, angle, scale) are drawn on the host with the
// reference's np.random calls (gdmae_hip/input_pipeline.py) and arrive as small tables.
//
// gdmae_gt_sample_select: one workgroup per frame.  The frame's GT boxes and its candidates sit in LDS (448 + 64 boxes of 7 floats =
// 14 KB).  The sample groups are walked in order with a barrier between them; the (candidate, other box) pairs of a group are
// strided over the threads and a hit ORs the candidate's flag in LDS, so the flags do not depend on arrival order.  A candidate is
// valid when bev_overlap (bev_iou.h: the library's one definition) is zero against every GT box of the frame (all names), every
// valid candidate of an earlier group, and every OTHER candidate of its own group, valid or not.  The same workgroup then compacts
// the valid candidates in candidate order (the boxes the point pass removes scene points in, enlarged, with the cosine and sine of
// -heading and the half extents precomputed), transforms the kept GT boxes and the valid candidates operation by operation in
// fp32 as the reference's numpy does, counts each box's corners inside the closed 3-D range, and compacts the survivors into the
// frame's zero-padded row of gt_boxes.
//
// gdmae_gt_sample_collate: one compaction scan (gd_device_scan, as gdmae_augment_collate) over a virtual row space: per frame all
// candidates' object points, then the scene points.  A row finds its segment (source buffer, source row, frame, candidate) by a
// binary search in a host-built table of at most B + total candidates entries.  An object row is kept when its candidate is valid
// and the transformed point is inside the xy range; a scene row when the point lies in none of the frame's valid enlarged boxes and
// is inside the range.  One read and one write per kept point; the box loop (at most 64 boxes per frame) adds arithmetic only.
//
// gdmae_gt_sample_select_aug / _drop_plan / _collate_aug add random_world_translation (data_augmentor.py:145-171) and
// random_world_drop (:42-53) between the scaling and the range masks; the two entry points above compute what they always did.
#include "aug_xform.h"
#include "bev_iou.h"

#define GS_MAX_CAND 64
#define GS_MAX_GT 448
#define GS_MAX_BOX (GS_MAX_CAND + GS_MAX_GT)
#define GS_BLOCK 256
#define GS_SEG 8          // ints per segment: [first virtual row, source row, source buffer, frame, box row or -1, candidate, first of frame, first virtual row of the frame (read by the drop only)]

namespace {
constexpr float kPi = 3.14159265358979323846f;            // np.float32(np.pi)
constexpr float kTwoPi = 6.28318530717958647692f;         // np.float32(2 * np.pi)

struct GsSelect {
  const float* boxes;        // (n_boxes, 8): per frame its GT boxes, then its candidates; column 7 = class index + 1, 0 = foreign name
  const int* desc;           // (B, 4): first box row, GT boxes, candidates, first candidate
  const int* cand_group;     // (n_candidates): sample group of every candidate
  const float* tab;          // (B, 8): [flip_x, flip_y, cos, sin, scale, angle, 0, 0]
  int n_groups, min_corners, cap;
  float lo[3], hi[3], extra[3];
  int* valid;                // (n_candidates)
  float* rm_boxes;           // (B, 64, 8): [cx, cy, cz, dx/2 + margin, dy/2 + margin, dz/2, cos(-h), sin(-h)] of the enlarged valid boxes
  int* n_valid;              // (B)
  float* gt_out;             // (B, cap, 8)
  int* num_gt;               // (B)
  const double* trans;       // (B, 3) fp64 or null: random_world_translation of the box centres (gdmae_gt_sample_select_aug)
};

// numpy's in-place float32 += float64 (data_augmentor.py:162-164): the sum is formed in fp64 and rounded once
__device__ inline float gs_translate(float v, double t) { return (float)((double)v + t); }

// world transformation of one box, operation by operation in fp32 (data_augmentor.py:68-82, :107-108, :136, :247), class column last
__device__ inline void gs_box_xform(const float* t, const float* b, float cls, float (&o)[8]) {
  float x = b[0], y = b[1], z = b[2], h = b[6];
  if (t[0] != 0.f) h = -h;
  if (t[1] != 0.f) h = -(h + kPi);
  AugLoad::apply(t, x, y, z);               // centres move like points
  h = h + t[5];
  const float q = h / kTwoPi;               // limit_period(h, 0.5, 2 pi)
  h = h - floorf(q + 0.5f) * kTwoPi;
  o[0] = x;
  o[1] = y;
  o[2] = z;
  o[3] = b[3] * t[4];
  o[4] = b[4] * t[4];
  o[5] = b[5] * t[4];
  o[6] = h;
  o[7] = cls;
}

// corners of boxes_to_corners_3d (box_utils.py:28-53) inside the closed 3-D range
__device__ inline int gs_corners_in_range(const float (&o)[8], const float* lo, const float* hi) {
  const float cs = cosf(o[6]), sn = sinf(o[6]);
  const float hx = o[3] * 0.5f, hy = o[4] * 0.5f, hz = o[5] * 0.5f;
  int n = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float lx = (k & 1) ? -hx : hx, ly = (k & 2) ? -hy : hy, lz = (k & 4) ? hz : -hz;
    const float x = (lx * cs + ly * (-sn)) + o[0], y = (lx * sn + ly * cs) + o[1], z = lz + o[2];
    n += (x >= lo[0] && x <= hi[0] && y >= lo[1] && y <= hi[1] && z >= lo[2] && z <= hi[2]) ? 1 : 0;
  }
  return n;
}

__global__ __launch_bounds__(GS_BLOCK) void gs_select_kernel(GsSelect a) {
  __shared__ float s_box[GS_MAX_BOX * 7];
  __shared__ float s_cls[GS_MAX_BOX];
  __shared__ int s_group[GS_MAX_CAND], s_flag[GS_MAX_CAND], s_rank[GS_MAX_CAND], s_cnt[GS_MAX_BOX / GD_WAVE];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (GD_WAVE - 1);
  const int box0 = a.desc[b * 4], n_gt = a.desc[b * 4 + 1], n_cand = a.desc[b * 4 + 2], cand0 = a.desc[b * 4 + 3];
  const int ne = n_gt + n_cand;                                   // <= GS_MAX_BOX, checked on the host
  for (int i = tid; i < ne * 7; i += GS_BLOCK) s_box[i] = a.boxes[(long long)(box0 + i / 7) * 8 + i % 7];
  for (int i = tid; i < ne; i += GS_BLOCK) s_cls[i] = a.boxes[(long long)(box0 + i) * 8 + 7];
  if (tid < GS_MAX_CAND) {
    s_flag[tid] = 0;
    s_group[tid] = tid < n_cand ? a.cand_group[cand0 + tid] : -1;
  }
  __syncthreads();
  for (int g = 0; g < a.n_groups; ++g) {
    for (int idx = tid; idx < n_cand * ne; idx += GS_BLOCK) {
      const int c = idx / ne, e = idx - c * ne;
      if (s_group[c] != g) continue;
      bool test = true;                                           // a GT box of the frame, whatever its name
      if (e >= n_gt) {
        const int k = e - n_gt, gk = s_group[k];
        test = gk == g ? k != c : (gk < g && s_flag[k] == 0);     // own group: every other one; earlier groups: the valid ones (final)
      }
      if (test && bev_overlap(&s_box[(n_gt + c) * 7], &s_box[e * 7]) > 0.f) atomicOr(&s_flag[c], 1);
    }
    __syncthreads();
  }
  // valid candidates, compacted in candidate order (wave 0: one lane per candidate)
  if (tid < GS_MAX_CAND) {
    const bool v = tid < n_cand && s_flag[tid] == 0;
    const unsigned long long m = __ballot(v);
    const int rank = __popcll(m & ((1ull << lane) - 1ull));
    s_rank[tid] = v ? rank : -1;
    if (tid < n_cand) a.valid[cand0 + tid] = v ? 1 : 0;
    if (v) {
      const float* q = &s_box[(n_gt + tid) * 7];
      float* o = a.rm_boxes + ((long long)b * GS_MAX_CAND + rank) * 8;
      o[0] = q[0];
      o[1] = q[1];
      o[2] = q[2];
      o[3] = (q[3] + a.extra[0]) * 0.5f + kMargin;
      o[4] = (q[4] + a.extra[1]) * 0.5f + kMargin;
      o[5] = (q[5] + a.extra[2]) * 0.5f;
      o[6] = cosf(-q[6]);
      o[7] = sinf(-q[6]);
    }
    if (tid == 0) a.n_valid[b] = __popcll(m);
  }
  __syncthreads();
  // GT boxes of the selected classes, then the valid candidates: transform, range test, compact in order
  const float* t = a.tab + b * 8;
  float ob[2][8];
  unsigned long long km[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = tid + j * GS_BLOCK;
    bool keep = false;
    if (i < ne && (i < n_gt ? s_cls[i] > 0.f : s_rank[i - n_gt] >= 0)) {
      gs_box_xform(t, &s_box[i * 7], s_cls[i], ob[j]);
      if (a.trans) {                                              // after the scaling, before the corner test
#pragma unroll
        for (int c = 0; c < 3; ++c) ob[j][c] = gs_translate(ob[j][c], a.trans[b * 3 + c]);
      }
      keep = gs_corners_in_range(ob[j], a.lo, a.hi) >= a.min_corners;
    }
    km[j] = __ballot(keep);
    if (lane == 0) s_cnt[i / GD_WAVE] = __popcll(km[j]);
  }
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int q = 0; q < GS_MAX_BOX / GD_WAVE; ++q) total += s_cnt[q];
  float* out = a.gt_out + (long long)b * a.cap * 8;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = tid + j * GS_BLOCK, chunk = i / GD_WAVE;
    if (!((km[j] >> lane) & 1ull)) continue;
    int pos = __popcll(km[j] & ((1ull << lane) - 1ull));
    for (int q = 0; q < chunk; ++q) pos += s_cnt[q];
    if (pos < a.cap)
      for (int c = 0; c < 8; ++c) out[pos * 8 + c] = ob[j][c];
  }
  for (int i = total * 8 + tid; i < a.cap * 8; i += GS_BLOCK) out[i] = 0.f;     // collate_batch pads with zero rows
  if (tid == 0) a.num_gt[b] = total;
}

struct GsLoad {
  const float* src[2];       // 0: the staged frames (and, in the staged mode, the object points behind them), 1: the resident database
  int F, S;
  const int* seg;            // (S, GS_SEG)
  const float* tab;
  const float* boxes;
  const int* valid;
  const float* rm_boxes;
  const int* n_valid;        // null: no scene point is removed
  float xmin, ymin, xmax, ymax;
  __device__ int find(long long i) const {          // last segment that starts at or before row i
    int lo = 0, hi = S - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (seg[mid * GS_SEG] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
  }
  // the row's source and its coordinates before the world transformation (object points: local point + fp32 box centre)
  __device__ const float* point(long long i, const int* g, float& x, float& y, float& z) const {
    const float* p = src[g[2]] + ((long long)g[1] + (i - g[0])) * F;
    x = p[0];
    y = p[1];
    z = p[2];
    if (g[4] >= 0) {
      const float* c = boxes + (long long)g[4] * 8;
      x = x + c[0];
      y = y + c[1];
      z = z + c[2];
    }
    return p;
  }
  // the first half of operator() on its own (the drop needs it): 1 when the reference's points holds the row after gt_sampling - an
  // object row of a valid candidate, a scene row in none of the frame's valid enlarged boxes.  x, y, z: the row's coordinates before
  // the world transformation
  __device__ int eligible(long long i, const int* g, float& x, float& y, float& z) const {
    if (g[4] >= 0) {
      if (!valid[g[5]]) return 0;
      point(i, g, x, y, z);
    } else {
      point(i, g, x, y, z);
      const int nv = n_valid ? n_valid[g[3]] : 0;          // null: REMOVE_POINTS is off
      const float* q = rm_boxes + (long long)g[3] * GS_MAX_CAND * 8;
      for (int k = 0; k < nv; ++k, q += 8) {          // roiaware_pool3d.cpp:128-140 on the enlarged box
        if (fabsf(z - q[2]) > q[5]) continue;
        const float sx = x - q[0], sy = y - q[1];
        const float lx = sx * q[6] + sy * (-q[7]), ly = sx * q[7] + sy * q[6];
        if (fabsf(lx) < q[3] && fabsf(ly) < q[4]) return 0;
      }
    }
    return 1;
  }
  __device__ int operator()(long long i) const {
    const int* g = seg + find(i) * GS_SEG;
    float x, y, z;
    if (g[4] >= 0) {
      if (!valid[g[5]]) return 0;
      point(i, g, x, y, z);
    } else {
      point(i, g, x, y, z);
      const int nv = n_valid ? n_valid[g[3]] : 0;          // null: REMOVE_POINTS is off
      const float* q = rm_boxes + (long long)g[3] * GS_MAX_CAND * 8;
      for (int k = 0; k < nv; ++k, q += 8) {          // roiaware_pool3d.cpp:128-140 on the enlarged box
        if (fabsf(z - q[2]) > q[5]) continue;
        const float sx = x - q[0], sy = y - q[1];
        const float lx = sx * q[6] + sy * (-q[7]), ly = sx * q[7] + sy * q[6];
        if (fabsf(lx) < q[3] && fabsf(ly) < q[4]) return 0;
      }
    }
    AugLoad::apply(tab + g[3] * 8, x, y, z);
    return (x >= xmin && x <= xmax && y >= ymin && y <= ymax) ? 1 : 0;
  }
};

struct GsStore {
  GsLoad L;
  float* out;        // (n_kept, 1 + F)
  int* kept_off;     // (B + 1): first output row of every frame that has virtual rows
  __device__ void operator()(long long i, int ex, int v) const {
    const int* g = L.seg + L.find(i) * GS_SEG;
    if (g[6] && i == g[0]) kept_off[g[3]] = ex;
    if (v) {
      float x, y, z;
      const float* p = L.point(i, g, x, y, z);
      AugLoad::apply(L.tab + g[3] * 8, x, y, z);
      float* o = out + (long long)ex * (L.F + 1);
      o[0] = (float)g[3];
      o[1] = x;
      o[2] = y;
      o[3] = z;
      for (int c = 3; c < L.F; ++c) o[1 + c] = p[c];
    }
  }
};

// ---- random_world_translation and random_world_drop (DESIGN §7l "translation and drop") -----------------------------------------
// The drop keeps, per frame, the k = (long long)(q * n) eligible rows that are smallest by (key, virtual row j of the frame).  Key and
// row form one 63-bit number c = key << 31 | j (j < 2^31) that no two rows of a frame share, so the kept set is "c <= the k-th
// smallest c": a radix select, most significant digit first.  Six digits: 8 + 12 + 12 bits of the key, 12 + 12 + 7 bits of the row.
// Per digit one launch builds, per frame, the histogram of the digit over the eligible rows whose higher digits equal the prefix
// chosen so far (LDS histogram per workgroup, flushed with integer atomics: the counts do not depend on arrival order), and one
// workgroup per frame picks the bucket that holds the k-th row.  After the third digit the key T of the k-th row, the number of
// rows with that key (ties) and how many of them are admitted are known; a frame goes on to the row digits only when some but not
// all of its ties are admitted, and leaves them with J, the last admitted tie's row.  A row is admitted when
// key < T || (key == T && j <= J).  The first pass also records every row's eligibility (one byte), which the later passes and
// the collate scan read instead of repeating the box test.
#define GS_DROP_TILE 4096      // rows per workgroup of a histogram pass
#define GS_DROP_BINS 4096      // widest digit: 12 bits
#define GS_PLAN 8              // ints per frame of the plan: [n, k, T, admitted ties, J, ties, 0, 0]
#define GS_STATE 4             // words per frame of the select's state: [prefix low, prefix high, rows still to take, active]

__device__ inline unsigned gs_drop_key(unsigned long long seed, unsigned j) {      // splitmix64's finaliser, upper half
  unsigned long long z = seed + ((unsigned long long)j + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (unsigned)((z ^ (z >> 31)) >> 32);
}

struct GsDrop {
  const unsigned long long* seeds;   // (B)
  const unsigned* keys;              // (n_rows) explicit keys by virtual row, or null: gs_drop_key(seeds[frame], j)
  const int* plan;                   // (B, GS_PLAN)
  const unsigned char* elig;         // (n_rows)
  __device__ unsigned key(long long i, int frame, unsigned j) const { return keys ? keys[i] : gs_drop_key(seeds[frame], j); }
  __device__ bool admitted(long long i, const int* g) const {
    const unsigned j = (unsigned)(i - g[7]);
    const unsigned k = key(i, g[3], j), T = (unsigned)plan[g[3] * GS_PLAN + 2];
    return k < T || (k == T && (int)j <= plan[g[3] * GS_PLAN + 4]);
  }
};

struct GsLoadAug : GsLoad {
  const double* trans;       // (B, 3) or null
  GsDrop D;                  // D.plan null: no drop in this batch
  __device__ void xform(int frame, float& x, float& y, float& z) const {
    AugLoad::apply(tab + frame * 8, x, y, z);
    if (trans) {
      x = gs_translate(x, trans[frame * 3]);
      y = gs_translate(y, trans[frame * 3 + 1]);
      z = gs_translate(z, trans[frame * 3 + 2]);
    }
  }
  __device__ int operator()(long long i) const {
    const int* g = seg + find(i) * GS_SEG;
    float x, y, z;
    if (D.plan) {
      if (!D.elig[i] || !D.admitted(i, g)) return 0;
      point(i, g, x, y, z);
    } else if (!eligible(i, g, x, y, z)) {
      return 0;
    }
    xform(g[3], x, y, z);
    return (x >= xmin && x <= xmax && y >= ymin && y <= ymax) ? 1 : 0;
  }
};

struct GsStoreAug {
  GsLoadAug L;
  float* out;
  int* kept_off;
  __device__ void operator()(long long i, int ex, int v) const {
    const int* g = L.seg + L.find(i) * GS_SEG;
    if (g[6] && i == g[0]) kept_off[g[3]] = ex;
    if (v) {
      float x, y, z;
      const float* p = L.point(i, g, x, y, z);
      L.xform(g[3], x, y, z);
      float* o = out + (long long)ex * (L.F + 1);
      o[0] = (float)g[3];
      o[1] = x;
      o[2] = y;
      o[3] = z;
      for (int c = 3; c < L.F; ++c) o[1 + c] = p[c];
    }
  }
};

struct GsPlanArgs {
  GsLoad L;
  long long n_rows;
  GsDrop D;                  // D.elig is written by the first pass (elig_w), D.plan by the picks (plan_w)
  unsigned char* elig_w;
  int* plan_w;
  const double* q;           // (B)
  unsigned* state;           // (B, GS_STATE)
  int* hist;                 // (B, GS_DROP_BINS), zero between the passes
};

// digit [lo, lo + w) of c over the rows of one tile; FIRST: the most significant digit, which also settles eligibility
template <bool FIRST>
__global__ __launch_bounds__(GS_BLOCK) void gs_drop_hist_kernel(GsPlanArgs a, int lo, int w) {
  __shared__ int s_hist[GS_DROP_BINS];
  __shared__ int s_seg[2];
  const int tid = threadIdx.x, nb = 1 << w;
  const long long base = (long long)blockIdx.x * GS_DROP_TILE;
  const long long end = base + GS_DROP_TILE < a.n_rows ? base + GS_DROP_TILE : a.n_rows;
  if (tid == 0) {
    s_seg[0] = a.L.find(base);
    s_seg[1] = a.L.find(end - 1);
  }
  for (int k = tid; k < nb; k += GS_BLOCK) s_hist[k] = 0;
  __syncthreads();
  const int s0 = s_seg[0], s1 = s_seg[1];
  int cur = -1;
  bool active = false, dirty = false;
  unsigned long long prefix = 0;
  for (int s = s0; s <= s1; ++s) {                      // every value that steers this loop is the same in all threads
    const int* g = a.L.seg + s * GS_SEG;
    const int f = g[3];
    if (f != cur) {
      if (dirty) {
        __syncthreads();
        for (int k = tid; k < nb; k += GS_BLOCK)
          if (const int v = s_hist[k]) {
            atomicAdd(&a.hist[cur * GS_DROP_BINS + k], v);
            s_hist[k] = 0;
          }
        __syncthreads();
        dirty = false;
      }
      cur = f;
      active = FIRST || a.state[f * GS_STATE + 3] != 0;
      prefix = FIRST ? 0ull : ((unsigned long long)a.state[f * GS_STATE + 1] << 32) | a.state[f * GS_STATE];
    }
    if (!active) continue;
    dirty = true;
    const long long r0 = g[0] > base ? (long long)g[0] : base;
    const long long nxt = s + 1 < a.L.S ? (long long)a.L.seg[(s + 1) * GS_SEG] : a.n_rows;
    const long long r1 = nxt < end ? nxt : end;
    for (long long i = r0 + tid; i < r1; i += GS_BLOCK) {
      int e;
      if (FIRST) {
        float x, y, z;
        e = a.L.eligible(i, g, x, y, z);
        a.elig_w[i] = (unsigned char)e;
      } else {
        e = a.D.elig[i];
      }
      if (!e) continue;
      const unsigned j = (unsigned)(i - g[7]);
      const unsigned long long c = ((unsigned long long)a.D.key(i, f, j) << 31) | j;
      if ((c >> (lo + w)) == prefix) atomicAdd(&s_hist[(int)(c >> lo) & (nb - 1)], 1);
    }
  }
  if (dirty) {
    __syncthreads();
    for (int k = tid; k < nb; k += GS_BLOCK)
      if (const int v = s_hist[k]) atomicAdd(&a.hist[cur * GS_DROP_BINS + k], v);
  }
}

// one workgroup per frame: the bucket of digit `pass` that holds the k-th row; leaves the frame's histogram zero
__global__ __launch_bounds__(GS_BLOCK) void gs_drop_pick_kernel(GsPlanArgs a, int pass, int w) {
  __shared__ int smem[GS_BLOCK / GD_WAVE + 1];
  constexpr int PER = GS_DROP_BINS / GS_BLOCK;
  const int f = blockIdx.x, tid = threadIdx.x, nb = 1 << w;
  unsigned* st = a.state + f * GS_STATE;
  int* plan = a.plan_w + f * GS_PLAN;
  int* h = a.hist + f * GS_DROP_BINS;
  if (pass > 0 && st[3] == 0) return;                   // settled: no row of this frame was counted
  const unsigned st_lo = st[0], st_hi = st[1], st_take = st[2];      // read before the scan's barriers: one thread rewrites them below
  int sum = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int b = tid * PER + k;
    if (b < nb) sum += h[b];
  }
  int total;
  const int ex = gd_block_exclusive_scan<int, GS_BLOCK>(sum, total, smem);
  long long take;
  unsigned long long prefix = 0;
  if (pass == 0) {
    take = (long long)(a.q[f] * (double)total);         // Python's int((1 - r) * n): fp64 product, truncation
    take = take < 0 ? 0 : (take > total ? total : take);
    if (tid == 0) {
      plan[0] = total;
      plan[1] = (int)take;
      plan[6] = plan[7] = 0;
      if (take == 0) {                                  // nothing is kept: no key is below 0 and no row at or below -1
        plan[2] = plan[3] = plan[5] = 0;
        plan[4] = -1;
        st[0] = st[1] = st[2] = st[3] = 0;
      }
    }
  } else {
    take = st_take;
    prefix = ((unsigned long long)st_hi << 32) | st_lo;
  }
  if (take > 0 && ex < take && take <= ex + sum) {      // exactly one thread: its buckets hold the take-th row
    int below = ex, b = tid * PER;
    while (below + h[b] < take) below += h[b++];
    const int cnt = h[b], rest = (int)take - below;     // 1 <= rest <= cnt
    prefix = (prefix << w) | (unsigned)b;
    int go = 1;
    if (pass == 2) {                                    // the key is complete
      plan[2] = (int)(unsigned)prefix;
      plan[3] = rest;
      plan[5] = cnt;
      if (rest == cnt) {                                // every tie is admitted
        plan[4] = 0x7FFFFFFF;
        go = 0;
      }
    } else if (pass == 5) {                             // the row is complete
      plan[4] = (int)(prefix & 0x7FFFFFFFull);
      go = 0;
    }
    st[0] = (unsigned)prefix;
    st[1] = (unsigned)(prefix >> 32);
    st[2] = (unsigned)rest;
    st[3] = (unsigned)go;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int b = tid * PER + k;
    if (b < nb) h[b] = 0;
  }
}
}  // namespace

extern "C" size_t gdmae_gt_sample_workspace_bytes(long long n_rows) { return (gd_scan_ws_elems(n_rows) + 4) * sizeof(int); }

// frame_desc_host / frame_desc: the same (B, 4) int32 table [first box row, GT boxes, candidates, first candidate] on the host (checked
// against the limits here) and on the device; range host {xmin, ymin, zmin, xmax, ymax, zmax}; extra_width host (3).
static int gs_select(const float* boxes, const int* frame_desc_host, const int* frame_desc, const int* cand_group, int B, int n_groups,
                     const float* frame_params, const double* translate, const float* range, const float* extra_width, int min_corners,
                     int cap, int* valid, float* rm_boxes, int* n_valid, float* gt_boxes, int* num_gt, void* stream) {
  GD_REQUIRE(B >= 1 && n_groups >= 0, "gt_sample_select: need at least one frame");
  for (int b = 0; b < B; ++b) {
    const int* d = frame_desc_host + b * 4;
    GD_REQUIRE(d[0] >= 0 && d[1] >= 0 && d[2] >= 0 && d[3] >= 0, "gt_sample_select: negative entry in the frame table");
    GD_REQUIRE(d[2] <= GS_MAX_CAND, "gt_sample_select: more than 64 candidates in one frame");
    GD_REQUIRE(d[1] <= GS_MAX_GT, "gt_sample_select: more than 448 existing boxes in one frame");
  }
  GD_REQUIRE(cap >= 0 && cap <= GS_MAX_BOX, "gt_sample_select: at most 512 output boxes per frame");
  GsSelect a{boxes, frame_desc, cand_group, frame_params, n_groups, min_corners, cap,
             {range[0], range[1], range[2]}, {range[3], range[4], range[5]}, {extra_width[0], extra_width[1], extra_width[2]},
             valid, rm_boxes, n_valid, gt_boxes, num_gt, translate};
  hipLaunchKernelGGL(gs_select_kernel, dim3(B), dim3(GS_BLOCK), 0, (hipStream_t)stream, a);
  GD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gdmae_gt_sample_select(const float* boxes, const int* frame_desc_host, const int* frame_desc, const int* cand_group, int B,
                                      int n_groups, const float* frame_params, const float* range, const float* extra_width,
                                      int min_corners, int cap, int* valid, float* rm_boxes, int* n_valid, float* gt_boxes, int* num_gt,
                                      void* stream) {
  return gs_select(boxes, frame_desc_host, frame_desc, cand_group, B, n_groups, frame_params, nullptr, range, extra_width, min_corners, cap,
                   valid, rm_boxes, n_valid, gt_boxes, num_gt, stream);
}

// translate (B, 3) fp64 device or null: every box centre becomes (float)((double)v + t) after the scaling and before the corner test
extern "C" int gdmae_gt_sample_select_aug(const float* boxes, const int* frame_desc_host, const int* frame_desc, const int* cand_group,
                                          int B, int n_groups, const float* frame_params, const double* translate, const float* range,
                                          const float* extra_width, int min_corners, int cap, int* valid, float* rm_boxes, int* n_valid,
                                          float* gt_boxes, int* num_gt, void* stream) {
  return gs_select(boxes, frame_desc_host, frame_desc, cand_group, B, n_groups, frame_params, translate, range, extra_width, min_corners,
                   cap, valid, rm_boxes, n_valid, gt_boxes, num_gt, stream);
}

// raw / db: the two source buffers of (rows, F) fp32 a segment can name (db may equal raw); seg (S, 8) int32 device, first rows
// ascending, covering [0, n_rows); boxes / valid / rm_boxes / n_valid: as gdmae_gt_sample_select read and wrote them;
// xy_range host {xmin, ymin, xmax, ymax}; out (>= n_rows, 1 + F); kept_off (B + 1) int32 device: first output row of every frame
// that has virtual rows (-1 for one without), kept_off[B] = rows written.
extern "C" int gdmae_gt_sample_collate(const float* raw, const float* db, int F, const int* seg, int S, long long n_rows, int B,
                                       const float* frame_params, const float* boxes, const int* valid, const float* rm_boxes,
                                       const int* n_valid, const float* xy_range, float* out, int* kept_off, void* workspace,
                                       void* stream) {
  GD_REQUIRE(F >= 3 && B >= 1, "gt_sample_collate: need xyz columns and at least one frame");
  GD_REQUIRE(n_rows < (1ll << 31), "gt_sample_collate: the segment table holds 32-bit rows");
  hipStream_t st = (hipStream_t)stream;
  if (n_rows <= 0) {
    GD_CHECK(hipMemsetAsync(kept_off, 0, sizeof(int) * (B + 1), st));
    return 0;
  }
  GD_REQUIRE(S >= 1, "gt_sample_collate: rows without a segment");
  GsLoad L{{raw, db}, F, S, seg, frame_params, boxes, valid, rm_boxes, n_valid, xy_range[0], xy_range[1], xy_range[2], xy_range[3]};
  GD_CHECK(hipMemsetAsync(kept_off, 0xFF, sizeof(int) * (B + 1), st));
  return gd_device_scan<int>(n_rows, L, GsStore{L, out, kept_off}, kept_off + B, (int*)workspace, st);
}

namespace {
struct GsDropWs {
  unsigned* state;
  int* hist;
  unsigned char* elig;
};
inline size_t gs_drop_ws_head(int B) { return gd_align(sizeof(unsigned) * GS_STATE * (size_t)B) + gd_align(sizeof(int) * GS_DROP_BINS * (size_t)B); }
inline GsDropWs gs_drop_ws(void* ws, int B) {
  char* p = (char*)ws;
  return {(unsigned*)p, (int*)(p + gd_align(sizeof(unsigned) * GS_STATE * (size_t)B)), (unsigned char*)(p + gs_drop_ws_head(B))};
}
}  // namespace

extern "C" size_t gdmae_gt_sample_drop_workspace_bytes(long long n_rows, int B) {
  return gs_drop_ws_head(B < 1 ? 1 : B) + gd_align((size_t)(n_rows > 0 ? n_rows : 0) + 1);
}

// The drop plan of a batch: seg, boxes, valid, rm_boxes, n_valid as gdmae_gt_sample_collate reads them (seg column 7 = the first virtual
// row of the segment's frame); seeds (B) uint64 and q (B) fp64 device; keys (n_rows) uint32 device or null; plan (B, 8) int32 device
// = [n, k, T, admitted rows with key T, J, rows with key T, 0, 0]; drop_ws: gdmae_gt_sample_drop_workspace_bytes(n_rows, B), handed
// unchanged to gdmae_gt_sample_collate_aug (it holds every row's eligibility).
extern "C" int gdmae_gt_sample_drop_plan(const float* raw, const float* db, int F, const int* seg, int S, long long n_rows, int B,
                                         const float* boxes, const int* valid, const float* rm_boxes, const int* n_valid,
                                         const unsigned long long* seeds, const double* q, const unsigned* keys, int* plan,
                                         void* drop_ws, void* stream) {
  GD_REQUIRE(F >= 3 && B >= 1, "gt_sample_drop_plan: need xyz columns and at least one frame");
  GD_REQUIRE(n_rows < (1ll << 31), "gt_sample_drop_plan: the segment table holds 32-bit rows");
  GD_REQUIRE(plan && drop_ws && q && (seeds || keys), "gt_sample_drop_plan: plan, workspace, q and seeds or keys are required");
  hipStream_t st = (hipStream_t)stream;
  if (n_rows <= 0) {
    GD_CHECK(hipMemsetAsync(plan, 0, sizeof(int) * GS_PLAN * B, st));
    return 0;
  }
  GD_REQUIRE(S >= 1, "gt_sample_drop_plan: rows without a segment");
  const GsDropWs W = gs_drop_ws(drop_ws, B);
  GsPlanArgs a{GsLoad{{raw, db}, F, S, seg, nullptr, boxes, valid, rm_boxes, n_valid, 0.f, 0.f, 0.f, 0.f}, n_rows,
               GsDrop{seeds, keys, plan, W.elig}, W.elig, plan, q, W.state, W.hist};
  GD_CHECK(hipMemsetAsync(W.hist, 0, sizeof(int) * GS_DROP_BINS * B, st));
  const int nblk = (int)gd_div_up(n_rows, GS_DROP_TILE);
  static const int kLo[6] = {55, 43, 31, 19, 7, 0}, kW[6] = {8, 12, 12, 12, 12, 7};      // 32 bits of key, 31 bits of row
  for (int p = 0; p < 6; ++p) {
    if (p == 0)
      hipLaunchKernelGGL(gs_drop_hist_kernel<true>, dim3(nblk), dim3(GS_BLOCK), 0, st, a, kLo[p], kW[p]);
    else
      hipLaunchKernelGGL(gs_drop_hist_kernel<false>, dim3(nblk), dim3(GS_BLOCK), 0, st, a, kLo[p], kW[p]);
    GD_LAUNCH_CHECK();
    hipLaunchKernelGGL(gs_drop_pick_kernel, dim3(B), dim3(GS_BLOCK), 0, st, a, p, kW[p]);
    GD_LAUNCH_CHECK();
  }
  return 0;
}

// gdmae_gt_sample_collate with the translation (translate (B, 3) fp64 device or null) applied after the scaling and before the range
// mask, and, when plan is not null, the scan predicate "eligible && admitted by the plan && in range"; seeds / keys / plan / drop_ws
// as gdmae_gt_sample_drop_plan took and left them.  With translate and plan null it computes what gdmae_gt_sample_collate computes.
extern "C" int gdmae_gt_sample_collate_aug(const float* raw, const float* db, int F, const int* seg, int S, long long n_rows, int B,
                                           const float* frame_params, const double* translate, const float* boxes, const int* valid,
                                           const float* rm_boxes, const int* n_valid, const unsigned long long* seeds,
                                           const unsigned* keys, const int* plan, void* drop_ws, const float* xy_range, float* out,
                                           int* kept_off, void* workspace, void* stream) {
  GD_REQUIRE(F >= 3 && B >= 1, "gt_sample_collate: need xyz columns and at least one frame");
  GD_REQUIRE(n_rows < (1ll << 31), "gt_sample_collate: the segment table holds 32-bit rows");
  GD_REQUIRE(!plan || (drop_ws && (seeds || keys)), "gt_sample_collate_aug: a plan needs its workspace and seeds or keys");
  hipStream_t st = (hipStream_t)stream;
  if (n_rows <= 0) {
    GD_CHECK(hipMemsetAsync(kept_off, 0, sizeof(int) * (B + 1), st));
    return 0;
  }
  GD_REQUIRE(S >= 1, "gt_sample_collate: rows without a segment");
  GsLoadAug L{{{raw, db}, F, S, seg, frame_params, boxes, valid, rm_boxes, n_valid, xy_range[0], xy_range[1], xy_range[2], xy_range[3]},
              translate, GsDrop{seeds, keys, plan, plan ? gs_drop_ws(drop_ws, B).elig : nullptr}};
  GD_CHECK(hipMemsetAsync(kept_off, 0xFF, sizeof(int) * (B + 1), st));
  return gd_device_scan<int>(n_rows, L, GsStoreAug{L, out, kept_off}, kept_off + B, (int*)workspace, st);
}
