// Anchor-head evaluation tail for the WHOLE batch in three launches: the survivors of gdmae_anchor_head_infer (count, score,
// label, box; the first count[b] rows of a sample, in anchor order) -> final boxes of all samples, padded to a shape that depends on
// the config only, nothing read on the host.  It is `Detector3DTemplate.finish_sample` made deterministic: the pre_max best rows by
// (score descending, row position ascending), rotated NMS with the bev_iou of gdmae_nms_bev, the first post_max kept boxes, rows with
// label 0 dropped behind that cut.
//
//   k_ad_select  one 1024-thread workgroup per sample.  count[b] <= pre_max: 64-bit keys (~score bits | row position) of all rows,
//                bitonic-sorted in LDS (32 KB at 4096 keys).  count[b] > pre_max: an MSB-first radix select on the score bits (8-bit
//                digits, four histogram passes over the sample's scores, LDS counters) finds the pre_max-th largest score value and how
//                many rows equal to it still fit; one more pass compacts, in input order (block prefix counts), the rows above that value
//                and the first fitting rows equal to it into the key array; then the same sort.  Sorted boxes / scores / labels and n[b]
//                go to the workspace.
//   k_ad_masks   (words, words, B) grid of 64-thread blocks, as k_cd_masks without classes: the suppression words of the pairs of one
//                row block and one column block.  Blocks below the diagonal or beyond n[b] return at once.
//   k_ad_scan    one wavefront per sample: the sequential scan with the 4096 removed bits in REGISTERS (lane w owns word w), the mask
//                rows staged 64 at a time through LDS; inside a tile only the diagonal word decides, it is read with v_readlane from
//                the lane that holds the row.  Stops when post_max boxes are kept; then the label-0 filter, the compacted rows, the zero
//                padding and num[b] in parallel.
//
// Scores are sigmoid outputs: never negative, never NaN, so the bit pattern orders them.  The position is in the key: the sort has
// no ties and the result does not depend on scheduling.  The LDS atomics only count histogram digits; no output position comes from
// an atomic.
#include "bev_iou.h"

namespace {
constexpr int kAdMax = 4096;           // NMS_PRE_MAXSIZE the LDS sort, the register bit set and the kept list are sized by
constexpr int kAdThreads = 1024;
constexpr int kAdItems = 4;            // rows per thread and step of the compaction pass
constexpr int kAdHistItems = 8;        // ... of a histogram pass
constexpr unsigned long long kAdInvalid = ~0ull;

struct AdWork {
  float* boxes;                // (B, pre_max, 7) sorted candidates that enter the NMS
  float* score;                // (B, pre_max)
  int* label;                  // (B, pre_max) 1-based, as the input
  int* n;                      // (B)
  unsigned long long* mask;    // (B, pre_max, words)
};

__global__ __launch_bounds__(kAdThreads) void k_ad_select(const int* __restrict__ count, const float* __restrict__ score,
                                                          const int* __restrict__ label, const float* __restrict__ box, int A, int pre_max,
                                                          AdWork Wk) {
  __shared__ unsigned long long keys[kAdMax];
  __shared__ unsigned hist[256];
  __shared__ int s_scan[kAdThreads / GD_WAVE + 1];
  __shared__ unsigned long long s_scan2[kAdThreads / GD_WAVE + 1];
  __shared__ unsigned s_prefix, s_remaining;
  const int b = blockIdx.x, t = threadIdx.x, lane = t & (GD_WAVE - 1);
  const long long row = (long long)b * A;
  const unsigned* sbits = (const unsigned*)score + row;
  int nc = count[b];
  nc = nc < 0 ? 0 : (nc > A ? A : nc);
  const int n = nc < pre_max ? nc : pre_max;
  if (t == 0) Wk.n[b] = n;
  if (n == 0) return;                                                // uniform
  int N = 2;
  while (N < n) N <<= 1;                                             // <= 4096
  if (nc <= pre_max) {
    for (int i = t; i < N; i += kAdThreads)
      keys[i] = i < nc ? ((unsigned long long)(~sbits[i]) << 32) | (unsigned)i : kAdInvalid;
  } else {
    // ---- the pre_max-th largest score value: prefix = its bits, remaining = how many rows equal to it are taken
    unsigned prefix = 0u, remaining = (unsigned)pre_max;
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (t < 256) hist[t] = 0u;
      __syncthreads();
      const unsigned himask = shift == 24 ? 0u : ~0u << (shift + 8);
      for (int base = 0; base < nc; base += kAdThreads * kAdHistItems) {      // uniform trip count: the ballots below see whole wavefronts
        unsigned u[kAdHistItems];
#pragma unroll
        for (int k = 0; k < kAdHistItems; ++k) {                       // the loads of a step go out together
          const int i = base + k * kAdThreads + t;
          u[k] = i < nc ? sbits[i] : 0u;
        }
#pragma unroll
        for (int k = 0; k < kAdHistItems; ++k) {
          const bool act = base + k * kAdThreads + t < nc && (u[k] & himask) == prefix;
          const unsigned d = (u[k] >> shift) & 255u;
          const unsigned long long m = __ballot(act);
          if (m) {
            // sigmoid scores share their leading bits: a wavefront whose rows all fall into one bin adds its count once
            const unsigned d0 = (unsigned)__shfl((int)d, __ffsll((long long)m) - 1, GD_WAVE);
            const unsigned long long same = __ballot(act && d == d0);
            if (same == m) {
              if (lane == __ffsll((long long)m) - 1) atomicAdd(&hist[d0], (unsigned)__popcll(m));
            } else if (act) {
              atomicAdd(&hist[d], 1u);
            }
          }
        }
      }
      __syncthreads();
      // bins in descending digit order: the bin in which the running count reaches `remaining`
      const unsigned h = t < 256 ? hist[255 - t] : 0u;                 // (counts of at most A rows: they fit an int)
      int tot;
      const unsigned ex = (unsigned)gd_block_exclusive_scan<int, kAdThreads>((int)h, tot, s_scan);
      if (t < 256 && h > 0u && ex < remaining && remaining <= ex + h) {
        s_prefix = prefix | ((unsigned)(255 - t) << shift);
        s_remaining = remaining - ex;
      }
      __syncthreads();
      prefix = s_prefix;
      remaining = s_remaining;
      __syncthreads();
    }
    const unsigned cut = prefix, need = remaining, above = (unsigned)pre_max - need;
    // ---- rows above the cut value and the first `need` rows equal to it, in input order
    unsigned long long carry = 0ull;                                 // rows above the cut << 32 | rows equal to it, before this step
    for (int base = 0; base < nc; base += kAdThreads * kAdItems) {
      unsigned u[kAdItems];
      unsigned long long v = 0ull;
#pragma unroll
      for (int k = 0; k < kAdItems; ++k) {
        const int i = base + t * kAdItems + k;
        u[k] = i < nc ? sbits[i] : 0u;
        if (i < nc) v += u[k] > cut ? 1ull << 32 : (u[k] == cut ? 1ull : 0ull);
      }
      unsigned long long tot;
      unsigned long long run = gd_block_exclusive_scan<unsigned long long, kAdThreads>(v, tot, s_scan2) + carry;
#pragma unroll
      for (int k = 0; k < kAdItems; ++k) {
        const int i = base + t * kAdItems + k;
        if (i >= nc) break;
        const unsigned g = (unsigned)(run >> 32), e = (unsigned)run;
        const bool gt = u[k] > cut, eq = u[k] == cut;
        if (gt || (eq && e < need)) {
          const unsigned slot = g + (e < need ? e : need);
          if (slot < (unsigned)pre_max) keys[slot] = ((unsigned long long)(~u[k]) << 32) | (unsigned)i;
        }
        run += gt ? 1ull << 32 : (eq ? 1ull : 0ull);
      }
      carry += tot;
      if ((unsigned)(carry >> 32) == above && (unsigned)carry >= need) break;      // uniform: all pre_max rows are placed
    }
    for (int i = pre_max + t; i < N; i += kAdThreads) keys[i] = kAdInvalid;
  }
  __syncthreads();
  // bitonic sort, ascending: N / 2 compare-exchanges per step
  for (int k = 2; k <= N; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = t; p < (N >> 1); p += kAdThreads) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const int l = i + j;
        const unsigned long long x = keys[i], y = keys[l];
        const bool up = (i & k) == 0;
        if ((x > y) == up) { keys[i] = y; keys[l] = x; }
      }
      __syncthreads();
    }
  const long long wrow = (long long)b * pre_max;
  for (int p = t; p < n; p += kAdThreads) {
    const unsigned long long key = keys[p];
    if ((unsigned)key >= (unsigned)nc) continue;                     // (never: every key below n holds a position < nc <= A)
    const long long i = row + (long long)(unsigned)key;
    for (int e = 0; e < 7; ++e) Wk.boxes[(wrow + p) * 7 + e] = box[i * 7 + e];
    Wk.score[wrow + p] = __uint_as_float(~(unsigned)(key >> 32));
    Wk.label[wrow + p] = label[i];
  }
}

// mask[b][i][cb] bit j: box (64 cb + j) > i overlaps box i beyond the threshold
__global__ __launch_bounds__(64) void k_ad_masks(int K, int words, float thr, AdWork Wk) {
  __shared__ float cols[64 * 7];
  const int b = blockIdx.z, rb = blockIdx.y, cb = blockIdx.x, t = threadIdx.x;
  const int n = Wk.n[b];
  const int nw = (n + 63) >> 6;
  if (rb >= nw || cb >= nw || cb < rb) return;                       // uniform: the scan reads words [row >> 6, nw) of rows < n only
  const long long row = (long long)b * K;
  const int cn = min(64, n - cb * 64), rn = min(64, n - rb * 64);
  if (t < cn) {
    const float* src = Wk.boxes + (row + cb * 64 + t) * 7;
    for (int e = 0; e < 7; ++e) cols[t * 7 + e] = src[e];
  }
  __syncthreads();
  if (t >= rn) return;
  const int i = rb * 64 + t;
  float bi[7];
  for (int e = 0; e < 7; ++e) bi[e] = Wk.boxes[(row + i) * 7 + e];
  const float hi = 0.5f * sqrtf(bi[3] * bi[3] + bi[4] * bi[4]);
  unsigned long long w = 0ull;
  for (int j = cb == rb ? t + 1 : 0; j < cn; ++j) {
    const float* bj = cols + j * 7;
    // exact pre-reject, as in k_cd_masks: every point of the intersection polygon is an edge crossing or a corner of one box within
    // the other's extent + 1e-2 (bev_iou.h), so centres farther apart than the half-diagonals + 0.05 give no point, an overlap of 0
    // and a bit of 0 for any threshold >= 0.  (inf / NaN sizes compare false and take the full test.)
    const float dx = bi[0] - bj[0], dy = bi[1] - bj[1];
    const float reach = hi + 0.5f * sqrtf(bj[3] * bj[3] + bj[4] * bj[4]) + 0.05f;
    if (dx * dx + dy * dy > reach * reach) continue;
    if (bev_iou(bi, bj) > thr) w |= 1ull << j;
  }
  Wk.mask[(row + i) * words + cb] = w;
}

__device__ __forceinline__ unsigned long long ad_readlane(unsigned long long v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(64) void k_ad_scan(int K, int words, int n_out, AdWork Wk, float* __restrict__ boxes, float* __restrict__ scores,
                                                long long* __restrict__ labels, int* __restrict__ num) {
  __shared__ unsigned long long tile[64][65];                        // tile[r][j]: word tb + j of row 64 tb + r
  __shared__ int kept[kAdMax];
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long row = (long long)b * K;
  const int n = Wk.n[b];
  const int nw = (n + 63) >> 6;
  unsigned long long mine = 0ull;                                    // removed bits of the boxes 64 lane .. 64 lane + 63
  int cnt = 0;
  for (int tb = 0; tb < nw && cnt < n_out; ++tb) {                   // n_out = min(pre_max, post_max) and cnt <= n <= pre_max
    const int nwc = nw - tb, rn = min(64, n - tb * 64);
    __syncthreads();
    if (lane < nwc) {
      const unsigned long long* src = Wk.mask + (row + tb * 64) * words + tb + lane;
      for (int r = 0; r < rn; ++r) tile[r][lane] = src[(long long)r * words];
    }
    __syncthreads();
    const unsigned long long diag = lane < rn ? tile[lane][0] : 0ull;
    unsigned long long cur = ad_readlane(mine, tb);                   // uniform: the removed bits of this tile's boxes
    for (int r = 0; r < rn && cnt < n_out; ++r) {
      if ((cur >> r) & 1ull) continue;
      if (lane == 0) kept[cnt] = tb * 64 + r;
      ++cnt;
      cur |= ad_readlane(diag, r);
      if (lane >= tb && lane < nw) mine |= tile[r][lane - tb];
    }
  }
  __syncthreads();
  // rows with label 0 leave behind the post_max cut (they suppressed and took their place); the list stays in scan order
  int out = 0;
  for (int base = 0; base < cnt; base += 64) {
    const int k = base + lane;
    const int src = k < cnt ? kept[k] : 0;
    const bool ok = k < cnt && Wk.label[row + src] != 0;
    const unsigned long long m = __ballot(ok);
    __syncthreads();
    if (ok) kept[out + __popcll(m & ((1ull << lane) - 1ull))] = src;
    out += __popcll(m);
    __syncthreads();
  }
  for (int k = lane; k < n_out; k += 64) {
    const long long o = (long long)b * n_out + k;
    if (k < out) {
      const long long s = row + kept[k];
      for (int e = 0; e < 7; ++e) boxes[o * 7 + e] = Wk.boxes[s * 7 + e];
      scores[o] = Wk.score[s];
      labels[o] = (long long)Wk.label[s];
    } else {
      for (int e = 0; e < 7; ++e) boxes[o * 7 + e] = 0.f;
      scores[o] = 0.f;
      labels[o] = 0;
    }
  }
  if (lane == 0) num[b] = out;
}

size_t ad_layout(int B, int pre_max, void* ws, AdWork* Wk) {
  const size_t words = (size_t)(pre_max + 63) / 64, rows = (size_t)B * pre_max;
  GdArena A(ws, ~(size_t)0);
  float* boxes = A.take<float>(rows * 7);
  float* score = A.take<float>(rows);
  int* label = A.take<int>(rows);
  int* n = A.take<int>((size_t)B);
  unsigned long long* mask = A.take<unsigned long long>(rows * words);
  if (Wk) *Wk = AdWork{boxes, score, label, n, mask};
  return A.off;
}
}  // namespace

extern "C" size_t gdmae_anchor_detect_workspace_bytes(int B, int pre_max) {
  if (B < 1 || pre_max < 1 || pre_max > kAdMax) return 0;
  return ad_layout(B, pre_max, nullptr, nullptr);
}

// see include/gdmae_hip.h
extern "C" int gdmae_anchor_detect(const int* count, const float* score, const int* label, const float* box, int B, int A, int pre_max,
                                   int post_max, float nms_thresh, int n_out, float* boxes, float* scores, long long* labels, int* num,
                                   void* workspace, void* stream) {
  GD_REQUIRE(B >= 1 && A >= 1, "anchor_detect: bad sizes");
  GD_REQUIRE(pre_max >= 1 && pre_max <= kAdMax, "anchor_detect: NMS_PRE_MAXSIZE outside 1 .. 4096 (the sort and the bit set live on chip)");
  GD_REQUIRE(post_max >= 1, "anchor_detect: NMS_POST_MAXSIZE below 1");
  GD_REQUIRE(nms_thresh >= 0.f, "anchor_detect: negative NMS threshold");          // (a NaN is refused as well)
  GD_REQUIRE(n_out == (pre_max < post_max ? pre_max : post_max), "anchor_detect: n_out is not min(NMS_PRE_MAXSIZE, NMS_POST_MAXSIZE)");
  GD_REQUIRE(count && score && label && box && boxes && scores && labels && num && workspace, "anchor_detect: null argument");
  AdWork Wk;
  ad_layout(B, pre_max, workspace, &Wk);
  const int words = (pre_max + 63) / 64;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ad_select, dim3(B), dim3(kAdThreads), 0, st, count, score, label, box, A, pre_max, Wk);
  GD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ad_masks, dim3(words, words, B), dim3(64), 0, st, pre_max, words, nms_thresh, Wk);
  GD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ad_scan, dim3(B), dim3(64), 0, st, pre_max, words, n_out, Wk, boxes, scores, labels, num);
  GD_LAUNCH_CHECK();
  return 0;
}
