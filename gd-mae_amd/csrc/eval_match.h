// The greedy matching of the AP evaluators, written once (csrc/kitti_eval.hip; csrc/once_eval.hip): the wave64
// reductions, the first pass (which prediction a GT row takes by score), the second pass (which it takes by overlap at every score
// threshold, and what is left over as a false positive) and the sum over the chunks.  A wavefront works on one (frame, combo) at a
// time: the GT rows in order, the predictions strided over the lanes (prediction = lane + 64 * bit of a 16-bit mask per lane).  A flag
// is -1 (not of this combo), 0 (counts) or 1 (ignored: it may take or be taken, and then counts for nothing).  No atomics; lane t
// keeps threshold t; every sum runs in a fixed order.
#pragma once
#include <limits.h>

#include "common.h"

// the wavefront's (largest v, lowest index among equal v); idx INT_MAX = none
__device__ inline void em_wave_argmax(float& v, int& idx) {
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
__device__ inline int em_wave_min(int v) {
#pragma unroll
  for (int d = GD_WAVE / 2; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d, GD_WAVE));
  return v;
}
__device__ inline int em_wave_sum(int v) {
#pragma unroll
  for (int d = GD_WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, GD_WAVE);
  return v;
}

// one (frame, combo): the GT-major overlap plane (G, D), the flag rows of both sides, the scores, the combo's overlap threshold
struct EmView {
  const float* ov;
  int G, D;
  const signed char *ig, *id;
  const float* sc;
  double min_ov;
};

struct EmCounts {
  int tp = 0, fp = 0, fn = 0;
};

// a second-pass hook that does nothing: hit(g, j) per true positive, end(mine) after every threshold (mine: this lane keeps it)
struct EmNoHook {
  __device__ void hit(int, int) {}
  __device__ void end(bool) {}
};

// First pass.  Per GT row the unassigned prediction of the highest score above `sentinel` (lowest index among equals) whose overlap
// is above min_ov.  Writes every slot of matched_row (G): the true positive's score, -inf elsewhere.
__device__ inline void em_first_pass(const EmView& v, int lane, float sentinel, float* __restrict__ matched_row) {
  const int nI = (v.D + GD_WAVE - 1) / GD_WAVE;
  unsigned live = 0, assigned = 0;
  for (int i = 0; i < nI; ++i) {
    const int j = lane + GD_WAVE * i;
    if (j < v.D && v.id[j] != -1) live |= 1u << i;
  }
  for (int g = 0; g < v.G; ++g) {
    float out = -INFINITY;
    const int ign_g = v.ig[g];
    if (ign_g != -1) {
      float bs = sentinel;                                   // a score at or below it never matches
      int bj = INT_MAX;
      const unsigned m = live & ~assigned;
      for (int i = 0; i < nI; ++i)
        if ((m >> i) & 1u) {
          const int j = lane + GD_WAVE * i;
          if ((double)v.ov[(size_t)g * v.D + j] > v.min_ov && v.sc[j] > bs) {
            bs = v.sc[j];
            bj = j;
          }
        }
      em_wave_argmax(bs, bj);
      if (bj != INT_MAX) {
        if (lane == (bj & (GD_WAVE - 1))) assigned |= 1u << (bj / GD_WAVE);
        if (!(ign_g == 1 || v.id[bj] == 1)) out = bs;
      }
    }
    if (lane == 0) matched_row[g] = out;
  }
}

// Second pass on one frame for the nt thresholds of combo k (thresholds: SLOTS per combo); lane t adds threshold t to acc.
// never_fp: this lane's predictions that are not counted as false positives when no GT row takes them.
template <int SLOTS, class Hook>
__device__ inline void em_second_pass(const EmView& v, int lane, int k, const float* __restrict__ thresholds, int nt, unsigned never_fp,
                                      Hook& hook, EmCounts& acc) {
  const int nI = (v.D + GD_WAVE - 1) / GD_WAVE;
  unsigned live0 = 0, live1 = 0;                             // predictions flagged 0 / 1
  for (int i = 0; i < nI; ++i) {
    const int j = lane + GD_WAVE * i;
    if (j < v.D) {
      if (v.id[j] == 0) live0 |= 1u << i;
      if (v.id[j] == 1) live1 |= 1u << i;
    }
  }
  for (int t = 0; t < nt; ++t) {
    const float thr = thresholds[k * SLOTS + t];
    unsigned keep = 0, assigned = 0;
    for (int i = 0; i < nI; ++i) {
      const int j = lane + GD_WAVE * i;
      if (j < v.D && !(v.sc[j] < thr)) keep |= 1u << i;
    }
    const unsigned c0 = live0 & keep, c1 = live1 & keep;
    int tp = 0, fn = 0;
    for (int g = 0; g < v.G; ++g) {
      const int ign_g = v.ig[g];
      if (ign_g == -1) continue;
      // a flag-0 prediction with the largest overlap (lowest index among equals) wins; without one, the first flag-1 prediction
      float bo = -1.f;
      int bj = INT_MAX;
      unsigned m = c0 & ~assigned;
      for (int i = 0; i < nI; ++i)
        if ((m >> i) & 1u) {
          const int j = lane + GD_WAVE * i;
          const float o = v.ov[(size_t)g * v.D + j];
          if ((double)o > v.min_ov && o > bo) {
            bo = o;
            bj = j;
          }
        }
      em_wave_argmax(bo, bj);
      bool ignored_pick = false;
      if (bj == INT_MAX) {
        m = c1 & ~assigned;
        for (int i = 0; i < nI && bj == INT_MAX; ++i)
          if ((m >> i) & 1u) {
            const int j = lane + GD_WAVE * i;
            if ((double)v.ov[(size_t)g * v.D + j] > v.min_ov) bj = j;
          }
        bj = em_wave_min(bj);
        ignored_pick = true;
      }
      if (bj == INT_MAX) {
        if (ign_g == 0) ++fn;
      } else {
        if (lane == (bj & (GD_WAVE - 1))) assigned |= 1u << (bj / GD_WAVE);
        if (!(ign_g == 1 || ignored_pick)) {
          ++tp;
          hook.hit(g, bj);
        }
      }
    }
    const int fp = em_wave_sum(__popc(c0 & ~assigned & ~never_fp));
    if (lane == t) {
      acc.tp += tp;
      acc.fp += fp;
      acc.fn += fn;
    }
    hook.end(lane == t);
  }
}

// a wavefront's chunk sums of combo k: slot `lane` of part (chunks, K, SLOTS, 3)
template <int SLOTS>
__device__ inline void em_store_part(const EmCounts& acc, int lane, size_t o, int* __restrict__ part) {
  if (lane < SLOTS) {
    part[o * 3 + 0] = acc.tp;
    part[o * 3 + 1] = acc.fp;
    part[o * 3 + 2] = acc.fn;
  }
}

// (combo, threshold) i of K * SLOTS: the chunks added in order; part_s / sim (the similarity column) may both be null
template <int SLOTS>
__device__ inline void em_reduce(int i, int n_chunks, int K, const int* __restrict__ part, const double* __restrict__ part_s,
                                 long long* __restrict__ counts, double* __restrict__ sim_out) {
  if (i >= K * SLOTS) return;
  long long tp = 0, fp = 0, fn = 0;
  double sim = 0.0;
  for (int c = 0; c < n_chunks; ++c) {
    const size_t o = (size_t)c * K * SLOTS + i;
    tp += part[o * 3 + 0];
    fp += part[o * 3 + 1];
    fn += part[o * 3 + 2];
    if (part_s) sim += part_s[o];
  }
  counts[i * 3 + 0] = tp;
  counts[i * 3 + 1] = fp;
  counts[i * 3 + 2] = fn;
  if (sim_out) sim_out[i] = sim;
}
