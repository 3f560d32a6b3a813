// DynVFE second point layer + per-pillar maximum without its (N, 128) intermediates (reference
// pcdet/models/backbones_3d/vfe/dyn_vfe.py:107-112, network_utils.py:7-21:  h = y1 W^T (64 -> 128),
// v = relu(BatchNorm1d_train(h)), pillar feature = max of v over the pillar's points [torch_scatter.scatter_max]).
//
// 16-bit throughput mode only (y1 is the bf16 - or, round 6, fp16 - output of gdmae_vfe_point_layer_fwd; the fp32 parity mode keeps the
// op-by-op path).  F16 instantiations (gdmae_vfe_max_layer_*_f16): y1 holds fp16 values and W arrives as the fp32 master matrix, rounded
// to fp16 for the pre-activation h = y1 W^T (v_mfma_f32_32x32x16_f16) and to bf16 for the gradient product dy1 = dx W; y1^T is converted
// to bf16 when k_v2_dydw stages it.  Why: the pillar maximum passes ONE point's value on - the rounding of y1 and of W does not average
// over a pillar's points - and DynVFE in bf16 was the largest term of config E's small-case loss scatter.  h (N x 128, 366 MB in bf16 for an 8-frame batch) is never stored: a 32-point tile of it is
// 16 v_mfma_f32_32x32x16_bf16 from a 4 KB tile of y1, so every kernel below recomputes it in accumulators:
//   forward   k_v2_stats  : column sums of h, h^2 (fp32 accumulators)  -> gd_bn_fold_from_partials
//             k_v2_max    : tiles in pillar (CSR) order; the tile goes through LDS and each lane walks one column
//   (see k_v2_max below)    a pillar is closed whenever the pillar id changes -> out, arg
//   backward  k_v2_gstats : gm = g [out > 0], column sums of gm, gm*h(arg) with h(arg) = (out - b) / a
//             k_v2_dydw   : dx = a dh + c0 + c1 h  (dh = gm at the arg-max point), once per tile, feeds both products:
//                           dy1 = dx W (dx through a shared LDS tile) and dW^T += y1^T dx (the dx accumulators are the B
//                           operand, y1^T comes from a transposed LDS tile; per-workgroup partials, fixed-order reduction)
// Accumulator layout of v_mfma_f32_32x32x16: lane (n = lane % 32, half = lane / 32) holds column n, register r holds
// row (r & 3) + 8 (r >> 2) + 4 half.
#include "common.h"
#include "gemm.h"

int gd_bn_fold_from_partials(hipStream_t st, const float* part, int nblk, int C, double count, const float* gamma,
                             const float* beta, double eps, double momentum, float* running_mean, float* running_var,
                             long long* num_batches, double* stats, float* ab, float* mv);
int gd_partials_to_f64(hipStream_t st, const float* part, int nblk, int C2, double* out);
extern "C" int gdmae_bn_bwd_coeffs(const double* st, int n_st, const double* stats, const float* ab, const float* gamma, int C,
                                   double count, const double* tot, float* dgamma, float* dbeta, int accumulate, float* c01,
                                   void* stream);

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
union V2Frag {
  uint4 u;
  uint2 u2[2];
  bf16x8 v;
  f16x8 hv;
  unsigned short s[8];
};

constexpr int V2_CI = 64, V2_CO = 128;
constexpr int V2_WAVES = 4;
constexpr int V2_LDW = V2_CI + 8;     // bf16 elements per row of the W tile (128 x 64) in LDS
constexpr int V2_LDX = V2_CO + 8;     // ... of the dx tile (32 x 128) and of W^T (64 x 128)
constexpr int V2_LDT = 32 + 8;        // ... of the transposed y1 tile (64 x 32)
constexpr int V2_MAX_GRID = 1024;     // rows of the statistics partials
constexpr int V2_DW_GRID = 1024;      // rows of the dW partials (32 KB each)
constexpr int V2_MAXW_GRID = 2048;    // workgroups of k_v2_max (8 workers each; their boundary slots share the dW partial area)
static_assert((size_t)V2_MAXW_GRID * 8 * 2 * 128 * 8 <= (size_t)V2_DW_GRID * 128 * 64 * 4, "boundary slots fit the partial area");

__device__ __forceinline__ int v2_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }
__device__ __forceinline__ unsigned short v2_f2bf(float f) { return gd_to_bf16(f); }
__device__ __forceinline__ f32x16 v2_mfma(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ bf16x8 v2_pack(const f32x16& a, int r0) {   // 8 accumulator registers -> bf16 fragment
  f32x8 t;
#pragma unroll
  for (int j = 0; j < 8; ++j) t[j] = a[r0 + j];
  return __builtin_convertvector(t, bf16x8);
}

// W (128, 64) -> LDS, rows padded to V2_LDW.  F16: W is the fp32 master matrix, rounded to fp16 here; else bf16, copied
template <bool F16>
__device__ __forceinline__ void v2_load_w(const void* __restrict__ Wv, unsigned short* __restrict__ sW) {
  for (int q = threadIdx.x; q < V2_CO * (V2_CI / 8); q += V2_WAVES * 64) {
    const int row = q >> 3, ch = q & 7;
    if constexpr (F16) {
      const float* W = (const float*)Wv + row * V2_CI + 8 * ch;
      const float4 a = *reinterpret_cast<const float4*>(W), b = *reinterpret_cast<const float4*>(W + 4);
      uint4 o;
      o.x = gd_pack_f16(a.x, a.y); o.y = gd_pack_f16(a.z, a.w); o.z = gd_pack_f16(b.x, b.y); o.w = gd_pack_f16(b.z, b.w);
      *reinterpret_cast<uint4*>(sW + row * V2_LDW + 8 * ch) = o;
    } else {
      *reinterpret_cast<uint4*>(sW + row * V2_LDW + 8 * ch) = *reinterpret_cast<const uint4*>((const unsigned short*)Wv + row * V2_CI + 8 * ch);
    }
  }
}

// A fragments of h = y1 W^T for tile row `row` (this lane: columns 16 s + 8 half .. + 8 of that row); zero when !live
__device__ __forceinline__ void v2_load_y(const unsigned short* __restrict__ y1, long long row, bool live, int half,
                                          V2Frag (&ya)[4]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    ya[s].u = *reinterpret_cast<const uint4*>(y1 + row * V2_CI + 16 * s + 8 * half);
    if (!live) ya[s].u = make_uint4(0, 0, 0, 0);
  }
}
// the same in two steps for software-pipelined loops: the loads now, the clearing of a dead row where the fragments are first needed
// (a select right behind the load waits for it there, and a prefetch "in flight behind the arithmetic" is drained before it starts)
__device__ __forceinline__ void v2_load_y_raw(const unsigned short* __restrict__ y1, long long row, int half, V2Frag (&ya)[4]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) ya[s].u = *reinterpret_cast<const uint4*>(y1 + row * V2_CI + 16 * s + 8 * half);
}
__device__ __forceinline__ void v2_keep_y(V2Frag (&ya)[4], bool live) {
  const unsigned m = live ? 0xFFFFFFFFu : 0u;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    ya[s].u.x &= m; ya[s].u.y &= m; ya[s].u.z &= m; ya[s].u.w &= m;
    asm volatile("" : "+v"(ya[s].u.x), "+v"(ya[s].u.y), "+v"(ya[s].u.z), "+v"(ya[s].u.w));      // here, not where the compiler would sink it
  }
}

// pillar id and A fragments of this lane's row (n) of tile t
__device__ __forceinline__ void v2_load_tile(const unsigned short* __restrict__ y1, const int* __restrict__ rowpil, long long t,
                                             long long N, int n, int half, V2Frag (&ya)[4], int& pil) {
  const bool live = t * 32 + n < N;
  const long long row = live ? t * 32 + n : N - 1;
  pil = rowpil[row];
  v2_load_y(y1, row, live, half, ya);
}

// h[:, 32 b + n] for the tile: D[i = row][j = column] = sum_k y1[row][k] W[column][k]
template <bool F16>
__device__ __forceinline__ f32x16 v2_h(const V2Frag (&ya)[4], const unsigned short* __restrict__ sW, int n, int half, int b) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    V2Frag w;
    w.u = *reinterpret_cast<const uint4*>(sW + (32 * b + n) * V2_LDW + 16 * s + 8 * half);
    if constexpr (F16) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ya[s].hv, w.hv, acc, 0, 0, 0);
    else acc = v2_mfma(ya[s].v, w.v, acc);
  }
  return acc;
}

// ---- forward statistics --------------------------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(V2_WAVES * 64) void k_v2_stats(const unsigned short* __restrict__ y1, long long N,
                                                            const void* __restrict__ W, float* __restrict__ part) {
  __shared__ unsigned short sW[V2_CO * V2_LDW];
  __shared__ float sR[V2_WAVES * 2 * V2_CO];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 31, half = lane >> 5;
  v2_load_w<F16>(W, sW);
  __syncthreads();
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  const long long ntiles = (N + 31) / 32;
  for (long long t = (long long)blockIdx.x * V2_WAVES + wave; t < ntiles; t += (long long)gridDim.x * V2_WAVES) {
    const long long row = t * 32 + n;
    V2Frag ya[4];
    v2_load_y(y1, row < N ? row : N - 1, row < N, half, ya);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const f32x16 h = v2_h<F16>(ya, sW, n, half, b);   // rows past N are exactly zero
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s1[b] += h[r];
        s2[b] = fmaf(h[r], h[r], s2[b]);
      }
    }
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    s1[b] += __shfl_xor(s1[b], 32, 64);
    s2[b] += __shfl_xor(s2[b], 32, 64);
    if (half == 0) {
      sR[wave * 2 * V2_CO + 32 * b + n] = s1[b];
      sR[wave * 2 * V2_CO + V2_CO + 32 * b + n] = s2[b];
    }
  }
  __syncthreads();
  {
    float a = 0.f;
#pragma unroll
    for (int w = 0; w < V2_WAVES; ++w) a += sR[w * 2 * V2_CO + threadIdx.x];
    part[(long long)blockIdx.x * 2 * V2_CO + threadIdx.x] = a;
  }
}

// ---- forward maximum -----------------------------------------------------------------------------------------
// Every half-wave is a worker with its own contiguous range of `per` rows - the SAME number of rows for every worker, wherever the
// pillar boundaries fall (ranges snapped to pillar starts gave a crowded pillar - 1 000 points next to the sensor against 11 on
// average - to one half-wave as a serial chain of 68 tiles: 118 of the launch's 174 us did not scale with the batch).  A 32-row MFMA
// tile holds 16 rows of each worker, permuted so that a lane's 16 accumulator registers are 16 CONSECUTIVE rows of its worker:
// MFMA row i = (r & 3) + 8 (r >> 2) + 4 h  <->  worker h, local row r.  Each lane then walks its registers in row order, closing a
// pillar (three coalesced 128-byte stores per column block) whenever the pillar id changes - no LDS, no atomics.  A pillar that lies
// inside the range goes straight to out / arg; the piece of a pillar that began before the range goes to the worker's boundary slot
// 0, the piece of one that continues behind it to slot 1 (a range inside one pillar: slot 0), and k_v2_max_fix joins the pieces of
// such a pillar in row order.  arg = row of the maximum (strict >: the first row, i.e. the lowest point id, wins ties - (max value,
// min row) is associative, so joining pieces in order gives the sequential walk's answer bit for bit).
// VIS (the pre-training step with a prefetched, masked plan): the walk runs over the COMPACT rows [0, N) of the visible pillars only -
// compact row rc is y1 row vis_rows[rc], rowpil[rc] is its stage-1 token, out / arg are (tokens, 128).  The rows of a token are
// contiguous in both row spaces, so the real row k_v2_dydw compares arg against is the compact one plus vis_rows[rc] - rc of any row of
// the pillar: added where a pillar (or a piece of one) is stored - one more load behind the rarely taken branch, no register per
// accumulator.
template <bool F16, bool VIS>
__global__ __launch_bounds__(V2_WAVES * 64) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_v2_max(const unsigned short* __restrict__ y1, long long N,
                                                          const void* __restrict__ W, const int* __restrict__ vis_rows,
                                                          const int* __restrict__ rowpil, int M, const float* __restrict__ ab,
                                                          float* __restrict__ out, int* __restrict__ arg, long long per,
                                                          float* __restrict__ pbest, int* __restrict__ parg) {
  __shared__ unsigned short sW[V2_CO * V2_LDW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 31, half = lane >> 5;
  v2_load_w<F16>(W, sW);
  __syncthreads();
  // this worker's share of the rows; head: its first pillar began before the range, tail: its last pillar continues behind it
  const int wk = (blockIdx.x * V2_WAVES + wave) * 2 + half;      // (int, and the slot offsets recomputed where used: 162 registers = 3 waves per SIMD)
  const long long qa = (long long)wk * per < N ? (long long)wk * per : N, qb = (long long)(wk + 1) * per < N ? (long long)(wk + 1) * per : N;
  const int q0 = (int)qa, q1 = (int)qb;
  bool hp, tail;
  {
    const long long ia = qa > 0 ? qa - 1 : 0, ib = qa < N ? qa : N - 1, ic = qb > 0 ? qb - 1 : 0, id = qb < N ? qb : N - 1;
    const int a0 = rowpil[ia], a1 = rowpil[ib], b0 = rowpil[ic], b1 = rowpil[id];     // four independent loads
    hp = qa > 0 && qa < qb && a0 == a1;
    tail = qb < N && qa < qb && b0 == b1;
  }
  // the tile row this lane loads as MFMA row n: worker (n >> 2) & 1, local row (n & 3) + 4 (n >> 3)
  const int ld_wk = (n >> 2) & 1, ld_r = (n & 3) + 4 * (n >> 3);
  const int q0o = __shfl(q0, lane ^ 32, 64), q1o = __shfl(q1, lane ^ 32, 64);
  const int lq0 = ld_wk == half ? q0 : q0o, lq1 = ld_wk == half ? q1 : q1o;   // range of the worker whose row this lane loads
  const int len = q1 - q0, leno = q1o - q0o;
  const int iters = ((len > leno ? len : leno) + 15) / 16;                      // wave-uniform
  float ca[4], cb[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    ca[b] = ab[32 * b + n];
    cb[b] = ab[V2_CO + 32 * b + n];
  }
  float best[4];
  int bi[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) { best[b] = -1.f; bi[b] = 0; }
  int cur = -1;

  V2Frag ya[4], yn[4];
  int pl = 0, pln = 0;                            // pillar of the row this lane loads
  {
    const int row = lq0 + ld_r;
    const bool live = row < lq1;
    const int rc = live ? row : (lq1 > 0 ? lq1 - 1 : 0);
    pl = rowpil[rc];
    v2_load_y(y1, VIS ? vis_rows[rc] : rc, live, half, ya);
  }
  for (int it = 0; it < iters; ++it) {
    const int qt = q0 + 16 * it;                 // first row of this worker's 16-row slice
    const int nrows = q1 - qt < 16 ? (q1 - qt > 0 ? q1 - qt : 0) : 16;
    bool live_n;
    {                                            // next tile: in flight during this tile's products (unconditional: past the
      const int row = lq0 + 16 * (it + 1) + ld_r;      // worker's last slice the clamped row is re-read and cleared)
      live_n = row < lq1;
      const int rc = live_n ? row : (lq1 > 0 ? lq1 - 1 : 0);
      pln = rowpil[rc];
      v2_load_y_raw(y1, VIS ? vis_rows[rc] : rc, half, yn);
    }
    __builtin_amdgcn_sched_barrier(0);           // the loads go out first
    int prow[16];                                // pillar of each of this worker's rows (uniform within the half-wave)
#pragma unroll
    for (int r = 0; r < 16; ++r) prow[r] = __shfl(pl, v2_row(r, half), 64);   // the lane that loaded this worker's row r
    // st[r]: row r opens a new pillar.  The walk itself is branch-free (selects); only the stores that close a pillar
    // sit behind a (rarely taken) branch.
    bool st[16];
    st[0] = nrows > 0 && prow[0] != cur;
#pragma unroll
    for (int r = 1; r < 16; ++r) st[r] = r < nrows && prow[r] != prow[r - 1];
    const int cur_in = cur;
#pragma unroll
    for (int r = 0; r < 16; ++r) cur = r < nrows ? prow[r] : cur;
    f32x16 h[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) h[b] = v2_h<F16>(ya, sW, n, half, b);
    // the next tile is waited for HERE, before this tile's stores go out: loads and stores retire out of order with respect to each
    // other, so once stores are pending any wait for a load is a full drain of both
    v2_keep_y(yn, live_n);
    asm volatile("" : "+v"(pln));
    if (st[0] && cur_in >= 0) {                  // the pillar carried over from the previous tile ends here
      float* const ob = hp ? pbest : out;
      int* const oa = hp ? parg : arg;
      const long long o0 = (long long)(hp ? wk * 2 : cur_in) * V2_CO;
      const int ro = VIS ? vis_rows[qt - 1] - (qt - 1) : 0;      // (cur_in >= 0: the worker has walked row qt - 1)
      hp = false;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        ob[o0 + 32 * b + n] = best[b];
        oa[o0 + 32 * b + n] = bi[b] + ro;
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float bin = st[r] ? -1.f : best[b];
        const float v = fmaxf(fmaf(ca[b], h[b][r], cb[b]), 0.f);
        const bool up = r < nrows && v > bin;    // strict: the first row of a pillar (lowest point id) wins ties
        best[b] = up ? v : bin;
        bi[b] = up ? qt + r : bi[b];
      }
      if (r < 15 && st[r < 15 ? r + 1 : 15]) {   // row r closes its pillar: one branch for the four column blocks
        float* const ob = hp ? pbest : out;
        int* const oa = hp ? parg : arg;
        const long long o0 = (long long)(hp ? wk * 2 : prow[r]) * V2_CO;
        const int ro = VIS ? vis_rows[qt + r] - (qt + r) : 0;
        hp = false;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          ob[o0 + 32 * b + n] = best[b];
          oa[o0 + 32 * b + n] = bi[b] + ro;
        }
      }
    }
    pl = pln;
#pragma unroll
    for (int s = 0; s < 4; ++s) ya[s] = yn[s];
  }
  if (cur >= 0) {                                // the range's last pillar: whole (out), first piece (slot 1) or a later piece (slot 0)
    float* const ob = hp || tail ? pbest : out;
    int* const oa = hp || tail ? parg : arg;
    const long long o0 = (long long)(hp ? wk * 2 : (tail ? wk * 2 + 1 : cur)) * V2_CO;
    const int ro = VIS ? vis_rows[q1 - 1] - (q1 - 1) : 0;        // (cur >= 0: the range is not empty)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      ob[o0 + 32 * b + n] = best[b];
      oa[o0 + 32 * b + n] = bi[b] + ro;
    }
  }
}

// joins the pieces of every pillar that crosses a range boundary of k_v2_max: one workgroup per worker; the worker in whose range
// the pillar BEGINS (its slot 1) walks the following workers' slot 0 pieces in row order until the pillar ends.  Chains are one
// piece long except for crowded pillars (points / per pieces).
__global__ __launch_bounds__(V2_CO) void k_v2_max_fix(const int* __restrict__ rowpil, long long N, long long per,
                                                      const float* __restrict__ pbest, const int* __restrict__ parg,
                                                      float* __restrict__ out, int* __restrict__ arg) {
  const long long w = blockIdx.x;
  const int c = threadIdx.x;
  const long long qa = w * per < N ? w * per : N, qb = (w + 1) * per < N ? (w + 1) * per : N;
  if (qa >= qb || qb >= N) return;
  const int P = rowpil[qb - 1];
  if (rowpil[qb] != P) return;                        // the last pillar ends with the range
  if (qa > 0 && rowpil[qa - 1] == P) return;          // it began before this range: the chain belongs to an earlier worker
  float bv = pbest[(w * 2 + 1) * V2_CO + c];
  int bi = parg[(w * 2 + 1) * V2_CO + c];
  for (long long v = w + 1;; ++v) {
    const float pv = pbest[(v * 2) * V2_CO + c];
    const int pi = parg[(v * 2) * V2_CO + c];
    const bool up = pv > bv;                           // strict: the earlier piece keeps ties
    bv = up ? pv : bv;
    bi = up ? pi : bi;
    const long long vb = (v + 1) * per < N ? (v + 1) * per : N;
    if (vb >= N || rowpil[vb] != P) break;
  }
  out[(long long)P * V2_CO + c] = bv;
  arg[(long long)P * V2_CO + c] = bi;
}

// ---- backward: masked gradient and its column sums ---------------------------------------------------------------
// the pre-activation at the arg-max row is recovered from the stored maximum, h = (out - b) / a (out > 0 there, so the
// ReLU was the identity; a = 0 only for gamma = 0, where the sum it feeds is multiplied by gamma anyway)
__global__ __launch_bounds__(256) void k_v2_gstats(const float* __restrict__ out, const float* __restrict__ ab,
                                                   const float* __restrict__ g, long long M, float* __restrict__ gm,
                                                   float* __restrict__ part) {
  // round 5: four channels (16 bytes) per thread, eight pillar rows per workgroup pass, four rows of each array in flight per thread
  // (4-byte accesses left this 200 MB stream at SQ_WAIT_ANY 0.94 / 3.4 TB/s)
  __shared__ float sR[8 * 2 * V2_CO];
  const int tr = threadIdx.x >> 5, c4 = (threadIdx.x & 31) * 4;
  const long long chunk = (M + gridDim.x - 1) / gridDim.x;
  const long long r0 = blockIdx.x * chunk, r1 = r0 + chunk < M ? r0 + chunk : M;
  float s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f};
  const float4 a4 = *reinterpret_cast<const float4*>(ab + c4), b4 = *reinterpret_cast<const float4*>(ab + V2_CO + c4);
  const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
  float ia[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) ia[e] = av[e] != 0.f ? 1.f / av[e] : 0.f;
  for (long long p0 = r0 + tr; p0 < r1; p0 += 32) {
    float4 ov[4], gv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {                    // unconditional (clamped row), masked below
      const long long p = p0 + 8 * u < r1 ? p0 + 8 * u : r1 - 1;
      ov[u] = *reinterpret_cast<const float4*>(out + p * V2_CO + c4);
      gv[u] = *reinterpret_cast<const float4*>(g + p * V2_CO + c4);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (p0 + 8 * u < r1) {
        const float o[4] = {ov[u].x, ov[u].y, ov[u].z, ov[u].w}, gg[4] = {gv[u].x, gv[u].y, gv[u].z, gv[u].w};
        float m[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          m[e] = o[e] > 0.f ? gg[e] : 0.f;
          s0[e] += m[e];
          s1[e] = fmaf(m[e], (o[e] - bv[e]) * ia[e], s1[e]);
        }
        *reinterpret_cast<float4*>(gm + (p0 + 8 * u) * V2_CO + c4) = make_float4(m[0], m[1], m[2], m[3]);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    sR[(tr * 2 + 0) * V2_CO + c4 + e] = s0[e];
    sR[(tr * 2 + 1) * V2_CO + c4 + e] = s1[e];
  }
  __syncthreads();
  {
    const int q = threadIdx.x;   // 256 = 2 * V2_CO: (statistic, channel)
    float a = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) a += sR[t * 2 * V2_CO + q];
    part[(long long)blockIdx.x * 2 * V2_CO + q] = a;
  }
}

// first index i of the ascending a[0 .. n) with a[i] >= key (n if none): 64 probes per round instead of one - three dependent loads
// for 32 k tokens where a binary search makes fifteen.  Invariant: the answer lies in [lo, lo + len], a[lo + len] >= key (or is the end).
__device__ __forceinline__ int v2_lower_bound_wave(const int* __restrict__ a, int n, int key, int lane) {
  int lo = 0, len = n;
  while (len > 0) {
    const int step = (len + 63) >> 6, idx = lo + lane * step;
    const int v = idx < lo + len ? a[idx] : 0x7FFFFFFF;
    const unsigned long long ge = __ballot(v >= key);
    const int first = ge ? __ffsll((long long)ge) - 1 : 64;
    if (first == 0) break;                               // a[lo] >= key
    const int nlo = lo + (first - 1) * step + 1, nend = lo + first * step < lo + len ? lo + first * step : lo + len;
    lo = nlo;
    len = nend - nlo;
  }
  return lo;
}

// k_v2_gstats on the rows of the visible pillars only: out / g / gm are (tokens, 128), tok_pillar (ascending) names each token's
// pillar.  Same grid, same pillar chunk per workgroup, and a visible pillar p is added by thread-row (p - r0) & 7 in ascending p -
// the thread and the order that add it in k_v2_gstats.  What that kernel adds for a masked pillar is m = +0 (its gradient row is
// zero): s + 0 = s and fmaf(0, x, s) = s exactly for finite x (a sum that starts at +0 never becomes -0), so every partial row is the
// same bits.  Each half-wave finds its tokens among 32 at a time with a ballot and keeps four rows of each array in flight.
__global__ __launch_bounds__(256) void k_v2_gstats_vis(const float* __restrict__ out, const float* __restrict__ ab,
                                                       const float* __restrict__ g, long long M, const int* __restrict__ tok_pillar,
                                                       int n_tok, float* __restrict__ gm, float* __restrict__ part) {
  __shared__ float sR[8 * 2 * V2_CO];
  __shared__ int sTok[2];
  const int tr = threadIdx.x >> 5, l = threadIdx.x & 31, c4 = l * 4;
  const long long chunk = (M + gridDim.x - 1) / gridDim.x;
  const long long r0 = blockIdx.x * chunk, r1 = r0 + chunk < M ? r0 + chunk : M;
  if (threadIdx.x < 128) {                             // waves 0 / 1: first token at or behind r0 / r1
    const int w = threadIdx.x >> 6;
    const int t = v2_lower_bound_wave(tok_pillar, n_tok, (int)(w == 0 ? r0 : (r1 > r0 ? r1 : r0)), threadIdx.x & 63);
    if ((threadIdx.x & 63) == 0) sTok[w] = t;
  }
  __syncthreads();
  const int t0 = sTok[0], t1 = sTok[1];
  float s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f};
  const float4 a4 = *reinterpret_cast<const float4*>(ab + c4), b4 = *reinterpret_cast<const float4*>(ab + V2_CO + c4);
  const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
  float ia[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) ia[e] = av[e] != 0.f ? 1.f / av[e] : 0.f;
  for (int tb = t0; tb < t1; tb += 32) {
    const int t = tb + l;
    const int p = tok_pillar[t < t1 ? t : t1 - 1];
    const bool mine = t < t1 && ((p - (int)r0) & 7) == tr;
    const unsigned long long bal = __ballot(mine);
    unsigned m = (unsigned)(bal >> (32 * (tr & 1)));   // this half-wave's tokens among the 32, ascending
    while (m) {
      int tk[4];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        ok[u] = m != 0u;
        tk[u] = ok[u] ? tb + __ffs((int)m) - 1 : tb;   // unconditional loads (a valid row), masked below
        m &= m - 1u;
      }
      float4 ov[4], gv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        ov[u] = *reinterpret_cast<const float4*>(out + (long long)tk[u] * V2_CO + c4);
        gv[u] = *reinterpret_cast<const float4*>(g + (long long)tk[u] * V2_CO + c4);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (ok[u]) {
          const float o[4] = {ov[u].x, ov[u].y, ov[u].z, ov[u].w}, gg[4] = {gv[u].x, gv[u].y, gv[u].z, gv[u].w};
          float mm[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            mm[e] = o[e] > 0.f ? gg[e] : 0.f;
            s0[e] += mm[e];
            s1[e] = fmaf(mm[e], (o[e] - bv[e]) * ia[e], s1[e]);
          }
          *reinterpret_cast<float4*>(gm + (long long)tk[u] * V2_CO + c4) = make_float4(mm[0], mm[1], mm[2], mm[3]);
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    sR[(tr * 2 + 0) * V2_CO + c4 + e] = s0[e];
    sR[(tr * 2 + 1) * V2_CO + c4 + e] = s1[e];
  }
  __syncthreads();
  {
    const int q = threadIdx.x;   // 256 = 2 * V2_CO: (statistic, channel)
    float a = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) a += sR[t * 2 * V2_CO + q];
    part[(long long)blockIdx.x * 2 * V2_CO + q] = a;
  }
}

// dx of one 32-column block of the tile: dx[row][c] = a dh + c0 + c1 h,  dh = gm[pillar][c] at the arg-max row
struct V2Coef {
  float a, c0, c1;
};
__device__ __forceinline__ f32x16 v2_dx(const f32x16& h, const V2Coef& k, const int* __restrict__ arg,
                                        const float* __restrict__ gm, int c, const int (&prow)[16], int q0, int half) {
  f32x16 dx;
  float gv[16];
  int am[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {          // 32 independent loads; the rows of a pillar are adjacent and share cache lines
    const unsigned o = ((unsigned)prow[r] * V2_CO + c) * 4u;      // byte offset: M * 512 < 2^32 (checked by the caller)
    am[r] = *reinterpret_cast<const int*>(reinterpret_cast<const char*>(arg) + o);
    gv[r] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(gm) + o);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float dh = am[r] == q0 + v2_row(r, half) ? gv[r] : 0.f;
    dx[r] = fmaf(k.c1, h[r], fmaf(k.a, dh, k.c0));
  }
  return dx;
}

// ---- backward: dy1 = dx W and dW = dx^T y1 in one pass over the rows ------------------------------------------------
// One workgroup per 32-row tile.  Wave w owns the 32 columns [32 w, 32 w + 32) of the tile's h and dx - one quarter of the (arg, gm)
// gathers, 4 MFMAs - and the same rows of dW^T (acc[2], the dx accumulators are the B operand; y1^T comes from the shared transposed
// tile sT, each wave stages 16 of its 64 channels before its gathers, so that the y1 fragments are dead while they are in flight).
// Its bf16 dx block also goes into the shared row-major tile sX; behind the workgroup barrier two of the four waves (alternating
// from tile to tile) multiply the whole tile by W^T: each owns 32 of the 64 input channels, 8 MFMAs in the k order 0 .. 127 - every
// dy1 element is the same chain of products as in a wave-per-tile kernel, whichever lane holds it.  dW leaves as per-workgroup
// partials for the fixed-order reduction.  LDS 49 664 bytes and 159 / 161 registers (bf16 / fp16 rows): three workgroups per CU, the
// grid k_v2_dw had - with the same tiles per workgroup dW is bit-identical to the two-kernel form.  (64-bit gather addresses in v2_dx
// cost 9 - 11 registers more: the fp16 instantiation then misses the 168 of three waves per SIMD.)
// VIS: rowpil holds each row's stage-1 token or -1 (a masked pillar's row) and arg / gm are (tokens, 128).  A masked row gathers at
// token 0, unconditionally like every other row, and gets dh = 0 with no test of its own: arg of a token only ever names rows of that
// token's pillar (k_v2_max always picks a row), a masked row is in no visible pillar, so its compare with arg cannot hold.  (A sign
// test per accumulator register on top of the compare took the kernel to 190 registers: two workgroups per CU.)
template <bool F16, bool VIS>
__global__ __launch_bounds__(V2_WAVES * 64) void k_v2_dydw(const unsigned short* __restrict__ y1, long long N,
                                                           const void* __restrict__ W, const int* __restrict__ rowpil,
                                                           const float* __restrict__ ab, const float* __restrict__ c01,
                                                           const int* __restrict__ arg, const float* __restrict__ gm,
                                                           unsigned* __restrict__ dy1, float* __restrict__ part) {
  __shared__ unsigned short sW[V2_CO * V2_LDW];
  __shared__ unsigned short sWT[V2_CI * V2_LDX];   // W^T: row j (input channel), column c
  __shared__ unsigned short sX[32 * V2_LDX];       // the tile's bf16 dx, row-major
  __shared__ unsigned short sT[V2_CI * V2_LDT];    // the tile's y1 transposed: row j, column = tile row
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), n = lane & 31, half = lane >> 5;
  v2_load_w<F16>(W, sW);
  for (int q = threadIdx.x; q < V2_CO * V2_CI; q += V2_WAVES * 64) {      // W^T in bf16: operand of the gradient product
    const int c = q >> 6, j = q & 63;
    sWT[j * V2_LDX + c] = F16 ? v2_f2bf(((const float*)W)[q]) : ((const unsigned short*)W)[q];
  }
  __syncthreads();
  const int b = wave, c = 32 * b + n;
  V2Coef k;
  k.a = ab[c]; k.c0 = c01[c]; k.c1 = c01[V2_CO + c];
  f32x16 acc[2];      // [input-channel block i2]: lane = column c, register = channel 32 i2 + row(r)
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = 0.f;
  const long long ntiles = (N + 31) / 32;
  long long t = blockIdx.x;
  V2Frag ya[4], yn[4];
  int pil = 0, piln = 0;
  if (t < ntiles) v2_load_tile(y1, rowpil, t, N, n, half, ya, pil);   // rows past the end are zero: nothing added to dW
  for (int it = 0; t < ntiles; t += gridDim.x, ++it) {
    const long long q = t * 32;
    const int nrows = (int)(N - q < 32 ? N - q : 32);
    if (t + gridDim.x < ntiles) v2_load_tile(y1, rowpil, t + gridDim.x, N, n, half, yn, piln);
    __syncthreads();                   // the previous tile's readers are done
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (s == wave) {                 // (F16: the transposed tile is the bf16 operand of the gradient product with dx)
#pragma unroll
        for (int j = 0; j < 8; ++j) sT[(16 * s + 8 * half + j) * V2_LDT + n] = F16 ? v2_f2bf((float)ya[s].hv[j]) : ya[s].s[j];
      }
    int prow[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) prow[r] = __shfl(VIS ? (pil > 0 ? pil : 0) : pil, v2_row(r, half), 64);
    const f32x16 h = v2_h<F16>(ya, sW, n, half, b);
    V2Frag bx[2];                      // dx in bf16: registers [8 kk, 8 kk + 8) of the accumulator layout
    {
      const f32x16 dx = v2_dx(h, k, arg, gm, c, prow, (int)q, half);
      bx[0].v = v2_pack(dx, 0);
      bx[1].v = v2_pack(dx, 8);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) sX[v2_row(r, half) * V2_LDX + c] = bx[r >> 3].s[r & 7];
    __syncthreads();
    // A fragments of D[i = channel][j = column] = sum_rows y1[row][channel] dx[row][column]: channel 32 i2 + n, the 8 rows
    // base + 4 half + {0..3}, base + 8 + 4 half + {0..3} - the rows of accumulator registers [base / 2, base / 2 + 8)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
      for (int i2 = 0; i2 < 2; ++i2) {
        V2Frag at;
        at.u2[0] = *reinterpret_cast<const uint2*>(sT + (32 * i2 + n) * V2_LDT + 16 * kk + 4 * half);
        at.u2[1] = *reinterpret_cast<const uint2*>(sT + (32 * i2 + n) * V2_LDT + 16 * kk + 8 + 4 * half);
        acc[i2] = v2_mfma(at.v, bx[kk].v, acc[i2]);
      }
    }
    if ((wave >> 1) == (it & 1)) {
      // D[i = row][j = input channel 32 u + n] = sum_c dx[row][c] W[c][j]
      const int j = 32 * (wave & 1) + n;
      f32x16 d;
#pragma unroll
      for (int r = 0; r < 16; ++r) d[r] = 0.f;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        V2Frag a, w;
        a.u = *reinterpret_cast<const uint4*>(sX + n * V2_LDX + 16 * s + 8 * half);
        w.u = *reinterpret_cast<const uint4*>(sWT + j * V2_LDX + 16 * s + 8 * half);
        d = v2_mfma(a.v, w.v, d);
      }
      // registers r, r + 1 are adjacent rows; neighbouring lanes swap one of them, so that every lane stores one channel pair
      // (4 bytes) of one row: the even lane of row(r), the odd lane of row(r + 1)
      const bool odd = n & 1;
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const unsigned lo = v2_f2bf(d[r]), hi = v2_f2bf(d[r + 1]);
        const unsigned got = (unsigned)__shfl_xor((int)(odd ? lo : hi), 1, 64);
        const int row = v2_row(r, half) + (odd ? 1 : 0);
        if (row < nrows) dy1[(q + row) * (V2_CI / 2) + (j >> 1)] = odd ? (got | (hi << 16)) : (lo | (got << 16));
      }
    }
    pil = piln;
#pragma unroll
    for (int s = 0; s < 4; ++s) ya[s] = yn[s];
  }
#pragma unroll
  for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      part[(long long)blockIdx.x * V2_CO * V2_CI + c * V2_CI + 32 * i2 + v2_row(r, half)] = acc[i2][r];
}

template <typename K>
int v2_resident_blocks(K kernel, int slot, int cap) {
  static int cache[12] = {0};
  if (cache[slot] == 0) {
    int per_cu = 0, dev = 0;
    hipDeviceProp_t prop;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, V2_WAVES * 64, 0) != hipSuccess || per_cu < 1) per_cu = 1;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) prop.multiProcessorCount = 256;
    const long long b = (long long)per_cu * prop.multiProcessorCount;
    cache[slot] = (int)(b > cap ? cap : b);
  }
  return cache[slot];
}

inline int v2_grid(long long N, int cap) {
  const long long blocks = ((N + 31) / 32 + V2_WAVES - 1) / V2_WAVES;
  return (int)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

struct V2Ws {
  float* part;
  double* sums;
  float* c01;
};
inline size_t v2_ws_bytes() {
  return gd_align((size_t)V2_DW_GRID * V2_CO * V2_CI * sizeof(float)) + gd_align(2 * V2_CO * sizeof(double)) +
         gd_align(2 * V2_CO * sizeof(float));
}
inline V2Ws v2_ws(void* workspace) {
  char* p = (char*)workspace;
  V2Ws w;
  w.part = (float*)p;
  p += gd_align((size_t)V2_DW_GRID * V2_CO * V2_CI * sizeof(float));
  w.sums = (double*)p;
  p += gd_align(2 * V2_CO * sizeof(double));
  w.c01 = (float*)p;
  return w;
}

}  // namespace

extern "C" size_t gdmae_vfe_max_layer_workspace_bytes(void) { return v2_ws_bytes(); }

// y1 (N, 64) bf16 with its rows in pillar-major order (gdmae_pillar_major_rows + gdmae_vfe_point_layer_fwd),
// row_pillar (N) = pillar of each row, pillar_pt_off (M + 1) = first row of each pillar; W (128, 64) bf16.
// out (M, 128) fp32 = max over the pillar of relu(BatchNorm1d_train(y1 W^T)), arg = row of the maximum (first row on
// ties = lowest point id); stats / ab / mv as gdmae_bn_fold.
// *_f16: y1 holds fp16 values (gdmae_vfe_point_layer_fwd with out_bf16 = 2) and W is the fp32 (128, 64) master matrix.
// VIS (gdmae_vfe_max_layer_vis_*): the statistics still run over all N rows; the maximum walks the Nv compact rows of the visible pillars
// (pillar_pt_off = vis_rows, row_pillar = vis_tok, M = tokens)
template <bool F16, bool VIS = false>
static int v2_fwd(const void* y1, long long N, long long Nv, const void* W, const int* pillar_pt_off, const int* row_pillar, int M, const float* gamma,
                  const float* beta, double eps, double momentum, float* running_mean, float* running_var, long long* num_batches,
                  double* stats, float* ab, float* mv, float* out, int* arg, void* workspace, void* stream) {
  GD_REQUIRE(N > 0 && M > 0, "vfe max layer: no points");
  hipStream_t st = (hipStream_t)stream;
  const V2Ws ws = v2_ws(workspace);
  const int g1 = v2_grid(N, v2_resident_blocks(k_v2_stats<F16>, F16 ? 3 : 0, V2_MAX_GRID));
  hipLaunchKernelGGL(k_v2_stats<F16>, dim3(g1), dim3(V2_WAVES * 64), 0, st, (const unsigned short*)y1, N, W, ws.part);
  GD_LAUNCH_CHECK();
  int rc = gd_bn_fold_from_partials(st, ws.part, g1, V2_CO, (double)N, gamma, beta, eps, momentum, running_mean, running_var,
                                    num_batches, stats, ab, mv);
  if (rc) return rc;
  // boundary pieces of k_v2_max: 2 slots x 128 columns x (value, row) per worker, in the partial area (the statistics partials have
  // been consumed by the fold above): V2_MAXW_GRID workgroups x 8 workers x 2 KB = the area's 32 MB
  const int g2 = v2_grid(Nv, v2_resident_blocks(k_v2_max<F16, VIS>, (VIS ? 6 : 0) + (F16 ? 4 : 1), V2_MAXW_GRID));
  const long long nwk = (long long)g2 * V2_WAVES * 2, per = (Nv + nwk - 1) / nwk;
  float* const pbest = ws.part;
  int* const parg = (int*)(ws.part + nwk * 2 * V2_CO);
  hipLaunchKernelGGL((k_v2_max<F16, VIS>), dim3(g2), dim3(V2_WAVES * 64), 0, st, (const unsigned short*)y1, Nv, W, pillar_pt_off, row_pillar, M,
                     (const float*)ab, out, arg, per, pbest, parg);
  GD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_v2_max_fix, dim3((unsigned)nwk), dim3(V2_CO), 0, st, row_pillar, Nv, per, (const float*)pbest, (const int*)parg,
                     out, arg);
  GD_LAUNCH_CHECK();
  return 0;
}
extern "C" int gdmae_vfe_max_layer_fwd(const void* y1, long long N, const void* W, const int* pillar_pt_off,
                                       const int* row_pillar, int M, const float* gamma,
                                       const float* beta, double eps, double momentum, float* running_mean,
                                       float* running_var, long long* num_batches, double* stats, float* ab, float* mv,
                                       float* out, int* arg, void* workspace, void* stream) {
  return v2_fwd<false>(y1, N, N, W, pillar_pt_off, row_pillar, M, gamma, beta, eps, momentum, running_mean, running_var, num_batches, stats, ab,
                       mv, out, arg, workspace, stream);
}
extern "C" int gdmae_vfe_max_layer_fwd_f16(const void* y1, long long N, const float* W, const int* pillar_pt_off,
                                           const int* row_pillar, int M, const float* gamma,
                                           const float* beta, double eps, double momentum, float* running_mean,
                                           float* running_var, long long* num_batches, double* stats, float* ab, float* mv,
                                           float* out, int* arg, void* workspace, void* stream) {
  return v2_fwd<true>(y1, N, N, W, pillar_pt_off, row_pillar, M, gamma, beta, eps, momentum, running_mean, running_var, num_batches, stats, ab,
                      mv, out, arg, workspace, stream);
}

// g (M, 128) fp32: gradient of out.  gm: scratch, M * 128 floats (the masked gradient).  dy1 (N, 64) bf16 is written; dgamma / dbeta / dW (128, 64)
// fp32 are written, or accumulated into when `accumulate`.
// VIS (tok_pillar != nullptr): g / out / arg / gm are (n_tok, 128) and row_pillar holds each row's token or -1
template <bool F16, bool VIS = false>
static int v2_bwd(const void* y1, long long N, const void* W, const int* row_pillar, int M, const float* gamma, const double* stats,
                  const float* ab, const float* out, const int* arg, const float* g, void* gm, void* dy1, float* dgamma, float* dbeta,
                  float* dW, int accumulate, void* workspace, void* stream, const int* tok_pillar = nullptr, int n_tok = 0) {
  GD_REQUIRE(N > 0 && M > 0, "vfe max layer: no points");
  GD_REQUIRE(M < (1 << 23), "vfe max layer: the (arg, gm) gathers use 32-bit byte offsets");
  GD_REQUIRE(!VIS || (tok_pillar != nullptr && n_tok > 0 && n_tok <= M), "vfe max layer: visible pillars");
  hipStream_t st = (hipStream_t)stream;
  const V2Ws ws = v2_ws(workspace);
  int g0 = (int)(M / 64 > V2_MAX_GRID ? V2_MAX_GRID : (M / 64 > 0 ? M / 64 : 1));      // (VIS too: the partial rows are those of the full path)
  if constexpr (VIS) hipLaunchKernelGGL(k_v2_gstats_vis, dim3(g0), dim3(256), 0, st, out, ab, g, (long long)M, tok_pillar, n_tok, (float*)gm, ws.part);
  else hipLaunchKernelGGL(k_v2_gstats, dim3(g0), dim3(256), 0, st, out, ab, g, (long long)M, (float*)gm, ws.part);
  GD_LAUNCH_CHECK();
  int rc = gd_partials_to_f64(st, ws.part, g0, 2 * V2_CO, ws.sums);
  if (rc) return rc;
  rc = gdmae_bn_bwd_coeffs(ws.sums, 2, stats, ab, gamma, V2_CO, (double)N, nullptr, dgamma, dbeta, accumulate, ws.c01, stream);
  if (rc) return rc;
  int g2 = v2_resident_blocks(k_v2_dydw<F16, VIS>, (VIS ? 6 : 0) + (F16 ? 5 : 2), V2_DW_GRID);   // one tile per workgroup and iteration; one partial tile each
  if (g2 > (N + 31) / 32) g2 = (int)((N + 31) / 32);
  hipLaunchKernelGGL((k_v2_dydw<F16, VIS>), dim3(g2), dim3(V2_WAVES * 64), 0, st, (const unsigned short*)y1, N, W, row_pillar, (const float*)ab,
                     (const float*)ws.c01, arg, (const float*)gm, (unsigned*)dy1, ws.part);
  GD_LAUNCH_CHECK();
  return gd_splitk_acc(st, ws.part, g2, (long long)V2_CO * V2_CI, dW, accumulate);
}
extern "C" int gdmae_vfe_max_layer_bwd(const void* y1, long long N, const void* W, const int* row_pillar, int M,
                                       const float* gamma, const double* stats, const float* ab,
                                       const float* out, const int* arg, const float* g, void* gm,
                                       void* dy1, float* dgamma, float* dbeta, float* dW, int accumulate, void* workspace,
                                       void* stream) {
  return v2_bwd<false>(y1, N, W, row_pillar, M, gamma, stats, ab, out, arg, g, gm, dy1, dgamma, dbeta, dW, accumulate, workspace, stream);
}
extern "C" int gdmae_vfe_max_layer_bwd_f16(const void* y1, long long N, const float* W, const int* row_pillar, int M,
                                           const float* gamma, const double* stats, const float* ab,
                                           const float* out, const int* arg, const float* g, void* gm,
                                           void* dy1, float* dgamma, float* dbeta, float* dW, int accumulate, void* workspace,
                                           void* stream) {
  return v2_bwd<true>(y1, N, W, row_pillar, M, gamma, stats, ab, out, arg, g, gm, dy1, dgamma, dbeta, dW, accumulate, workspace, stream);
}

// The same layer when only the visible pillars' features are wanted (pre-training with a prefetched, masked geometry plan: the encoder
// gathers a quarter of the pillars at a mask ratio of 0.75).  vis_rows (Nv) = the pillar-major rows of the visible pillars, ascending;
// vis_tok (Nv) = the stage-1 token of each of them; out / arg / g / gm are (n_tok, 128) - arg still holds pillar-major rows;
// row_tok (N) = token of each row's pillar or -1, tok_pillar (n_tok) ascending.  The statistics, dy1, dW, dgamma and dbeta are those of
// the entries above bit for bit (given a gradient that is zero at the masked pillars); M = number of ALL pillars.
extern "C" int gdmae_vfe_max_layer_vis_fwd(const void* y1, long long N, const void* W, const int* vis_rows, const int* vis_tok, long long Nv,
                                           int n_tok, const float* gamma, const float* beta, double eps, double momentum,
                                           float* running_mean, float* running_var, long long* num_batches, double* stats, float* ab,
                                           float* mv, float* out, int* arg, void* workspace, void* stream) {
  GD_REQUIRE(Nv > 0 && Nv <= N && n_tok > 0, "vfe max layer: no visible rows");
  return v2_fwd<false, true>(y1, N, Nv, W, vis_rows, vis_tok, n_tok, gamma, beta, eps, momentum, running_mean, running_var, num_batches, stats,
                             ab, mv, out, arg, workspace, stream);
}
extern "C" int gdmae_vfe_max_layer_vis_fwd_f16(const void* y1, long long N, const float* W, const int* vis_rows, const int* vis_tok,
                                               long long Nv, int n_tok, const float* gamma, const float* beta, double eps, double momentum,
                                               float* running_mean, float* running_var, long long* num_batches, double* stats, float* ab,
                                               float* mv, float* out, int* arg, void* workspace, void* stream) {
  GD_REQUIRE(Nv > 0 && Nv <= N && n_tok > 0, "vfe max layer: no visible rows");
  return v2_fwd<true, true>(y1, N, Nv, W, vis_rows, vis_tok, n_tok, gamma, beta, eps, momentum, running_mean, running_var, num_batches, stats,
                            ab, mv, out, arg, workspace, stream);
}
extern "C" int gdmae_vfe_max_layer_vis_bwd(const void* y1, long long N, const void* W, const int* row_tok, const int* tok_pillar, int n_tok,
                                           int M, const float* gamma, const double* stats, const float* ab, const float* out,
                                           const int* arg, const float* g, void* gm, void* dy1, float* dgamma, float* dbeta, float* dW,
                                           int accumulate, void* workspace, void* stream) {
  return v2_bwd<false, true>(y1, N, W, row_tok, M, gamma, stats, ab, out, arg, g, gm, dy1, dgamma, dbeta, dW, accumulate, workspace, stream,
                             tok_pillar, n_tok);
}
extern "C" int gdmae_vfe_max_layer_vis_bwd_f16(const void* y1, long long N, const float* W, const int* row_tok, const int* tok_pillar,
                                               int n_tok, int M, const float* gamma, const double* stats, const float* ab, const float* out,
                                               const int* arg, const float* g, void* gm, void* dy1, float* dgamma, float* dbeta, float* dW,
                                               int accumulate, void* workspace, void* stream) {
  return v2_bwd<true, true>(y1, N, W, row_tok, M, gamma, stats, ab, out, arg, g, gm, dy1, dgamma, dbeta, dW, accumulate, workspace, stream,
                            tok_pillar, n_tok);
}
