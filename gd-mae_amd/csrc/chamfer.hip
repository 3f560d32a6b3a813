// Reconstruction targets and the masked Chamfer loss (forward + gradient w.r.t. the prediction).
//
// Replaces:
//   group_inner_inds_kernel + repeat_group_idx_kernel   reference pcdet/ops/sst_ops/src/sst_ops_gpu.cu:22-39
//     (atomic arrival order there; here the first min(cnt,K) points by ascending index, then cyclic pad)
//   points[group_inds] gather, get_voxel_centers, gt - centre
//                                                        pcdet/ops/sst_ops/sst_ops_utils.py:15-27,
//                                                        pcdet/utils/common_utils.py:130-145,
//                                                        pcdet/models/backbones_3d/spt_backbone_mae.py:64-69
//   pytorch3d.loss.chamfer_distance(pred, gt, weights=mask)   spt_backbone_mae.py:88 (knn_points K=1 x2)
//
// MI355X mapping: NUM_GT_POINTS = 64 = one wavefront: lane j owns ground-truth point j of a pillar, the
// 16 predicted points are broadcast from LDS, the 16x64 distance tile lives in registers; row minima are
// wave reductions, column minima are lane-local.  Pillars with weight 0 (visible pillars) are skipped.
// The scalar loss is assembled from per-pillar partials in a fixed order (deterministic).
#include "common.h"

struct GtParams {
  float lo[3], vs[3];
  int ncols;
  int K;
};

// The one definition of a target: slot k of a pillar with cnt points takes its point k (first cnt by list order, then cyclic), relative
// to the pillar centre (idx + 0.5) * vs + lo per axis, one rounding per operation in the reference's order.
__device__ __forceinline__ int gt_slot(int k, int cnt) { return k < cnt ? k : k % cnt; }
__device__ __forceinline__ float gt_centre(long long idx, float vs, float lo) {
  return __fadd_rn(__fmul_rn(__fadd_rn((float)idx, 0.5f), vs), lo);
}

__global__ __launch_bounds__(256) void k_group_gt(const float* __restrict__ pts, const int* __restrict__ pt_off,
                                                  const int* __restrict__ csr, const long long* __restrict__ voxel_coords,
                                                  int M, GtParams P, float* __restrict__ gt, int* __restrict__ gidx) {
  const int lane = threadIdx.x & (GD_WAVE - 1);
  const int wib = threadIdx.x / GD_WAVE;
  for (int p = blockIdx.x * 4 + wib; p < M; p += gridDim.x * 4) {
    const int off = pt_off[p];
    const int cnt = pt_off[p + 1] - off;
    const long long* vc = voxel_coords + 4ll * p;  // b, z, y, x
    const float cx = gt_centre(vc[3], P.vs[0], P.lo[0]);
    const float cy = gt_centre(vc[2], P.vs[1], P.lo[1]);
    const float cz = gt_centre(vc[1], P.vs[2], P.lo[2]);
    for (int k = lane; k < P.K; k += GD_WAVE) {
      const int src = gt_slot(k, cnt);
      const int pid = csr[off + src];
      const float* r = pts + (long long)pid * P.ncols;
      float* o = gt + ((long long)p * P.K + k) * 3;
      o[0] = __fsub_rn(r[1], cx);
      o[1] = __fsub_rn(r[2], cy);
      o[2] = __fsub_rn(r[3], cz);
      if (gidx) gidx[(long long)p * P.K + k] = pid;
    }
  }
}

extern "C" int gdmae_group_gt_points(const float* points, int n_cols, const int* pillar_pt_off, const int* pillar_pts,
                                     const long long* voxel_coords, int M, int K, const float* lo, const float* vs,
                                     float* gt_points, int* gt_index, void* stream) {
  if (M <= 0) return 0;
  GtParams P;
  for (int i = 0; i < 3; ++i) {
    P.lo[i] = lo[i];
    P.vs[i] = vs[i];
  }
  P.ncols = n_cols;
  P.K = K;
  int grid = gd_div_up(M, 4);
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(k_group_gt, dim3(grid), dim3(256), 0, (hipStream_t)stream, points, pillar_pt_off, pillar_pts,
                     voxel_coords, M, P, gt_points, gt_index);
  GD_LAUNCH_CHECK();
  return 0;
}

// term[m] = w_m * ( (1/P1) sum_i min_j |x_i - y_j|^2 + (1/P2) sum_j min_i |x_i - y_j|^2 )
// dpred[m,i,:] = d term[m] / d x_i
template <int P1MAX>
__global__ __launch_bounds__(256) void k_chamfer(const float* __restrict__ pred, const float* __restrict__ gt,
                                                 const float* __restrict__ w, int M, int P1, int P2,
                                                 float* __restrict__ term, float* __restrict__ dpred) {
  __shared__ float sx[4][P1MAX * 3];
  const int lane = threadIdx.x & (GD_WAVE - 1);
  const int wib = threadIdx.x / GD_WAVE;
  for (int m = blockIdx.x * 4 + wib; m < M; m += gridDim.x * 4) {
    const float wm = w[m];
    float* dp = dpred + (long long)m * P1 * 3;
    if (wm == 0.f) {
      for (int e = lane; e < P1 * 3; e += GD_WAVE) dp[e] = 0.f;
      if (lane == 0) term[m] = 0.f;
      continue;
    }
    for (int e = lane; e < P1 * 3; e += GD_WAVE) sx[wib][e] = pred[(long long)m * P1 * 3 + e];
    __builtin_amdgcn_wave_barrier();
    const bool has = lane < P2;
    float y0 = 0.f, y1 = 0.f, y2 = 0.f;
    if (has) {
      const float* g = gt + ((long long)m * P2 + lane) * 3;
      y0 = g[0];
      y1 = g[1];
      y2 = g[2];
    }
    float best = INFINITY;
    int besti = 0;
    float sumx = 0.f;
    const float cx = wm / (float)P1, cy = wm / (float)P2;
    for (int i = 0; i < P1; ++i) {
      const float x0 = sx[wib][3 * i], x1 = sx[wib][3 * i + 1], x2 = sx[wib][3 * i + 2];
      const float d0 = x0 - y0, d1 = x1 - y1, d2 = x2 - y2;
      const float d = has ? (d0 * d0 + d1 * d1 + d2 * d2) : INFINITY;
      if (d < best) {
        best = d;
        besti = i;
      }
      const float dmin = gd_wave_min(d);
      const unsigned long long bal = __ballot(d == dmin);
      const int jstar = __ffsll((long long)bal) - 1;
      sumx += dmin;
      // gradient through min_j for row i: 2 (x_i - y_j*) * w / P1
      const float g0 = 2.f * cx * __shfl(d0, jstar, GD_WAVE);
      const float g1 = 2.f * cx * __shfl(d1, jstar, GD_WAVE);
      const float g2 = 2.f * cx * __shfl(d2, jstar, GD_WAVE);
      if (lane == 0) {
        dp[3 * i] = g0;
        dp[3 * i + 1] = g1;
        dp[3 * i + 2] = g2;
      }
    }
    const float sumy = gd_wave_sum(has ? best : 0.f);
    if (lane == 0) term[m] = cx * sumx + cy * sumy;
    // gradient through min_i for column j: lanes whose nearest prediction is i add 2 (x_i - y_j) * w / P2
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    for (int i = 0; i < P1; ++i) {
      const bool mine = has && besti == i;
      const float x0 = sx[wib][3 * i], x1 = sx[wib][3 * i + 1], x2 = sx[wib][3 * i + 2];
      const float a0 = gd_wave_sum(mine ? 2.f * cy * (x0 - y0) : 0.f);
      const float a1 = gd_wave_sum(mine ? 2.f * cy * (x1 - y1) : 0.f);
      const float a2 = gd_wave_sum(mine ? 2.f * cy * (x2 - y2) : 0.f);
      if (lane == 0) {
        dp[3 * i] += a0;
        dp[3 * i + 1] += a1;
        dp[3 * i + 2] += a2;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// NUM_PRD_POINTS = 16 fast path.  The generic kernel above spends its time in cross-lane reductions (16 wave-minima
// + 48 wave-sums per pillar, ~600 us per step).  Here lane j keeps the 16 distances to its ground-truth point in
// registers as sortable keys (distance bits << 32 | j) and the 16 row minima are ONE transposed butterfly
// (8+4+2+1 exchanges halve the values per lane while doubling the lanes merged, then 2 plain steps): 17 64-bit
// exchanges instead of 96, ties resolved to the lowest j like the generic kernel.  The column-term gradient is
// gathered by 48 lanes (one per prediction coordinate) from an LDS copy of (nearest prediction, y) per ground-truth
// point in ascending j order, and dpred is written as one coalesced 192-byte row.
template <int N>
__device__ __forceinline__ void ch_tstep(unsigned long long (&k)[16], int mask, int lane) {
  const bool hi = (lane & mask) != 0;
#pragma unroll
  for (int t = 0; t < N; ++t) {
    const unsigned long long send = hi ? k[t] : k[t + N];
    const unsigned long long keep = hi ? k[t + N] : k[t];
    const unsigned long long recv = __shfl_xor(send, mask, GD_WAVE);
    k[t] = keep < recv ? keep : recv;
  }
}

// POINTS = true (gdmae_chamfer_points): the (M, P2, 3) targets are never written.  Lane j takes target j of k_group_gt itself,
// points[pillar_pts[off + gt_slot(j, cnt)]] - centre: a pillar has ~11 points, so the array was a ~6-fold replication of them, written
// for the visible pillars too.  Offset, index and point loads are unconditional with a clamped slot (a branch around a load is a join
// with a load in flight); lanes >= P2 are cleared afterwards.  A zero-weight pillar leaves before any of them.
template <bool POINTS>
__global__ __launch_bounds__(256) void k_chamfer16(const float* __restrict__ pred, const float* __restrict__ gt,
                                                   const float* __restrict__ pts, const int* __restrict__ pt_off,
                                                   const int* __restrict__ csr, const long long* __restrict__ voxel_coords,
                                                   GtParams G, const float* __restrict__ w, int M, int P2,
                                                   float* __restrict__ term, float* __restrict__ dpred) {
  __shared__ float sx[4][48];
  __shared__ float sy[4][GD_WAVE * 3];
  __shared__ int sb[4][GD_WAVE];
  __shared__ float sg[4][48];
  const int lane = threadIdx.x & (GD_WAVE - 1);
  const int wib = threadIdx.x / GD_WAVE;
  const int my_i = ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1);
  for (int m = blockIdx.x * 4 + wib; m < M; m += gridDim.x * 4) {
    const float wm = w[m];
    float* dp = dpred + (long long)m * 48;
    if (wm == 0.f) {
      if (lane < 48) dp[lane] = 0.f;
      if (lane == 0) term[m] = 0.f;
      continue;
    }
    if (lane < 48) sx[wib][lane] = pred[(long long)m * 48 + lane];
    const bool has = lane < P2;
    float y0 = 0.f, y1 = 0.f, y2 = 0.f;
    if (POINTS) {
      const int off = pt_off[m];
      const int cnt = pt_off[m + 1] - off;
      const long long* vc = voxel_coords + 4ll * m;  // b, z, y, x
      const int pid = csr[off + gt_slot(has ? lane : P2 - 1, cnt)];
      const float* r = pts + (long long)pid * G.ncols;
      const float r1 = r[1], r2 = r[2], r3 = r[3];
      const float t0 = __fsub_rn(r1, gt_centre(vc[3], G.vs[0], G.lo[0]));
      const float t1 = __fsub_rn(r2, gt_centre(vc[2], G.vs[1], G.lo[1]));
      const float t2 = __fsub_rn(r3, gt_centre(vc[1], G.vs[2], G.lo[2]));
      y0 = has ? t0 : 0.f;
      y1 = has ? t1 : 0.f;
      y2 = has ? t2 : 0.f;
    } else if (has) {
      const float* g = gt + ((long long)m * P2 + lane) * 3;
      y0 = g[0];
      y1 = g[1];
      y2 = g[2];
    }
    __builtin_amdgcn_wave_barrier();
    const float cx = wm / 16.f, cy = wm / (float)P2;
    unsigned long long k[16];
    float best = INFINITY;
    int besti = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float d0 = sx[wib][3 * i] - y0, d1 = sx[wib][3 * i + 1] - y1, d2 = sx[wib][3 * i + 2] - y2;
      const float d = has ? (d0 * d0 + d1 * d1 + d2 * d2) : INFINITY;
      if (d < best) {
        best = d;
        besti = i;
      }
      k[i] = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)lane;
    }
    ch_tstep<8>(k, 32, lane);
    ch_tstep<4>(k, 16, lane);
    ch_tstep<2>(k, 8, lane);
    ch_tstep<1>(k, 4, lane);
    unsigned long long k0 = k[0];
    {
      unsigned long long o = __shfl_xor(k0, 2, GD_WAVE);
      k0 = k0 < o ? k0 : o;
      o = __shfl_xor(k0, 1, GD_WAVE);
      k0 = k0 < o ? k0 : o;
    }
    const float dmin = __uint_as_float((unsigned)(k0 >> 32));
    const int jstar = (int)(k0 & 63u);
    const float ys0 = __shfl(y0, jstar, GD_WAVE), ys1 = __shfl(y1, jstar, GD_WAVE), ys2 = __shfl(y2, jstar, GD_WAVE);
    if ((lane & 3) == 0) {
      sg[wib][3 * my_i] = 2.f * cx * (sx[wib][3 * my_i] - ys0);
      sg[wib][3 * my_i + 1] = 2.f * cx * (sx[wib][3 * my_i + 1] - ys1);
      sg[wib][3 * my_i + 2] = 2.f * cx * (sx[wib][3 * my_i + 2] - ys2);
    }
    const float sumx = gd_wave_sum((lane & 3) == 0 ? dmin : 0.f);
    const float sumy = gd_wave_sum(has ? best : 0.f);
    if (lane == 0) term[m] = cx * sumx + cy * sumy;
    if (POINTS) {
      // column term, once per ground-truth point: lane j leaves 2 cy (x_besti - y_j) where the loop below would have formed it for
      // the one prediction i = besti that keeps it - the same operands and operations (no contraction in this build), so the 48
      // lanes only pick and add.  The two-launch entry keeps the loop it always had, and the tests hold the two against each other.
      sy[wib][3 * lane] = 2.f * cy * (sx[wib][3 * besti] - y0);
      sy[wib][3 * lane + 1] = 2.f * cy * (sx[wib][3 * besti + 1] - y1);
      sy[wib][3 * lane + 2] = 2.f * cy * (sx[wib][3 * besti + 2] - y2);
    } else {
      sy[wib][3 * lane] = y0;
      sy[wib][3 * lane + 1] = y1;
      sy[wib][3 * lane + 2] = y2;
    }
    sb[wib][lane] = has ? besti : -1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    if (lane < 48) {
      const int i = lane / 3, c = lane - 3 * i;
      const float xi = sx[wib][lane];
      float acc = 0.f;
      for (int j = 0; j < P2; ++j) {
        const float v = POINTS ? sy[wib][3 * j + c] : 2.f * cy * (xi - sy[wib][3 * j + c]);
        acc += sb[wib][j] == i ? v : 0.f;
      }
      dp[lane] = sg[wib][lane] + acc;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

extern "C" int gdmae_chamfer(const float* pred, const float* gt, const float* weights, int M, int P1, int P2, float* term,
                             float* dpred, void* stream) {
  if (M <= 0) return 0;
  GD_REQUIRE(P2 >= 1 && P2 <= GD_WAVE, "NUM_GT_POINTS must be <= 64 (one lane per ground-truth point)");
  GD_REQUIRE(P1 >= 1 && P1 <= 64, "NUM_PRD_POINTS must be <= 64");
  int grid = gd_div_up(M, 4);
  if (grid > 8192) grid = 8192;
  if (P1 == 16)
    hipLaunchKernelGGL(k_chamfer16<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, pred, gt, nullptr, nullptr, nullptr, nullptr,
                       GtParams{}, weights, M, P2, term, dpred);
  else
    hipLaunchKernelGGL((k_chamfer<64>), dim3(grid), dim3(256), 0, (hipStream_t)stream, pred, gt, weights, M, P1, P2, term,
                       dpred);
  GD_LAUNCH_CHECK();
  return 0;
}

// gdmae_group_gt_points(K = P2) -> gdmae_chamfer(P1 = 16) as one launch, bit for bit, without the (M, P2, 3) targets in between
extern "C" int gdmae_chamfer_points(const float* pred, const float* points, int n_cols, const int* pillar_pt_off, const int* pillar_pts,
                                    const long long* voxel_coords, const float* lo, const float* vs, const float* weights, int M,
                                    int P1, int P2, float* term, float* dpred, void* stream) {
  if (M <= 0) return 0;
  GD_REQUIRE(P1 == 16, "chamfer_points serves NUM_PRD_POINTS = 16 (gdmae_group_gt_points + gdmae_chamfer for the others)");
  GD_REQUIRE(P2 >= 1 && P2 <= GD_WAVE, "NUM_GT_POINTS must be <= 64 (one lane per ground-truth point)");
  GD_REQUIRE(n_cols >= 4, "point rows are (b, x, y, z, ...)");
  GtParams G;
  for (int i = 0; i < 3; ++i) {
    G.lo[i] = lo[i];
    G.vs[i] = vs[i];
  }
  G.ncols = n_cols;
  G.K = P2;
  int grid = gd_div_up(M, 4);
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(k_chamfer16<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, pred, nullptr, points, pillar_pt_off, pillar_pts,
                     voxel_coords, G, weights, M, P2, term, dpred);
  GD_LAUNCH_CHECK();
  return 0;
}
