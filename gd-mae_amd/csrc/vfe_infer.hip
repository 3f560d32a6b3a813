// DynVFE for inference: decoration, relu(W1' f + b1), relu(W2' h + b2) and the per-pillar maximum in ONE kernel over the pillar-major
// point rows (reference pcdet/models/backbones_3d/vfe/dyn_vfe.py:74-112 in eval mode: BatchNorm1d with running statistics is a constant
// per-channel affine, folded into W' / b by the caller).  Neither the (N, 64) nor the (N, 128) rows reach HBM: the training kernels
// (vfe_fused.hip, vfe_layer2.hip) each make a statistics pass and a second pass and keep y1 for the backward; nothing of that is needed
// when the affine is known up front.  Bytes per point: its row (4 (F + 1)), its pillar id and the pillar's cell / mean (L2 hits) -
// about 30 B against 128 B (y1 written and read twice in fp16) + the two decoration reads of the training forward.
//
// Layer 1 runs on the fp32 matrix cores like k_vfe1 (the features carry absolute coordinates), TRANSPOSED: A = W1' (channel x k),
// B = the features of the lane's point, so lane (n, half) ends up with 32 channels of point n in its accumulators - which is the A
// operand of layer 2 (point x k) once rounded to fp16: the k index of a matrix-core product may be permuted freely as long as both
// operands agree, so W2' is staged in LDS with its columns in the order the accumulators hold them.  b1 rides along as the weight of
// a constant feature.  Layer 2: v_mfma_f32_32x32x16_f16, D[point][channel]: lane (n, half) holds channel 32 c + n of 16 points.
//
// Pillar maximum: the scheme of k_v2_max (vfe_layer2.hip).  Every half-wave is a worker with a contiguous range of `per` rows, the
// same number for every worker wherever the pillar boundaries fall, so a pillar of thousands of points is shared by many workers
// instead of being one serial chain.  The tile rows are permuted so that a lane's 16 accumulator registers are 16 CONSECUTIVE rows of
// its worker; the lane walks them in order and closes a pillar whenever the pillar id changes.  A pillar inside the range is written
// with plain stores; the pieces of a pillar that crosses a range boundary meet in `out` through atomic integer maxima (the values are
// ReLU outputs: non-negative floats order like their bit patterns, and a maximum does not depend on the order of its operands - the
// result is bit-repeatable).  `out` is cleared before the launch for them.
#include "../../include/gdmae_hip.h"
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
union ViFrag {
  uint4 u;
  f16x8 h;
};

constexpr int VI_C1 = 64, VI_C2 = 128;
constexpr int VI_WAVES = 4;
constexpr int VI_LDW = VI_C1 + 8;      // fp16 elements per row of the W2' tile in LDS (conflict-free 16-byte reads)
constexpr int VI_MAX_GRID = 1024;
constexpr int VI_MIN_ROWS = 32;        // rows per worker below which the grid shrinks instead

struct ViGeom {
  float lo[3], vs[3];
};

// accumulator register r of lane (n, half) of a 32 x 32 product is row (r & 3) + 8 (r >> 2) + 4 half
__device__ __forceinline__ int vi_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

template <int F>
struct ViA {          // stage A of a point: its row and pillar
  float r[F + 1];
  int pil;
};
struct ViB {          // stage B: the pillar's cell and mean
  int cz, cy, cx;
  float m[3];
};

template <int F>
__device__ __forceinline__ void vi_load_a(const float* __restrict__ pts, const int* __restrict__ rowpil, long long row, int N, ViA<F>& A) {
  const long long rc = row < N ? row : N - 1;      // clamped into [0, N): every load is unconditional; a row outside the worker's range is
                                                   // never looked at (the walk stops at the range's row count)
  const float* p = pts + rc * (F + 1);
#pragma unroll
  for (int k = 0; k < F + 1; ++k) A.r[k] = p[k];
  A.pil = rowpil[rc];
}
template <int F>
__device__ __forceinline__ void vi_load_b(const long long* __restrict__ coords, const float* __restrict__ mean, int pil, ViB& B) {
  const int* c = reinterpret_cast<const int*>(coords + 4ll * pil);      // (b, z, y, x) int64, non-negative: the low words
  const float* m = mean + (long long)pil * F;
  B.cz = c[2]; B.cy = c[4]; B.cx = c[6];
  B.m[0] = m[0]; B.m[1] = m[1]; B.m[2] = m[2];
}
// decorated features in the reference's order [xyz - cell centre | raw point | xyz - pillar mean] (the arithmetic of k_decorate /
// vf_features), then the constant 1 that carries b1
template <int F>
__device__ __forceinline__ void vi_features(const ViA<F>& A, const ViB& B, const ViGeom& G, float (&f)[F + 8]) {
  const float x = A.r[1], y = A.r[2], z = A.r[3];
  f[0] = __fsub_rn(x, __fadd_rn(__fmul_rn(__fadd_rn((float)B.cx, 0.5f), G.vs[0]), G.lo[0]));
  f[1] = __fsub_rn(y, __fadd_rn(__fmul_rn(__fadd_rn((float)B.cy, 0.5f), G.vs[1]), G.lo[1]));
  f[2] = __fsub_rn(z, __fadd_rn(__fmul_rn(__fadd_rn((float)B.cz, 0.5f), G.vs[2]), G.lo[2]));
#pragma unroll
  for (int k = 0; k < F; ++k) f[3 + k] = A.r[1 + k];
  f[3 + F] = __fsub_rn(x, B.m[0]);
  f[4 + F] = __fsub_rn(y, B.m[1]);
  f[5 + F] = __fsub_rn(z, B.m[2]);
  f[6 + F] = 1.f;
  f[7 + F] = 0.f;
}

template <int F>
__global__ __launch_bounds__(VI_WAVES * 64) void k_vfe_infer(const float* __restrict__ pts, const long long* __restrict__ coords,
                                                             const int* __restrict__ rowpil, const float* __restrict__ mean, int N,
                                                             ViGeom G, const float* __restrict__ W1, const float* __restrict__ b1,
                                                             const float* __restrict__ W2, const float* __restrict__ b2,
                                                             float* __restrict__ out, int per) {
  constexpr int D = F + 6;                 // decorated features
  constexpr int KS = (D + 2) / 2;          // fp32 k-steps (K = 2 each) of layer 1 over D features + the constant
  __shared__ unsigned short sW[VI_C2 * VI_LDW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 31, half = lane >> 5;

  // ---- W2' (128, 64) fp32 -> fp16 in LDS, columns in accumulator order: slot 16 s + 8 h + j of a row holds the channel
  // 32 (s >> 1) + vi_row(8 (s & 1) + j, h) = 32 (s >> 1) + 16 (s & 1) + 8 (j >> 2) + 4 h + (j & 3)
  for (int q = threadIdx.x; q < VI_C2 * 8; q += VI_WAVES * 64) {
    const int col = q >> 3, s = (q & 7) >> 1, h = q & 1;
    const float* w = W2 + col * VI_C1 + 32 * (s >> 1) + 16 * (s & 1) + 4 * h;
    const float4 a = *reinterpret_cast<const float4*>(w), b = *reinterpret_cast<const float4*>(w + 8);
    uint4 o;
    o.x = gd_pack_f16(a.x, a.y); o.y = gd_pack_f16(a.z, a.w); o.z = gd_pack_f16(b.x, b.y); o.w = gd_pack_f16(b.z, b.w);
    *reinterpret_cast<uint4*>(sW + col * VI_LDW + 16 * s + 8 * h) = o;
  }
  // ---- A operand of layer 1: lane (n, half) holds [W1' | b1][32 blk + n][2 s + half]
  float wa[2][KS];
#pragma unroll
  for (int blk = 0; blk < 2; ++blk)
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int d = 2 * s + half, ch = 32 * blk + n;
      wa[blk][s] = d < D ? W1[ch * D + d] : (d == D ? b1[ch] : 0.f);
    }
  float cb[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) cb[c] = b2[32 * c + n];
  __syncthreads();

  // ---- this worker's rows; hp: its first pillar began before the range, tail: its last pillar continues behind it
  const int wk = (blockIdx.x * VI_WAVES + wave) * 2 + half;
  const long long qa = (long long)wk * per < N ? (long long)wk * per : N, qb = (long long)(wk + 1) * per < N ? (long long)(wk + 1) * per : N;
  const int q0 = (int)qa, q1 = (int)qb;
  bool hp, tail;
  {
    const int ia = q0 > 0 ? q0 - 1 : 0, ib = q0 < N ? q0 : N - 1, ic = q1 > 0 ? q1 - 1 : 0, id = q1 < N ? q1 : N - 1;
    const int a0 = rowpil[ia], a1 = rowpil[ib], c0 = rowpil[ic], c1 = rowpil[id];
    hp = q0 > 0 && q0 < q1 && a0 == a1;
    tail = q1 < N && q0 < q1 && c0 == c1;
  }
  // the tile row this lane loads as product row n: worker (n >> 2) & 1, local row (n & 3) + 4 (n >> 3)
  const int ld_wk = (n >> 2) & 1, ld_r = (n & 3) + 4 * (n >> 3);
  const int q0o = __shfl(q0, lane ^ 32, 64), q1o = __shfl(q1, lane ^ 32, 64);
  const int lq0 = ld_wk == half ? q0 : q0o;
  const int len = q1 - q0, leno = q1o - q0o;
  const int iters = ((len > leno ? len : leno) + 15) / 16;                  // wave-uniform

  float best[4] = {0.f, 0.f, 0.f, 0.f};
  int cur = -1;
  auto flush = [&](int pillar, bool shared) {
    float* o = out + (long long)pillar * VI_C2 + n;
    if (shared) {
#pragma unroll
      for (int c = 0; c < 4; ++c) atomicMax(reinterpret_cast<int*>(o + 32 * c), __float_as_int(best[c]));
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) o[32 * c] = best[c];
    }
  };

  // two-stage pipeline of a point's loads (row + pillar id, then the pillar's cell and mean), as k_vfe1: A of tile it + 2 and B of
  // tile it + 1 are requested while tile it is multiplied
  ViA<F> A1, A2, A3;
  ViB B1, B2;
  vi_load_a<F>(pts, rowpil, (long long)lq0 + ld_r, N, A1);
  vi_load_a<F>(pts, rowpil, (long long)lq0 + 16 + ld_r, N, A2);
  vi_load_b<F>(coords, mean, A1.pil, B1);
  for (int it = 0; it < iters; ++it) {
    const int qt = q0 + 16 * it;                   // first row of this worker's 16-row slice
    const int nrows = q1 - qt < 16 ? (q1 - qt > 0 ? q1 - qt : 0) : 16;
    vi_load_a<F>(pts, rowpil, (long long)lq0 + 16 * (it + 2) + ld_r, N, A3);
    vi_load_b<F>(coords, mean, A2.pil, B2);
    __builtin_amdgcn_sched_barrier(0);             // the requests go out first

    int prow[16];                                  // pillar of each of this worker's rows (uniform within the half-wave)
#pragma unroll
    for (int r = 0; r < 16; ++r) prow[r] = __shfl(A1.pil, vi_row(r, half), 64);
    bool st[16];                                   // row r opens a new pillar
    st[0] = nrows > 0 && prow[0] != cur;
#pragma unroll
    for (int r = 1; r < 16; ++r) st[r] = r < nrows && prow[r] != prow[r - 1];
    const int cur_in = cur;
#pragma unroll
    for (int r = 0; r < 16; ++r) cur = r < nrows ? prow[r] : cur;

    // ---- layer 1 (fp32 matrix cores): h1[blk][r] = channel 32 blk + vi_row(r, half) of point n
    float f[F + 8];
    vi_features<F>(A1, B1, G, f);
    f32x16 h1[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) h1[0][r] = h1[1][r] = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const float fb = half ? f[2 * s + 1] : f[2 * s];
      h1[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[0][s], fb, h1[0], 0, 0, 0);
      h1[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[1][s], fb, h1[1], 0, 0, 0);
    }
    // ---- ReLU, fp16: slot s of the layer-2 operand = registers 8 (s & 1) .. + 7 of block s >> 1
    ViFrag ya[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const f32x16& a = h1[s >> 1];
      const int r0 = 8 * (s & 1);
      ya[s].u.x = gd_pack_f16_relu(a[r0], a[r0 + 1]);
      ya[s].u.y = gd_pack_f16_relu(a[r0 + 2], a[r0 + 3]);
      ya[s].u.z = gd_pack_f16_relu(a[r0 + 4], a[r0 + 5]);
      ya[s].u.w = gd_pack_f16_relu(a[r0 + 6], a[r0 + 7]);
    }
    // ---- layer 2: h2[c][r] = channel 32 c + n of this worker's row qt + r
    f32x16 h2[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int r = 0; r < 16; ++r) h2[c][r] = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        ViFrag w;
        w.u = *reinterpret_cast<const uint4*>(sW + (32 * c + n) * VI_LDW + 16 * s + 8 * half);
        h2[c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ya[s].h, w.h, h2[c], 0, 0, 0);
      }
    }
    // ---- the walk: branch-free selects; only the stores that close a pillar sit behind a (rarely taken) branch
    if (st[0] && cur_in >= 0) {                    // the pillar carried over from the previous slice ends here
      flush(cur_in, hp);
      hp = false;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float bin = st[r] ? 0.f : best[c];
        const float v = fmaxf(h2[c][r] + cb[c], 0.f);
        best[c] = r < nrows ? fmaxf(v, bin) : bin;
      }
      if (r < 15 && st[r < 15 ? r + 1 : 15]) {     // row r closes its pillar
        flush(prow[r], hp);
        hp = false;
      }
    }
    A1 = A2;
    A2 = A3;
    B1 = B2;
  }
  if (cur >= 0) flush(cur, hp || tail);            // the range's last pillar
}

template <int F>
int vi_launch(hipStream_t st, const float* pts, const long long* coords, const int* rowpil, const float* mean, long long N, const ViGeom& G,
              const float* W1, const float* b1, const float* W2, const float* b2, float* out) {
  int grid = gd_div_up(N, 2 * VI_WAVES * VI_MIN_ROWS);
  grid = grid < 1 ? 1 : (grid > VI_MAX_GRID ? VI_MAX_GRID : grid);
  const int workers = grid * VI_WAVES * 2;
  const int per = gd_div_up(gd_div_up(N, workers), 16) * 16;
  hipLaunchKernelGGL((k_vfe_infer<F>), dim3(grid), dim3(VI_WAVES * 64), 0, st, pts, coords, rowpil, mean, (int)N, G, W1, b1, W2, b2, out, per);
  GD_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// C ABI: see include/gdmae_hip.h
extern "C" int gdmae_vfe_infer(const float* points_pm, const long long* voxel_coords, const int* row_pillar, const float* pillar_mean,
                               long long N, long long M, int n_cols, const float* lo, const float* vs, const float* W1, const float* b1,
                               int c1, const float* W2, const float* b2, int c2, float* out, void* stream) {
  const int F = n_cols - 1;
  GD_REQUIRE(F >= 3 && F <= 5, "vfe_infer: 3 to 5 point features");
  GD_REQUIRE(c1 == VI_C1 && c2 == VI_C2, "vfe_infer: layers of 64 and 128 channels");
  GD_REQUIRE(N >= 0 && M >= 0 && N < (1ll << 31) - 4096 && M < (1ll << 31), "vfe_infer: row counts");
  if (N == 0 || M == 0) return 0;                  // no pillar, nothing to write: no launch
  hipStream_t st = (hipStream_t)stream;
  GD_CHECK(hipMemsetAsync(out, 0, (size_t)M * VI_C2 * sizeof(float), st));
  ViGeom G;
  for (int k = 0; k < 3; ++k) { G.lo[k] = lo[k]; G.vs[k] = vs[k]; }
  GdTimed timed(GD_T_VFE, st, (double)N * (4.0 * n_cols + 4.0) + (double)M * (4.0 * VI_C2 * 2 + 32.0 + 4.0 * F),
                2.0 * N * ((F + 7) * VI_C1 + (double)VI_C1 * VI_C2));
  if (F == 3) return vi_launch<3>(st, points_pm, voxel_coords, row_pillar, pillar_mean, N, G, W1, b1, W2, b2, out);
  if (F == 4) return vi_launch<4>(st, points_pm, voxel_coords, row_pillar, pillar_mean, N, G, W1, b1, W2, b2, out);
  return vi_launch<5>(st, points_pm, voxel_coords, row_pillar, pillar_mean, N, G, W1, b1, W2, b2, out);
}
