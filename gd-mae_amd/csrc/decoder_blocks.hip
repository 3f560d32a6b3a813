// Decoder conv_out backward on TOKEN BLOCKS (source stages with an upsampling stride u = 2 or 4, 128 channels, bf16 rows).
//
// The rows of such a stage are the u x u full-resolution sites of its tokens, token after token (plan.py upsample_cells: row
// t u^2 + dy u + dx is cell (b, ty u + dy, tx u + dx)).  The rulebook path (gdmae_spconv / gdmae_tap_dw over nbr (n, 9)) treats
// them as unrelated rows and gathers nine dY rows per site; the u^2 sites of a token need only the (u + 2)^2 rows of its halo -
// 36 instead of 144 at u = 4, 16 instead of 36 at u = 2.
//
// gdmae_decoder_block_dw: the stage's part of the weight gradient
//     dWk[k][co][col + ci] += sum_t dY[site_t - offset(k)][co] * Zd[t][ci]        Zd = bf16(bf16(relu(a P + b)) - bg)
// A workgroup (8 wavefronts) owns a slice of whole tokens and 32 of the 128 dY channels: all 128 input channels x 9 taps; wavefront
// w owns input channels 32 (w & 3) .. + 31 and taps 0 - 4 (w < 4) or 5 - 8, one 32 x 32 accumulator per tap.  Per chunk of 64 sites
// the workgroup stages the dY halo rows of its channel quarter (resolved from tile_slot like k_decoder_site_rulebook does, zero outside
// the map) and the chunk's Zd rows - computed from P on the way into LDS with the formula and the roundings of
// gdmae_rows_affine_relu_sub, Zd is never written - and every Zd fragment meets the dY fragments of the wavefront's taps, which differ
// only in their row offset inside the halo.  Both operands contract over the slow (row) axis and are read with ds_read_b64_tr_b16
// as in dw_grouped.hip.
//
// SAME BITS as the rulebook path: the slices are gdmae_tap_dw's (gd_dw_pick: the same count, the same rows per slice), a slice's
// 64-row chunks are multiplied in the same order with the same instruction (v_mfma_f32_32x32x16_bf16, the 16 rows of a k-step in the
// same positions; dY is the A operand here and the B operand there, which the products do not see), and the partial tiles (slice,
// tap, co, ci) are summed in slice order by k_block_dw_reduce exactly as k_tap_dw_reduce does.  Every element of dW is therefore the
// same chain of fp32 operations; tests/test_decoder_block_backward.py asserts equality.  No floating-point atomics.
//
// Load discipline: every global load has a clamped address, masks are applied when a chunk is staged, and what a phase
// consumes was requested an iteration earlier: the rows of chunk c + 2 when chunk c + 1 is staged, the tile slots of their halo cells
// (one thread per halo row, the resolved row published in LDS) two iterations before that.  The cells of all the slice's tokens are
// decoded once, before the loop.
#include "../../include/gdmae_hip.h"
#include "common.h"
#include "dw_grouped.h"
#include <stdlib.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kC = 128;                  // channels of P / dY
constexpr int kChunk = 64;               // sites per staged chunk (four k-steps of 16)
constexpr int kXBytes = kChunk * kC * 2; // Zd chunk: 16 KB
constexpr int kMaxTok = 2048;            // tokens of a slice (their decoded cells live in LDS: 32 KB); more: the entry refuses
constexpr int kHP = 6;                   // halo row pitch of a token's patch in LDS rows (u + 2 = 6 at u = 4; 6 at u = 2 as well: the
                                         // four rows of a transposed read are then distinct mod 4 - conflict-free, see dy_off)
constexpr int kQ = 32;                   // dY channels of a workgroup (64-byte halo rows in LDS)

template <int U>
struct Geo {
  static constexpr int TPC = kChunk / (U * U);        // tokens per chunk: 4 / 16
  static constexpr int HW = U + 2;                    // halo width
  static constexpr int HS = HW * HW;                  // halo rows per token: 36 / 16
  static constexpr int LT = U == 4 ? 36 : 24;         // LDS rows per token patch
  static constexpr int NP = 2;                        // 16-byte pieces per thread and chunk (TPC * HS * 4 = 576 / 1024 pieces of 1024)
  static constexpr int LROWS = U == 4 ? NP * 128 : TPC * LT;     // LDS rows of a halo chunk (u = 4: the rounded-up pieces land behind)
  static constexpr int DBytes = LROWS * 64;           // 16 KB / 24 KB
  static constexpr int Buf = kXBytes + DBytes;
  static constexpr int KSR = U == 4 ? 36 : 96;        // LDS rows per k-step of 16 sites (1 token / 4 tokens): a multiple of 4
  static constexpr int HRP = NP * 128;                // halo rows of a chunk, rounded up to the pieces (one resolving thread each)
  static constexpr int MaxCps = kMaxTok / TPC;        // chunks per slice the token table holds
};

// byte offset of 16-byte unit u16 (0..15) of Zd row `row` (the image of dw_grouped.hip: 64-byte segments XOR (row & 3))
__device__ __forceinline__ int x_off(int row, int u16) { return row * 256 + (((u16 >> 2) ^ (row & 3)) << 6) + ((u16 & 3) << 4); }
// byte offset of halo row `row` (64-byte rows: one channel quarter).  Position inside the 256-byte bank row = 64 (row & 3), so four
// rows that are distinct mod 4 never share a bank.
__device__ __forceinline__ int dy_off(int row) { return row * 64; }

__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* p0, const unsigned char* p1) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)p0);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)p1);
  const uint2 a = __builtin_bit_cast(uint2, lo), b = __builtin_bit_cast(uint2, hi);
  return __builtin_bit_cast(bf16x8, make_uint4(a.x, a.y, b.x, b.y));
}

struct BlockDwArgs {
  const unsigned short* P;       // (n, 128) bf16 rows of the stage
  const float* a;                // (128) BatchNorm scale / shift of the stage
  const float* b;
  const unsigned short* bg;      // (128) bf16 background of the stage's channels
  const int* site;               // (n) full-resolution cells; site[t u^2] = the token's first cell
  const unsigned short* dY;      // (n_act * 64, 128) bf16 tile-compact output gradient
  const int* tile_slot;
  float* part;                   // (S, 9, 128, 128) fp32 partial tiles [slice][tap][co][ci]
  long long n;                   // sites
  int ntok, H, W, TH, TW;
  int S, cps;                    // slices, chunks per slice
};

template <int U>
__global__ __launch_bounds__(512) void k_decoder_block_dw(BlockDwArgs A) {
  using G = Geo<U>;
  extern __shared__ __align__(16) unsigned char lds[];
  // the four channel quarters of a slice on one XCD (blockIdx % 8): the later reads of the slice's P rows are L2 hits
  const int quarter = (blockIdx.x >> 3) & 3;
  const int s = (int)(blockIdx.x & 7) + 8 * (int)(blockIdx.x >> 5);      // (S is a multiple of 8)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nb = wv & 3;                                // this wavefront's 32 input channels
  const int tap0 = (wv >> 2) * 5, ntap = wv < 4 ? 5 : 4;      // ... and taps (uniform per wavefront)
  float* cst = reinterpret_cast<float*>(lds + 2 * G::Buf);            // a (128), b (128), bg (128) as fp32
  int4* tokinfo = reinterpret_cast<int4*>(lds + 2 * G::Buf + 3 * kC * 4);      // (b, y0, x0) of every token of the slice
  int* rowidx = reinterpret_cast<int*>(lds + 2 * G::Buf + 3 * kC * 4 + kMaxTok * 16);      // [3][HRP]: dY row of a chunk's halo rows / -1
  if (tid < kC) {
    cst[tid] = A.a[tid];
    cst[kC + tid] = A.b[tid];
    cst[2 * kC + tid] = __uint_as_float((unsigned)A.bg[tid] << 16);
  }
  const long long chunk0 = (long long)s * A.cps;        // first chunk of the slice
  const long long total_chunks = (A.n + kChunk - 1) / kChunk;
  const int nc = (int)(chunk0 + A.cps <= total_chunks ? A.cps : total_chunks - chunk0);      // chunks with rows (the rest of the
                                                        // slice grid is padding: gdmae_tap_dw multiplies zeros there)
  if (nc <= 0) {                                        // uniform: a slice of padding only
    float* z = A.part + (((long long)s * 9) * kC + quarter * kQ) * kC;
    for (int e = tid; e < 9 * kQ * kC; e += 512) z[((long long)(e / (kQ * kC)) * kC) * kC + e % (kQ * kC)] = 0.f;
    return;
  }
  // ---- the first cell of every token of the slice, decoded once (nc * TPC <= kMaxTok tokens)
  for (int t = tid; t < nc * G::TPC; t += 512) {
    const long long tok = chunk0 * G::TPC + t;
    const int sv = A.site[(tok < A.ntok ? tok : A.ntok - 1) * (U * U)];
    const int x0 = sv % A.W, r = sv / A.W;
    const int y0 = tok < A.ntok ? r % A.H : -(1 << 20);            // no such token: every halo cell is outside the map
    tokinfo[t] = make_int4(r / A.H, y0, x0, 0);
  }

  // ---- halo row tid of a chunk (threads < HRP: whole wavefronts): tile slot requested (resolve_a), dY row published (resolve_b)
  const int pc = tid & 3;                               // this thread's 16-byte piece of the 64-byte quarter rows it copies
  int slotv = -1, locv = -1;
  auto resolve_a = [&](int cc) {
    if (tid < G::HRP) {
      const int ce = cc < nc ? cc : nc - 1;             // (chunks behind the slice are requested and staged, never multiplied)
      const int tl = tid / G::HS, rem = tid - tl * G::HS;
      const int hy = rem / G::HW, hx = rem - hy * G::HW;
      const int4 t = tokinfo[ce * G::TPC + (tl < G::TPC ? tl : 0)];
      const int yy = t.y + hy - 1, xx = t.z + hx - 1;
      const bool in = tl < G::TPC && yy >= 0 && yy < A.H && xx >= 0 && xx < A.W;
      slotv = A.tile_slot[in ? (t.x * A.TH + (yy >> 3)) * A.TW + (xx >> 3) : 0];
      locv = in ? (yy & 7) * 8 + (xx & 7) : -1;
    }
  };
  auto resolve_b = [&](int cc) {
    if (tid < G::HRP) rowidx[(cc % 3) * G::HRP + tid] = (locv >= 0 && slotv >= 0) ? slotv * 64 + locv : -1;
  };
  uint4 dq[G::NP], xq[2];
  unsigned dkeep = 0u;
  auto load_x = [&](int cc) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      long long r = (chunk0 + cc) * kChunk + (tid >> 4) + 32 * j;
      if (r > A.n - 1) r = A.n - 1;
      xq[j] = *reinterpret_cast<const uint4*>(A.P + r * kC + (tid & 15) * 8);
    }
  };
  auto load_d = [&](int cc) {
    unsigned k = 0u;
#pragma unroll
    for (int p = 0; p < G::NP; ++p) {
      const int rix = rowidx[(cc % 3) * G::HRP + ((p * 512 + tid) >> 2)];
      const bool ok = rix >= 0;
      const long long row = ok ? rix : 0;
      k |= ok ? 1u << p : 0u;
      dq[p] = *reinterpret_cast<const uint4*>(A.dY + row * kC + quarter * kQ + pc * 8);
    }
    dkeep = k;
  };
  auto stage_d = [&](int cc) {
    unsigned char* bd = lds + (cc & 1) * G::Buf + kXBytes;
#pragma unroll
    for (int p = 0; p < G::NP; ++p) {
      const int hr = (p * 512 + tid) >> 2;
      int lrow = hr;
      if (U == 2) {
        const int tl = hr / G::HS, rem = hr - tl * G::HS;
        lrow = tl * G::LT + (rem >> 2) * kHP + (rem & 3);
      }
      const unsigned m = ((dkeep >> p) & 1u) ? 0xFFFFFFFFu : 0u;
      uint4 q = dq[p];
      q.x &= m; q.y &= m; q.z &= m; q.w &= m;
      *reinterpret_cast<uint4*>(bd + dy_off(lrow) + pc * 16) = q;
    }
  };
  auto stage_x = [&](int cc) {
    unsigned char* bx = lds + (cc & 1) * G::Buf;
    const int c8 = (tid & 15) * 8;
    const float4* cq = reinterpret_cast<const float4*>(cst + c8);
    const float4 a0 = cq[0], a1 = cq[1], b0 = cq[kC / 4], b1 = cq[kC / 4 + 1], g0 = cq[kC / 2], g1 = cq[kC / 2 + 1];
    const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w}, bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    const float gv[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int rl = (tid >> 4) + 32 * j;
      const unsigned w[4] = {xq[j].x, xq[j].y, xq[j].z, xq[j].w};
      float o[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        o[2 * i] = __uint_as_float(w[i] << 16);
        o[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {                     // bf16(bf16(relu(a p + b)) - bg): gdmae_rows_affine_relu_sub's value
        const float h = fmaf(av[i], o[i], bv[i]);
        const float z = h > 0.f ? h : 0.f;
        o[i] = __uint_as_float((unsigned)gd_to_bf16(z) << 16) - gv[i];
      }
      const unsigned m = (chunk0 + cc) * kChunk + rl < A.n ? 0xFFFFFFFFu : 0u;
      uint4 q;
      q.x = gd_pack_bf16(o[0], o[1]) & m; q.y = gd_pack_bf16(o[2], o[3]) & m;
      q.z = gd_pack_bf16(o[4], o[5]) & m; q.w = gd_pack_bf16(o[6], o[7]) & m;
      *reinterpret_cast<uint4*>(bx + x_off(rl, tid & 15)) = q;
    }
  };

  // ---- fragment addresses of k-step 0 (k-step ks adds 16 Zd rows / KSR halo rows: neither changes the swizzle)
  const int li = lane & 15, grp = (lane >> 4) & 1, h = lane >> 5;
  const int q4 = li >> 2, inl = 32 * grp + 8 * (li & 3);
  int xa[2], da[5][2];
  {
    const int r0 = 8 * h + q4;
    xa[0] = r0 * 256 + ((nb ^ (r0 & 3)) << 6) + inl;
    xa[1] = (r0 + 4) * 256 + ((nb ^ ((r0 + 4) & 3)) << 6) + inl;
    int c0, c1;                                         // centre rows of sites r0 and r0 + 4 of the k-step
    if (U == 4) {
      c0 = ((r0 >> 2) + 1) * kHP + (r0 & 3) + 1;
      c1 = c0 + kHP;
    } else {
      c0 = (r0 >> 2) * G::LT + (((r0 >> 1) & 1) + 1) * kHP + (r0 & 1) + 1;
      c1 = c0 + G::LT;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int tap = tap0 + k < 9 ? tap0 + k : 8;
      const int off = (tap / 3 - 1) * kHP + (tap % 3 - 1);      // a tap reads the row of site - offset(tap)
      da[k][0] = dy_off(c0 - off) + inl;
      da[k][1] = dy_off(c1 - off) + inl;
    }
  }

  f32x16 acc[5];
#pragma unroll
  for (int k = 0; k < 5; ++k)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[k][e] = 0.f;

  // ---- fill the pipeline.  In the loop the rows of chunk c + 2 are requested right after chunk c + 1 left the same registers for
  // LDS, BEFORE the barrier: they have a whole iteration (barrier, resolving, the products of chunk c + 1) to land.  The resolved rows
  // they need were published at the top of the iteration before (a ring of three tables: one written, one read, one between).
  __syncthreads();                                      // token table, constants
  resolve_a(0);
  resolve_b(0);
  resolve_a(1);
  resolve_b(1);
  resolve_a(2);
  __syncthreads();
  load_d(0);
  load_x(0);
  stage_d(0);
  stage_x(0);
  load_d(1);
  load_x(1);
  resolve_b(2);
  resolve_a(3);
  __syncthreads();

  for (int c = 0; c < nc; ++c) {
    resolve_b(c + 3);                                   // -> rowidx[c % 3], last read two iterations ago
    resolve_a(c + 4);
    __builtin_amdgcn_sched_barrier(0);                  // the slot request goes out before the products
    const unsigned char* bx = lds + (c & 1) * G::Buf;
    const unsigned char* bd = bx + kXBytes;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const bf16x8 xf = tr_frag(bx + xa[0] + ks * 16 * 256, bx + xa[1] + ks * 16 * 256);
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        if (k < ntap) {                                 // (scalar condition: EXEC stays whole for the transposed reads)
          const bf16x8 df = tr_frag(bd + da[k][0] + ks * G::KSR * 64, bd + da[k][1] + ks * G::KSR * 64);
          acc[k] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df, xf, acc[k], 0, 0, 0);
        }
      }
    }
    stage_d(c + 1);                                     // the other buffer: last read before the previous barrier
    stage_x(c + 1);
    load_d(c + 2);                                      // rowidx[(c + 2) % 3], published an iteration ago
    load_x(c + 2);
    __syncthreads();
  }

  // ---- partial tiles: D[row = co by register, column = ci by lane]
  float* out = A.part + (((long long)s * 9 + tap0) * kC + quarter * kQ) * kC + nb * 32 + (lane & 31);
#pragma unroll
  for (int k = 0; k < 5; ++k)
    if (k < ntap) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        out[((long long)k * kC + m) * kC] = acc[k][e];
      }
    }
}

// out[(k * 128 + co) * ld_out + m_off + ci] += sum_s part[s][k][co][ci], slices in order
__global__ __launch_bounds__(256) void k_block_dw_reduce(const float* __restrict__ part, int S, float* __restrict__ out, int ld_out, int m_off) {
  constexpr int total = 9 * kC * kC;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const float* p = part + e;
  float acc = 0.f;
  int s = 0;
  for (; s + 16 <= S; s += 16) {                        // sixteen slices requested before the first is added, added in slice order
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = p[(long long)(s + j) * total];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc += v[j];
  }
  for (; s < S; ++s) acc += p[(long long)s * total];
  out[(long long)(e / kC) * ld_out + m_off + (e % kC)] += acc;
}

// slices of a stage: gdmae_tap_dw's (spconv.hip tap_dw_pick) - the same slice count and rows per slice give the same sums
void block_dw_pick(long long n, int* S, int* cps) {
  static const int wgs = getenv("GDMAE_SPCONV_DW_WGS") ? atoi(getenv("GDMAE_SPCONV_DW_WGS")) : 640;
  long long n_pad = 0;
  *S = gd_dw_pick(n, 9, wgs, &n_pad);
  *cps = (int)(n_pad / *S / kChunk);
}
bool block_dw_fits(int u, int cps) { return cps <= (u == 4 ? Geo<4>::MaxCps : Geo<2>::MaxCps); }

template <int U>
int block_dw_launch(const BlockDwArgs& A, hipStream_t st) {
  using G = Geo<U>;
  constexpr int lds = 2 * G::Buf + 3 * kC * 4 + kMaxTok * 16 + 3 * G::HRP * 4;
  static bool once = false;
  if (!once) {
    GD_CHECK(hipFuncSetAttribute((const void*)k_decoder_block_dw<U>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    once = true;
  }
  hipLaunchKernelGGL((k_decoder_block_dw<U>), dim3(4u * (unsigned)A.S), dim3(512), lds, st, A);
  GD_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// 0: the stage is not served (u other than 2 / 4, or more tokens per slice than the kernel's token table holds) - the caller keeps
// the rulebook path
extern "C" size_t gdmae_decoder_block_dw_workspace_bytes(long long n, int u) {
  if (u != 2 && u != 4) return 0;
  if (n <= 0) return 256;
  int S = 0, cps = 0;
  block_dw_pick(n, &S, &cps);
  if (!block_dw_fits(u, cps)) return 0;
  return gd_align((size_t)S * 9 * kC * kC * sizeof(float));
}

extern "C" int gdmae_decoder_block_dw(const void* P, const float* a, const float* b, const void* bg, const int* site, long long n, int u,
                                      const void* dYc, const int* tile_slot, int H, int W, float* out, int ld_out, int m_off,
                                      void* workspace, void* stream) {
  GD_REQUIRE(u == 2 || u == 4, "decoder_block_dw: u must be 2 or 4");
  GD_REQUIRE(n >= 0 && n % (u * u) == 0, "decoder_block_dw: rows must be whole tokens (u * u sites each)");
  if (n == 0) return 0;
  GD_REQUIRE(n < (1ll << 31) && H > 0 && W > 0 && H % u == 0 && W % u == 0, "decoder_block_dw: map size");
  hipStream_t st = (hipStream_t)stream;
  BlockDwArgs A{(const unsigned short*)P, a, b, (const unsigned short*)bg, site, (const unsigned short*)dYc, tile_slot, (float*)workspace,
                n, (int)(n / (u * u)), H, W, (H + 7) / 8, (W + 7) / 8, 0, 0};
  block_dw_pick(n, &A.S, &A.cps);
  GD_REQUIRE(A.S % 8 == 0 && block_dw_fits(u, A.cps), "decoder_block_dw: too many tokens per slice (gdmae_decoder_block_dw_workspace_bytes returns 0)");
  {
    // algorithmic bytes: the P rows and the dY rows once, the site cells, the partial tiles
    GdTimed timed(GD_T_DEC_CONV_BWD, st, (double)n * (2.0 * kC + 2.0 * kC + 4.0) + 36.0 * A.S * kC * kC, 2.0 * n * 9.0 * kC * kC);
    const int rc = u == 4 ? block_dw_launch<4>(A, st) : block_dw_launch<2>(A, st);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_block_dw_reduce, dim3(gd_div_up(9ll * kC * kC, 256)), dim3(256), 0, st, (const float*)workspace, A.S, out, ld_out, m_off);
  GD_LAUNCH_CHECK();
  return 0;
}
