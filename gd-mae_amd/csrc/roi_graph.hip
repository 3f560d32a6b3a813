// Second stage of the two-stage detector after the pooling (GraphRCNNHead in eval mode): the graph network over the 256
// pooled points of a RoI, the shared layer, the two heads, the box decoding and the score fusion, specialised to the shipped
// ATTN_GNN_CONFIG (IN_DIM 11, MLPS [32, 32, 64], CALIB_DIM 64, EXP_MLPS [512], OUT_DIM 256, K 8, reduction + shortcut).
//
//   k_roi_graph   one 256-thread workgroup per RoI, everything in LDS: neighbour search (thread = slot, sorted top-8 in registers),
//                 edge layer 1 in fp32, edge layers 2 / 3, the calib gate and the expansion on the matrix cores (bf16 operands, fp32
//                 accumulation), the expansion's max over the slots in its epilogue -> 512 fp32 values per RoI
//   k_roi_tail    8 RoIs per workgroup, fp32: reduction, shortcut block, shared layer, heads, decode, score fusion
//
// An edge layer max_j ReLU(a (W [x_j - x_i ; x_i]) + b) is evaluated as ReLU(max_j P_j + Q_i) with P = (a W_nbr) x and
// Q = (a (W_ctr - W_nbr)) x + b: two products per slot and an 8-way gather-max over LDS, no edge tensor.  The BatchNorm scale is
// folded into the weights BEFORE the max (it may be negative).  No atomics; a RoI's result depends on its own rows only.
#include "common.h"
#include "../../include/gdmae_hip.h"

#include <math.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int RG_K = 256;            // slots per RoI (NUM_FPS_POINTS)
constexpr int RG_IN = 11;            // IN_DIM
constexpr int RG_NN = 8;             // neighbours
constexpr int RG_EXP = 512;          // EXP_MLPS[0]
constexpr int RG_OUT = 256;          // OUT_DIM and the shared layer
constexpr int RG_TAIL_ROIS = 8;

// ---- the folded fp32 weights the pack call reads (float offsets), [out][in] row-major
constexpr int F_E1P = 0, F_E1Q = F_E1P + 32 * 11, F_E1B = F_E1Q + 32 * 11;
constexpr int F_E2P = F_E1B + 32, F_E2Q = F_E2P + 32 * 32, F_E2B = F_E2Q + 32 * 32;
constexpr int F_E3P = F_E2B + 32, F_E3Q = F_E3P + 64 * 32, F_E3B = F_E3Q + 64 * 32;
constexpr int F_C1W = F_E3B + 64, F_C1B = F_C1W + 64 * 128;
constexpr int F_C2W = F_C1B + 64, F_C2B = F_C2W + 128 * 64;
constexpr int F_EXW = F_C2B + 128, F_EXB = F_EXW + 512 * 128;
constexpr int F_RDW = F_EXB + 512, F_RDB = F_RDW + 256 * 512;
constexpr int F_N1A = F_RDB + 256, F_N1B = F_N1A + 256;
constexpr int F_S1W = F_N1B + 256, F_S1B = F_S1W + 256 * 256;
constexpr int F_S2W = F_S1B + 256, F_S2B = F_S2W + 256 * 256;
constexpr int F_N2A = F_S2B + 256, F_N2B = F_N2A + 256;
constexpr int F_FCW = F_N2B + 256, F_FCB = F_FCW + 256 * 256;
constexpr int F_HDW = F_FCB + 256, F_HDB = F_HDW + 8 * 256;
constexpr int F_TOTAL = F_HDB + 8;

// ---- the packed image: an fp32 part (float offsets), then the bf16 A-operand images (bf16 offsets from the start of that part)
constexpr int I_E1P = 0, I_E1Q = I_E1P + 32 * 11, I_E1B = I_E1Q + 32 * 11;
constexpr int I_E2B = I_E1B + 32, I_E3B = I_E2B + 32, I_C1B = I_E3B + 64, I_C2B = I_C1B + 64, I_EXB = I_C2B + 128;
constexpr int I_RDW = I_EXB + 512, I_RDB = I_RDW + 512 * 256;            // transposed: [in][out]
constexpr int I_N1A = I_RDB + 256, I_N1B = I_N1A + 256;
constexpr int I_S1W = I_N1B + 256, I_S1B = I_S1W + 256 * 256;
constexpr int I_S2W = I_S1B + 256, I_S2B = I_S2W + 256 * 256;
constexpr int I_N2A = I_S2B + 256, I_N2B = I_N2A + 256;
constexpr int I_FCW = I_N2B + 256, I_FCB = I_FCW + 256 * 256;
constexpr int I_HDW = I_FCB + 256, I_HDB = I_HDW + 8 * 256;              // [out][in]
constexpr int I_F32 = (I_HDB + 8 + 63) / 64 * 64;
constexpr int H_E2 = 0, H_E3 = H_E2 + 64 * 32, H_C1 = H_E3 + 128 * 32, H_C2 = H_C1 + 64 * 128, H_EX = H_C2 + 128 * 64;
constexpr int H_TOTAL = H_EX + 512 * 128;
constexpr size_t RG_PACKED_BYTES = (size_t)I_F32 * 4 + (size_t)H_TOTAL * 2;

// ---- LDS of k_roi_graph
constexpr int ACT_LD = 136;          // bf16 per row of the 128-channel tile (272 B: 8-byte operand reads of a half wave hit 64 banks)
constexpr int P_LD = 68;             // floats per row of the P tile
constexpr int HID_LD = 72;           // bf16 per row of the calib hidden tile (lives in the P tile's space)
constexpr size_t L_ACT = 0, L_P = L_ACT + (size_t)RG_K * ACT_LD * 2, L_X = L_P + (size_t)RG_K * P_LD * 4;
constexpr size_t L_NBR = L_X + (size_t)RG_K * RG_IN * 4, RG_LDS_BYTES = L_NBR + RG_K * RG_NN;
static_assert((size_t)RG_K * HID_LD * 2 <= (size_t)RG_K * P_LD * 4, "hidden tile inside the P tile");
static_assert(4 * RG_EXP * 4 <= RG_K * RG_IN * 4, "per-wave maxima inside the input tile");
static_assert(RG_LDS_BYTES <= 160 * 1024, "LDS per CU");

__global__ __launch_bounds__(256) void k_rg_copy(const float* __restrict__ src, float* __restrict__ dst, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}
// src [rows][cols] -> dst [cols][rows]
__global__ __launch_bounds__(256) void k_rg_transpose(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < rows * cols) dst[(i % cols) * rows + i / cols] = src[i];
}
// rows [0, mp) from p, rows [mp, m) from q, both [.][k] -> MFMA 16x16x16 A-operand order: ((tile_m * k/16 + kstep) * 64 + lane) * 4 + e
// holds W[tile_m 16 + lane % 16][kstep 16 + 4 (lane / 16) + e], rounded to bf16 (nearest even)
__global__ __launch_bounds__(256) void k_rg_pack_a(const float* __restrict__ p, const float* __restrict__ q, int mp, int m, int k,
                                                   unsigned short* __restrict__ dst) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m * k) return;
  const int e = i & 3, lane = (i >> 2) & 63, t = i >> 8, ks = t % (k / 16), mt = t / (k / 16);
  const int row = mt * 16 + (lane & 15), col = ks * 16 + 4 * (lane >> 4) + e;
  const float v = row < mp ? p[row * k + col] : q[(row - mp) * k + col];
  dst[i] = gd_to_bf16(v);
}

__device__ __forceinline__ float rg_bf16(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ s16x4 rg_ld4(const unsigned short* p) { return __builtin_bit_cast(s16x4, *(const uint2*)p); }
__device__ __forceinline__ f32x4 rg_mfma(s16x4 a, s16x4 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0); }

// One bf16 edge layer for the wave's 64 slots: [P ; Q] = Wcat act[:, KIN : KIN + 32], P -> s_P, then ReLU(max_j P_j + Q + b) -> bf16
// act[:, KOUT : KOUT + C]
template <int C, int KIN, int KOUT>
__device__ __forceinline__ void rg_edge_layer(const unsigned short* __restrict__ img, const float* __restrict__ bias,
                                              unsigned short* s_act, float* s_P, const unsigned char* s_nbr) {
  constexpr int MT = C / 16;           // channel tiles of P (and of Q)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4;
  f32x4 q[4][MT];
  __syncthreads();                     // the P tile is free (the gather of the layer before is over), the input columns are written
#pragma unroll
  for (int st = 0; st < 4; ++st) {
    const int slot = wave * 64 + st * 16 + col;
    s16x4 b[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) b[ks] = rg_ld4(s_act + slot * ACT_LD + KIN + ks * 16 + quad * 4);
#pragma unroll
    for (int mt = 0; mt < 2 * MT; ++mt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) acc = rg_mfma(rg_ld4(img + ((mt * 2 + ks) * 64 + lane) * 4), b[ks], acc);
      if (mt < MT) *(f32x4*)(s_P + slot * P_LD + mt * 16 + quad * 4) = acc;
      else q[st][mt - MT] = acc;
    }
  }
  __syncthreads();
#pragma unroll
  for (int st = 0; st < 4; ++st) {
    const int slot = wave * 64 + st * 16 + col;
    const uint2 nb = *(const uint2*)(s_nbr + slot * RG_NN);
    int n[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      n[j] = (nb.x >> (8 * j)) & 255;
      n[4 + j] = (nb.y >> (8 * j)) & 255;
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int c0 = mt * 16 + quad * 4;
      f32x4 m = *(const f32x4*)(s_P + n[0] * P_LD + c0);
#pragma unroll
      for (int j = 1; j < 8; ++j) {
        const f32x4 v = *(const f32x4*)(s_P + n[j] * P_LD + c0);
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], v[e]);
      }
      float h[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) h[e] = fmaxf((m[e] + q[st][mt][e]) + bias[c0 + e], 0.f);
      uint2 o;
      o.x = gd_pack_bf16(h[0], h[1]);
      o.y = gd_pack_bf16(h[2], h[3]);
      *(uint2*)(s_act + slot * ACT_LD + KOUT + c0) = o;
    }
  }
}

__global__ __launch_bounds__(256) void k_roi_graph(const float* __restrict__ feats, const int* __restrict__ pooled_num,
                                                   const float* __restrict__ wf, const unsigned short* __restrict__ wh,
                                                   float* __restrict__ gmax, int* __restrict__ nbr_debug) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned short* s_act = (unsigned short*)(lds + L_ACT);
  float* s_P = (float*)(lds + L_P);
  unsigned short* s_hid = (unsigned short*)(lds + L_P);
  float* s_x = (float*)(lds + L_X);
  float* s_max = (float*)(lds + L_X);
  unsigned char* s_nbr = lds + L_NBR;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  const long long roi = blockIdx.x;

  // ---- inputs (an empty RoI: all zero, corner columns included)
  const bool live = pooled_num[roi] > 0;
  const float* src = feats + roi * (RG_K * RG_IN);
  for (int i = tid; i < RG_K * RG_IN; i += 256) s_x[i] = live ? src[i] : 0.f;
  __syncthreads();

  // ---- the 8 nearest slots of slot tid: d = (dx dx + dy dy) + dz dz, the slot itself included, ties to the lowest slot
  float x[RG_IN];
#pragma unroll
  for (int k = 0; k < RG_IN; ++k) x[k] = s_x[tid * RG_IN + k];
  {
    float bd[RG_NN];
    int bi[RG_NN];
#pragma unroll
    for (int k = 0; k < RG_NN; ++k) {
      bd[k] = INFINITY;
      bi[k] = 0;
    }
    for (int j0 = 0; j0 < RG_K; j0 += 8) {
      float dj[8];                     // the LDS reads of 8 candidates go out together
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float* c = s_x + (j0 + u) * RG_IN;
        const float dx = c[0] - x[0], dy = c[1] - x[1], dz = c[2] - x[2];
        dj[u] = (dx * dx + dy * dy) + dz * dz;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float d = dj[u];
        if (d < bd[RG_NN - 1]) {
          bd[RG_NN - 1] = d;
          bi[RG_NN - 1] = j0 + u;
#pragma unroll
          for (int k = RG_NN - 1; k > 0; --k) {
            const bool sw = bd[k] < bd[k - 1];
            const float td = bd[k];
            const int ti = bi[k];
            bd[k] = sw ? bd[k - 1] : td;
            bi[k] = sw ? bi[k - 1] : ti;
            bd[k - 1] = sw ? td : bd[k - 1];
            bi[k - 1] = sw ? ti : bi[k - 1];
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < RG_NN; ++k) s_nbr[tid * RG_NN + k] = (unsigned char)bi[k];
    if (nbr_debug) {
#pragma unroll
      for (int k = 0; k < RG_NN; ++k) nbr_debug[(roi * RG_K + tid) * RG_NN + k] = bi[k];
    }
  }

  // ---- edge layer 1 in fp32 (metre-scale coordinates): thread = slot
  {
    float q[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) {
      float p = wf[I_E1P + c * RG_IN] * x[0], qq = wf[I_E1Q + c * RG_IN] * x[0];
#pragma unroll
      for (int k = 1; k < RG_IN; ++k) {
        p = fmaf(wf[I_E1P + c * RG_IN + k], x[k], p);
        qq = fmaf(wf[I_E1Q + c * RG_IN + k], x[k], qq);
      }
      s_P[tid * P_LD + c] = p;
      q[c] = qq;
    }
    __syncthreads();
    int n[RG_NN];
#pragma unroll
    for (int k = 0; k < RG_NN; ++k) n[k] = s_nbr[tid * RG_NN + k];
#pragma unroll
    for (int c0 = 0; c0 < 32; c0 += 4) {
      f32x4 m = *(const f32x4*)(s_P + n[0] * P_LD + c0);
#pragma unroll
      for (int j = 1; j < RG_NN; ++j) {
        const f32x4 v = *(const f32x4*)(s_P + n[j] * P_LD + c0);
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], v[e]);
      }
      float h[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) h[e] = fmaxf((m[e] + q[c0 + e]) + wf[I_E1B + c0 + e], 0.f);
      uint2 o;
      o.x = gd_pack_bf16(h[0], h[1]);
      o.y = gd_pack_bf16(h[2], h[3]);
      *(uint2*)(s_act + tid * ACT_LD + c0) = o;
    }
  }

  // ---- edge layers 2 and 3 on the matrix cores
  rg_edge_layer<32, 0, 32>(wh + H_E2, wf + I_E2B, s_act, s_P, s_nbr);
  rg_edge_layer<64, 32, 64>(wh + H_E3, wf + I_E3B, s_act, s_P, s_nbr);
  __syncthreads();                     // the concat tile is complete, the P tile is free for the hidden tile

  // ---- calib gate: hid = ReLU(W1 x + b1) in bf16, x <- sigmoid(W2 hid + b2) x; a wave touches its own 64 slots only
#pragma unroll
  for (int st = 0; st < 4; ++st) {
    const int slot = wave * 64 + st * 16 + col;
    f32x4 acc[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const s16x4 b = rg_ld4(s_act + slot * ACT_LD + ks * 16 + quad * 4);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) acc[mt] = rg_mfma(rg_ld4(wh + H_C1 + ((mt * 8 + ks) * 64 + lane) * 4), b, acc[mt]);
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int c0 = mt * 16 + quad * 4;
      float h[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) h[e] = fmaxf(acc[mt][e] + wf[I_C1B + c0 + e], 0.f);
      uint2 o;
      o.x = gd_pack_bf16(h[0], h[1]);
      o.y = gd_pack_bf16(h[2], h[3]);
      *(uint2*)(s_hid + slot * HID_LD + c0) = o;
    }
  }
  __syncthreads();
#pragma unroll
  for (int st = 0; st < 4; ++st) {
    const int slot = wave * 64 + st * 16 + col;
    f32x4 acc[8];
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const s16x4 b = rg_ld4(s_hid + slot * HID_LD + ks * 16 + quad * 4);
#pragma unroll
      for (int mt = 0; mt < 8; ++mt) acc[mt] = rg_mfma(rg_ld4(wh + H_C2 + ((mt * 4 + ks) * 64 + lane) * 4), b, acc[mt]);
    }
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
      const int c0 = mt * 16 + quad * 4;
      const uint2 xin = *(const uint2*)(s_act + slot * ACT_LD + c0);
      const float xv[4] = {rg_bf16(xin.x & 0xFFFF), rg_bf16(xin.x >> 16), rg_bf16(xin.y & 0xFFFF), rg_bf16(xin.y >> 16)};
      float h[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) h[e] = xv[e] * (1.0f / (1.0f + expf(-(acc[mt][e] + wf[I_C2B + c0 + e]))));
      uint2 o;
      o.x = gd_pack_bf16(h[0], h[1]);
      o.y = gd_pack_bf16(h[2], h[3]);
      *(uint2*)(s_act + slot * ACT_LD + c0) = o;
    }
  }
  __syncthreads();

  // ---- expansion 128 -> 512 with the max over the slots in the epilogue: the wave's 64 slots stay in registers as B operands
  {
    s16x4 b[4][8];
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) b[st][ks] = rg_ld4(s_act + (wave * 64 + st * 16 + col) * ACT_LD + ks * 16 + quad * 4);
    constexpr int CH = 4, NCH = RG_EXP / 16 / CH;          // channel tiles per chunk, chunks
    s16x4 a[2][CH][8];
#pragma unroll
    for (int i = 0; i < CH; ++i)
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) a[0][i][ks] = rg_ld4(wh + H_EX + ((i * 8 + ks) * 64 + lane) * 4);
#pragma unroll 2
    for (int ch = 0; ch < NCH; ++ch) {
      const int cur = ch & 1;
      if (ch + 1 < NCH) {
#pragma unroll
        for (int i = 0; i < CH; ++i)
#pragma unroll
          for (int ks = 0; ks < 8; ++ks) a[cur ^ 1][i][ks] = rg_ld4(wh + H_EX + ((((ch + 1) * CH + i) * 8 + ks) * 64 + lane) * 4);
      }
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        const int mt = ch * CH + i;
        f32x4 acc[4];
#pragma unroll
        for (int st = 0; st < 4; ++st) acc[st] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
#pragma unroll
          for (int st = 0; st < 4; ++st) acc[st] = rg_mfma(a[cur][i][ks], b[st][ks], acc[st]);
        float m[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          m[e] = fmaxf(fmaxf(acc[0][e], acc[1][e]), fmaxf(acc[2][e], acc[3][e]));
#pragma unroll
          for (int d = 1; d < 16; d <<= 1) m[e] = fmaxf(m[e], __shfl_xor(m[e], d, GD_WAVE));
        }
        if (col == 0) *(f32x4*)(s_max + wave * RG_EXP + mt * 16 + quad * 4) = f32x4{m[0], m[1], m[2], m[3]};
      }
    }
  }
  __syncthreads();
  for (int c = tid; c < RG_EXP; c += 256) {
    const float m = fmaxf(fmaxf(s_max[c], s_max[RG_EXP + c]), fmaxf(s_max[2 * RG_EXP + c], s_max[3 * RG_EXP + c]));
    gmax[roi * RG_EXP + c] = fmaxf(m + wf[I_EXB + c], 0.f);
  }
}

// y[r][c] = sum_k WT[k][c] v[r][k] for the workgroup's rows; thread = output channel
template <int KDIM>
__device__ __forceinline__ void rg_rows_dot(const float* __restrict__ wt, const float* s_v, int ld, float* acc) {
  const int c = threadIdx.x;
#pragma unroll
  for (int r = 0; r < RG_TAIL_ROIS; ++r) acc[r] = 0.f;
#pragma unroll 2
  for (int k = 0; k < KDIM; k += 4) {
    float w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) w[u] = wt[(k + u) * RG_OUT + c];
#pragma unroll
    for (int r = 0; r < RG_TAIL_ROIS; ++r) {
      const f32x4 v = *(const f32x4*)(s_v + r * ld + k);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[r] = fmaf(w[u], v[u], acc[r]);
    }
  }
}

__global__ __launch_bounds__(256) void k_roi_tail(const float* __restrict__ gmax, const float* __restrict__ wf, const float* __restrict__ rois,
                                                  int roi_cols, const float* __restrict__ roi_scores, int total, int scores_normalized,
                                                  float* __restrict__ rcnn_cls, float* __restrict__ rcnn_reg,
                                                  float* __restrict__ box_out, float* __restrict__ cls_out) {
  __shared__ __attribute__((aligned(16))) float s_v[RG_TAIL_ROIS * RG_EXP];
  __shared__ __attribute__((aligned(16))) float s_a[RG_TAIL_ROIS * RG_OUT];
  __shared__ __attribute__((aligned(16))) float s_b[RG_TAIL_ROIS * RG_OUT];
  __shared__ float s_o[RG_TAIL_ROIS * 8];
  const int tid = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * RG_TAIL_ROIS;
  for (int i = tid; i < RG_TAIL_ROIS * RG_EXP; i += 256) {
    const long long row = r0 + i / RG_EXP;
    s_v[i] = row < total ? gmax[row * RG_EXP + i % RG_EXP] : 0.f;
  }
  __syncthreads();
  float acc[RG_TAIL_ROIS];
  // reduction + BatchNorm + ReLU, then norm1 of x + dropout1(x) = 2 x (the 2 is folded into n1_a)
  rg_rows_dot<RG_EXP>(wf + I_RDW, s_v, RG_EXP, acc);
#pragma unroll
  for (int r = 0; r < RG_TAIL_ROIS; ++r) s_a[r * RG_OUT + tid] = wf[I_N1A + tid] * fmaxf(acc[r] + wf[I_RDB + tid], 0.f) + wf[I_N1B + tid];
  __syncthreads();
  rg_rows_dot<RG_OUT>(wf + I_S1W, s_a, RG_OUT, acc);
#pragma unroll
  for (int r = 0; r < RG_TAIL_ROIS; ++r) s_b[r * RG_OUT + tid] = fmaxf(acc[r] + wf[I_S1B + tid], 0.f);
  __syncthreads();
  rg_rows_dot<RG_OUT>(wf + I_S2W, s_b, RG_OUT, acc);
#pragma unroll
  for (int r = 0; r < RG_TAIL_ROIS; ++r)
    s_a[r * RG_OUT + tid] = wf[I_N2A + tid] * (s_a[r * RG_OUT + tid] + (acc[r] + wf[I_S2B + tid])) + wf[I_N2B + tid];
  __syncthreads();
  rg_rows_dot<RG_OUT>(wf + I_FCW, s_a, RG_OUT, acc);
#pragma unroll
  for (int r = 0; r < RG_TAIL_ROIS; ++r) s_b[r * RG_OUT + tid] = fmaxf(acc[r] + wf[I_FCB + tid], 0.f);
  __syncthreads();
  if (tid < RG_TAIL_ROIS * 8) {
    const int r = tid >> 3, o = tid & 7;
    float s = 0.f;
    for (int k = 0; k < RG_OUT; ++k) s = fmaf(wf[I_HDW + o * RG_OUT + k], s_b[r * RG_OUT + k], s);
    s_o[tid] = s + wf[I_HDB + o];
  }
  __syncthreads();
  if (tid < RG_TAIL_ROIS && r0 + tid < total) {
    const long long g = r0 + tid;
    const float* o = s_o + tid * 8;
    const float* roi = rois + g * roi_cols;
    rcnn_cls[g] = o[0];
    for (int k = 0; k < 7; ++k) rcnn_reg[g * 7 + k] = o[1 + k];
    // ResidualCoder decode against the RoI with zeroed centre, rotation by the RoI heading, shift to the centre
    const float dxa = roi[3], dya = roi[4], dza = roi[5], ra = roi[6];
    const float diag = sqrtf(dxa * dxa + dya * dya);
    const float xl = o[1] * diag, yl = o[2] * diag, zl = o[3] * dza;
    const float ca = cosf(ra), sa = sinf(ra);
    float* bx = box_out + g * 7;
    bx[0] = (xl * ca - yl * sa) + roi[0];
    bx[1] = (xl * sa + yl * ca) + roi[1];
    bx[2] = zl + roi[2];
    bx[3] = expf(o[4]) * dxa;
    bx[4] = expf(o[5]) * dya;
    bx[5] = expf(o[6]) * dza;
    bx[6] = o[7] + ra;
    const float rs = roi_scores[g];
    const float ps = scores_normalized ? rs : 1.0f / (1.0f + expf(-rs));
    cls_out[g] = sqrtf(1.0f / (1.0f + expf(-o[0]))) * sqrtf(ps);
  }
}

int rg_launch1(void (*kern)(const float*, float*, int), const float* s, float* d, int n, hipStream_t st) {
  hipLaunchKernelGGL(kern, dim3(gd_div_up(n, 256)), dim3(256), 0, st, s, d, n);
  GD_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" size_t gdmae_roi_graph_folded_floats(void) { return (size_t)F_TOTAL; }
extern "C" size_t gdmae_roi_graph_packed_bytes(void) { return RG_PACKED_BYTES; }
extern "C" size_t gdmae_roi_graph_workspace_bytes(long long n_rois_total) {
  return gd_align((size_t)(n_rois_total > 0 ? n_rois_total : 1) * RG_EXP * 4);
}

extern "C" int gdmae_roi_graph_pack(const float* folded, void* packed, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  GD_REQUIRE(folded && packed, "roi_graph_pack: null pointer");
  float* wf = (float*)packed;
  unsigned short* wh = (unsigned short*)((char*)packed + (size_t)I_F32 * 4);
  const int copies[][3] = {{F_E1P, I_E1P, 32 * 11 * 2 + 32}, {F_E2B, I_E2B, 32}, {F_E3B, I_E3B, 64}, {F_C1B, I_C1B, 64},
                           {F_C2B, I_C2B, 128}, {F_EXB, I_EXB, 512}, {F_RDB, I_RDB, 256 * 3}, {F_S1B, I_S1B, 256},
                           {F_S2B, I_S2B, 256 * 3}, {F_FCB, I_FCB, 256}, {F_HDW, I_HDW, 8 * 256 + 8}};
  for (const auto& c : copies)
    if (int rc = rg_launch1(k_rg_copy, folded + c[0], wf + c[1], c[2], st)) return rc;
  const int trans[][4] = {{F_RDW, I_RDW, 256, 512}, {F_S1W, I_S1W, 256, 256}, {F_S2W, I_S2W, 256, 256}, {F_FCW, I_FCW, 256, 256}};
  for (const auto& t : trans) {
    hipLaunchKernelGGL(k_rg_transpose, dim3(gd_div_up(t[2] * t[3], 256)), dim3(256), 0, st, folded + t[0], wf + t[1], t[2], t[3]);
    GD_LAUNCH_CHECK();
  }
  const int mats[][6] = {{F_E2P, F_E2Q, 32, 64, 32, H_E2}, {F_E3P, F_E3Q, 64, 128, 32, H_E3}, {F_C1W, F_C1W, 64, 64, 128, H_C1},
                         {F_C2W, F_C2W, 128, 128, 64, H_C2}, {F_EXW, F_EXW, 512, 512, 128, H_EX}};
  for (const auto& m : mats) {
    hipLaunchKernelGGL(k_rg_pack_a, dim3(gd_div_up(m[3] * m[4], 256)), dim3(256), 0, st, folded + m[0], folded + m[1], m[2], m[3], m[4],
                       wh + m[5]);
    GD_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int gdmae_roi_graph_forward(const float* feats_local, const int* pooled_num, const float* rois, int roi_cols,
                                       const float* roi_scores, int batch, int n_rois, int scores_normalized, const void* packed,
                                       float* rcnn_cls, float* rcnn_reg, float* batch_box_preds, float* batch_cls_preds,
                                       int* nbr_debug, void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  GD_REQUIRE(roi_cols >= 7, "roi_graph_forward: rois need 7 columns");
  if (batch <= 0 || n_rois <= 0) return 0;
  const long long total = (long long)batch * n_rois;
  GD_REQUIRE(total < (1ll << 31) / (RG_K * RG_IN), "roi_graph_forward: RoI count");
  GD_REQUIRE(workspace_bytes >= gdmae_roi_graph_workspace_bytes(total), "roi_graph_forward: workspace too small");
  const float* wf = (const float*)packed;
  const unsigned short* wh = (const unsigned short*)((const char*)packed + (size_t)I_F32 * 4);
  float* gmax = (float*)workspace;
  GD_CHECK(hipFuncSetAttribute((const void*)k_roi_graph, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RG_LDS_BYTES));
  hipLaunchKernelGGL(k_roi_graph, dim3((unsigned)total), dim3(256), RG_LDS_BYTES, st, feats_local, pooled_num, wf, wh, gmax, nbr_debug);
  GD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_roi_tail, dim3(gd_div_up(total, RG_TAIL_ROIS)), dim3(256), 0, st, (const float*)gmax, wf, rois, roi_cols,
                     roi_scores, (int)total, scores_normalized, rcnn_cls, rcnn_reg, batch_box_preds, batch_cls_preds);
  GD_LAUNCH_CHECK();
  return 0;
}
