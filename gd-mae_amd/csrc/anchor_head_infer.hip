// Anchor head at inference, from the BEV map to the compacted survivors of the score threshold, in two launches.
//
// The training-time path (anchor_head.hip) writes the 1 x 1 convolutions' fp32 rows, decodes every anchor into dense (B, A, .) arrays
// and then scans the class logits again for the few anchors at or above the threshold.  Here nothing dense leaves the chip:
//   k_ahi_tile     one workgroup per tile of 128 consecutive sites of ONE sample: the three convolutions as one product
//                  Y^T = W X^T on v_mfma_f32_32x32x16_bf16 (bf16 operands, fp32 accumulation, + the fp32 bias; the logits are never
//                  rounded), the fp32 logits of the tile staged in LDS, then per anchor the best-class score and - for anchors with
//                  score >= thresh only - the decoded box, written in anchor order to the tile's own staging slots together with the
//                  tile's survivor count.  With rows_out the tile's logits are also stored (the head_maps / test path).
//   k_ahi_gather   per sample, the exclusive scan of its tile counts and the copy of every tile's survivors to their final position.
// A workgroup never waits for another one (no look-back, no flags, no output-position atomics): the staging slots of a tile are fixed
// by its index, so the result does not depend on scheduling and two calls agree bit for bit.
// Output width: K (C + 7 + nb) <= 96 columns, padded to 96 = three 32-row blocks of the 32 x 32 x 16 form (the shipped head has 72).
// The alternative, 80 = five blocks of the 16 x 16 x 32 form, has 17 % fewer matrix-core cycles, but the launch is bound by reading X
// (256 B per site against 24 MFMAs per 32 sites); the 32-wide form needs 3 instead of 5 weight-fragment reads per k-step and leaves
// each lane four consecutive channels of one site per register group, which go to the LDS tile as 16-byte stores.
// Score / label / decode arithmetic: anchor_decode.h, shared with k_ah_select / k_ah_decode.
#include "anchor_decode.h"
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

namespace {
constexpr int kRows = 128;                 // sites per tile (four wavefronts, 32 sites each)
constexpr int kCols = 96;                  // padded output width
constexpr int kSP = kCols * 4 + 16;        // bytes per site of the fp32 logit tile in LDS
constexpr int kGatherTiles = 16;           // tiles per workgroup of the gather launch (one per wavefront)
constexpr int kMaxCin = 256;
constexpr int kMaxCls = 8;
constexpr int kMaxBins = 8;

union AiFrag {
  uint4 q;
  bf16x8 v;
};

inline size_t ahi_image_bytes(int cin) { return (size_t)kCols * cin * 2; }
inline int ahi_lds_bytes(int cin) {
  const int prod = kRows * (cin * 2 + 16) + (int)ahi_image_bytes(cin), stage = kRows * kSP;
  return prod > stage ? prod : stage;
}

// image: uint4 [j = 0..2][ks = 0..cin/16)[lane]: W[n = 32 j + (lane & 31)][k = 16 ks + 8 (lane >> 5) + 0..7] as bf16, rows
// [cls K*C | box K*7 | dir K*nb | zeros]; then the fp32 bias (96)
__global__ __launch_bounds__(256) void k_ahi_pack(const float* __restrict__ w_cls, const float* __restrict__ b_cls, const float* __restrict__ w_box,
                                                  const float* __restrict__ b_box, const float* __restrict__ w_dir,
                                                  const float* __restrict__ b_dir, int cin, int n_cls, int n_box, int n_dir,
                                                  uint4* __restrict__ image, float* __restrict__ bias) {
  const int KS = cin / 16, total = 3 * KS * 64;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
    const int lane = e & 63, ks = (e >> 6) % KS, j = (e >> 6) / KS;
    const int n = 32 * j + (lane & 31), k0 = 16 * ks + 8 * (lane >> 5);
    const float* src = nullptr;
    if (n < n_cls) src = w_cls + (long long)n * cin;
    else if (n < n_cls + n_box) src = w_box + (long long)(n - n_cls) * cin;
    else if (n < n_cls + n_box + n_dir) src = w_dir + (long long)(n - n_cls - n_box) * cin;
    float f[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = src ? src[k0 + i] : 0.f;
    image[e] = make_uint4(gd_pack_bf16(f[0], f[1]), gd_pack_bf16(f[2], f[3]), gd_pack_bf16(f[4], f[5]), gd_pack_bf16(f[6], f[7]));
  }
  if (blockIdx.x == 0 && threadIdx.x < kCols) {
    const int n = threadIdx.x;
    float v = 0.f;
    if (n < n_cls) v = b_cls ? b_cls[n] : 0.f;
    else if (n < n_cls + n_box) v = b_box ? b_box[n - n_cls] : 0.f;
    else if (n < n_cls + n_box + n_dir) v = b_dir ? b_dir[n - n_cls - n_box] : 0.f;
    bias[n] = v;
  }
}

struct AiWs {
  int* cnt;          // (B, T)
  int* idx;          // (B, T, 128 K)
  float* score;
  int* label;
  float* box;        // (B, T, 128 K, 7)
};
inline size_t ahi_ws(void* ws, int B, int T, int K, AiWs* w) {
  const size_t slots = (size_t)B * T * kRows * K;
  char* p = (char*)ws;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* r = p + off; off += gd_align(bytes); return r; };
  int* cnt = (int*)take((size_t)B * T * sizeof(int));
  int* idx = (int*)take(slots * sizeof(int));
  float* score = (float*)take(slots * sizeof(float));
  int* label = (int*)take(slots * sizeof(int));
  float* box = (float*)take(slots * 7 * sizeof(float));
  if (w) *w = AiWs{cnt, idx, score, label, box};
  return off;
}

struct AiArgs {
  const uint4* X;            // (B n_loc, cin) bf16 rows
  const uint4* image;
  const float* bias;
  int n_loc, W, cin, K, C, nb, T;
  const float *xc, *yc, *slot;
  float dir_offset, dir_limit_offset, thresh;
  float* rows_out;           // optional (B n_loc, K (C + 7 + nb)) fp32
  AiWs ws;
};

// grid (T, B): tile t of sample b = its sites [128 t, min(128 t + 128, n_loc))
__global__ __launch_bounds__(256) void k_ahi_tile(AiArgs A) {
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ int s_wave[4];
  __shared__ int s_base;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int t = blockIdx.x, b = blockIdx.y;
  const int loc0 = t * kRows;
  const int nrows = A.n_loc - loc0 < kRows ? A.n_loc - loc0 : kRows;
  const long long site0 = (long long)b * A.n_loc + loc0;
  const int XP = A.cin * 2 + 16, cpr = A.cin / 8, KS = A.cin / 16;
  unsigned char* lds_w = lds + kRows * XP;
  if (tid == 0) s_base = 0;
  for (int i = tid; i < kRows * cpr; i += 256) {
    const int row = i / cpr, c = i - row * cpr;
    uint4 q = make_uint4(0u, 0u, 0u, 0u);
    if (row < nrows) q = A.X[(site0 + row) * cpr + c];
    *(uint4*)(lds + row * XP + c * 16) = q;
  }
  for (int i = tid; i < 3 * KS * 64; i += 256) ((uint4*)lds_w)[i] = A.image[i];
  __syncthreads();
  f32x16 acc[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
  {
    const unsigned char* xp = lds + (32 * wv + (lane & 31)) * XP + (lane >> 5) * 16;
    const uint4* wp = (const uint4*)lds_w + lane;
    for (int ks = 0; ks < KS; ++ks) {
      AiFrag xf;
      xf.q = *(const uint4*)(xp + ks * 32);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        AiFrag wf;
        wf.q = wp[(j * KS + ks) * 64];
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf.v, xf.v, acc[j], 0, 0, 0);
      }
    }
  }
  __syncthreads();                       // every wavefront is done with the operand tiles: the logit tile takes their place
  {   // accumulator (row = channel in the registers, column = site on the lane) + bias -> [site][channel] fp32
    const int row = 32 * wv + (lane & 31);
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ch = 32 * j + 8 * q + 4 * (lane >> 5);
        const float4 bv = *(const float4*)(A.bias + ch);
        *(float4*)(lds + row * kSP + ch * 4) =
            make_float4(acc[j][4 * q] + bv.x, acc[j][4 * q + 1] + bv.y, acc[j][4 * q + 2] + bv.z, acc[j][4 * q + 3] + bv.w);
      }
  }
  __syncthreads();
  const int ncols = A.K * (A.C + 7 + A.nb);
  if (A.rows_out) {
    float* dst = A.rows_out + site0 * ncols;                     // the tile's rows are contiguous
    for (int i = tid; i < nrows * ncols; i += 256) {
      const int row = i / ncols, c = i - row * ncols;
      dst[i] = *(const float*)(lds + row * kSP + c * 4);
    }
  }
  const int n_anchor = nrows * A.K;
  const long long slot0 = ((long long)b * A.T + t) * kRows * A.K;
  for (int a0 = 0; a0 < n_anchor; a0 += 256) {                  // uniform trip count: the barriers below are reached by all
    const int a = a0 + tid;
    float best = -1.f;
    int arg = 0, row = 0, k = 0;
    bool ok = false;
    const float* r = nullptr;
    if (a < n_anchor) {
      row = a / A.K;
      k = a - row * A.K;
      r = (const float*)(lds + row * kSP);
      const float* q = r + k * A.C;
      ah_best_class([&](int c) { return q[c]; }, A.C, 0, best, arg);
      ok = best >= A.thresh;
    }
    const unsigned long long m = __ballot(ok);
    if (lane == 0) s_wave[wv] = __popcll(m);
    __syncthreads();
    int off = s_base;
    for (int w = 0; w < wv; ++w) off += s_wave[w];
    if (ok) {
      const long long o = slot0 + off + __popcll(m & ((1ull << lane) - 1ull));
      const int loc = loc0 + row;
      const int x = loc % A.W, y = loc / A.W;
      const float* pb = r + A.K * A.C + k * 7;
      const float* pd = r + A.K * (A.C + 7) + k * A.nb;
      float bx[7];
      ah_decode_box([&](int i) { return pb[i]; }, [&](int d) { return pd[d]; }, A.nb, A.xc[x], A.yc[y], A.slot + k * 5, A.dir_offset,
                    A.dir_limit_offset, bx);
      A.ws.idx[o] = loc * A.K + k;
      A.ws.score[o] = best;
      A.ws.label[o] = arg + 1;
#pragma unroll
      for (int i = 0; i < 7; ++i) A.ws.box[o * 7 + i] = bx[i];
    }
    __syncthreads();
    if (tid == 0) s_base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
  }
  if (tid == 0) A.ws.cnt[b * A.T + t] = s_base;
}

// grid (ceil(T / 16), B), 1024 threads: wavefront w copies the survivors of tile 16 blockIdx.x + w behind those of the sample's earlier tiles
__global__ __launch_bounds__(1024) void k_ahi_gather(AiWs ws, int T, int K, long long A, int* __restrict__ count, int* __restrict__ idx,
                                                     float* __restrict__ score, int* __restrict__ label, float* __restrict__ box) {
  __shared__ int s_part[16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.y, t0 = blockIdx.x * kGatherTiles;
  const int* cnt = ws.cnt + (long long)b * T;
  int part = 0;
  for (int i = tid; i < t0; i += 1024) part += cnt[i];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d);
  if (lane == 0) s_part[wv] = part;
  __syncthreads();
  int off = 0;
  for (int w = 0; w < 16; ++w) off += s_part[w];
  const int c = (lane < kGatherTiles && t0 + lane < T) ? cnt[t0 + lane] : 0;
  int n = 0, total = 0;
  for (int i = 0; i < kGatherTiles; ++i) {
    const int v = __shfl(c, i);
    if (i < wv) off += v;
    if (i == wv) n = v;
    total += v;
  }
  if (blockIdx.x == gridDim.x - 1 && wv == 0 && lane == 0) count[b] = off + total;        // wv == 0: off is the sum in front of t0
  const int t = t0 + wv;
  if (t >= T || n == 0) return;
  const long long src = ((long long)b * T + t) * kRows * K, dst = (long long)b * A + off;
  for (int i = lane; i < n; i += 64) {
    idx[dst + i] = ws.idx[src + i];
    score[dst + i] = ws.score[src + i];
    label[dst + i] = ws.label[src + i];
  }
  for (int i = lane; i < n * 7; i += 64) box[dst * 7 + i] = ws.box[src * 7 + i];
}

inline bool ahi_head_ok(int cin, int K, int C, int nb) {
  return cin >= 32 && cin <= kMaxCin && cin % 32 == 0 && K >= 1 && C >= 1 && C <= kMaxCls && nb >= 0 && nb <= kMaxBins &&
         (long long)K * (C + 7 + nb) <= kCols;
}
#define AHI_HEAD_MSG "anchor_head_infer: cin a multiple of 32 up to 256, K (C + 7 + nb) <= 96 output columns, C <= 8, nb <= 8"
}  // namespace

extern "C" size_t gdmae_anchor_head_infer_packed_bytes(int cin) { return gd_align(ahi_image_bytes(cin > 0 ? cin : 0)) + kCols * sizeof(float); }

// weights (K*C | K*7 | K*nb, cin) fp32 and their biases (null: zero), device; w_dir / b_dir are not read with nb = 0
extern "C" int gdmae_anchor_head_infer_pack(const float* w_cls, const float* b_cls, const float* w_box, const float* b_box, const float* w_dir,
                                            const float* b_dir, int cin, int K, int C, int nb, void* packed, void* stream) {
  GD_REQUIRE(ahi_head_ok(cin, K, C, nb), AHI_HEAD_MSG);
  GD_REQUIRE(w_cls && w_box && (nb == 0 || w_dir) && packed, "anchor_head_infer_pack: bad arguments");
  float* bias = (float*)((char*)packed + gd_align(ahi_image_bytes(cin)));
  hipLaunchKernelGGL(k_ahi_pack, dim3(gd_div_up(3 * (cin / 16) * 64, 256)), dim3(256), 0, (hipStream_t)stream, w_cls, b_cls, w_box, b_box, w_dir,
                     b_dir, cin, K * C, K * 7, K * nb, (uint4*)packed, bias);
  GD_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t gdmae_anchor_head_infer_workspace_bytes(int B, int H, int W, int K) {
  if (B < 1 || H < 1 || W < 1 || K < 1) return 0;
  return ahi_ws(nullptr, B, gd_div_up((long long)H * W, kRows), K, nullptr);
}

// X (B H W, cin) bf16 channels-last rows; packed: gdmae_anchor_head_infer_pack; xc (W), yc (H), slot (K, 5): the anchor tables of
// gdmae_anchor_decode.  Per sample b: count[b] anchors with best-class sigmoid score >= thresh, in anchor order
// (a = (y W + x) K + k): idx / label (1-based) int32 (B, A), score (B, A), box (B, A, 7) fp32, A = H W K; entries at or beyond
// count[b] are not written.  rows_out (optional): (B H W, K (C + 7 + nb)) fp32 logits [cls | box | dir].
extern "C" int gdmae_anchor_head_infer(const void* X, int B, int H, int W, int cin, int K, int C, int nb, const void* packed, const float* xc,
                                       const float* yc, const float* slot, float dir_offset, float dir_limit_offset, float thresh,
                                       float* rows_out, int* count, int* idx, float* score, int* label, float* box, void* workspace,
                                       void* stream) {
  GD_REQUIRE(ahi_head_ok(cin, K, C, nb), AHI_HEAD_MSG);
  GD_REQUIRE(X && packed && xc && yc && slot && count && idx && score && label && box && workspace && B >= 1 && H >= 1 && W >= 1,
             "anchor_head_infer: bad arguments");
  const long long n_loc = (long long)H * W;
  GD_REQUIRE(n_loc * K < (1ll << 31) && B <= 65535, "anchor_head_infer: anchors per sample must fit 31 bits, B <= 65535");
  hipStream_t st = (hipStream_t)stream;
  const int T = gd_div_up(n_loc, kRows);
  AiArgs A;
  A.X = (const uint4*)X;
  A.image = (const uint4*)packed;
  A.bias = (const float*)((const char*)packed + gd_align(ahi_image_bytes(cin)));
  A.n_loc = (int)n_loc; A.W = W; A.cin = cin; A.K = K; A.C = C; A.nb = nb; A.T = T;
  A.xc = xc; A.yc = yc; A.slot = slot;
  A.dir_offset = dir_offset; A.dir_limit_offset = dir_limit_offset; A.thresh = thresh;
  A.rows_out = rows_out;
  ahi_ws(workspace, B, T, K, &A.ws);
  static bool once = false;
  if (!once) {
    GD_CHECK(hipFuncSetAttribute((const void*)k_ahi_tile, hipFuncAttributeMaxDynamicSharedMemorySize, ahi_lds_bytes(kMaxCin)));
    once = true;
  }
  hipLaunchKernelGGL(k_ahi_tile, dim3(T, B), dim3(256), ahi_lds_bytes(cin), st, A);
  GD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ahi_gather, dim3(gd_div_up(T, kGatherTiles), B), dim3(1024), 0, st, A.ws, T, K, n_loc * K, count, idx, score, label, box);
  GD_LAUNCH_CHECK();
  return 0;
}
