// RoI point pooling of the two-stage detector (GraphRCNNHead.roipool3d_gpu): for every RoI find its points through a 1 m BEV patch
// grid, thin them to one point per dynamic voxel, run farthest-point sampling and emit canonical-frame features.
//
// The contract is deterministic: the representative of a voxel is its lowest `points` row, a crowded RoI keeps the
// lowest rows, FPS starts at the lowest row and breaks ties towards the lowest row, a crowded patch keeps the lowest RoI indices.
// Nothing below depends on the order in which atomics land: counts are sums, the table keeps a minimum, candidates are sorted.
//
//   k_point_cells   point -> cell of the (B, Y, X) patch grid (or -1: other sample / outside the xy range), cell histogram
//   gd_device_scan  cell starts
//   k_fill_cells    patch -> point CSR (the order inside a cell is arbitrary and never observed)
//   k_roi_spans     truncated patch span of the enlarged RoI's rotated-corner bounding box
//   k_roi_pool      one workgroup per RoI: walk the occupied patches of the span whose capped RoI list holds this RoI, in-box test,
//                   voxel key -> LDS table (64-bit key, atomicMin on the row), sort the rows, FPS out of LDS, features
//
// A RoI with more distinct voxels than the table takes (RP_FILL) repeats the walk with a row limit found by bisection: the voxel
// count of the rows below a limit grows by at most one per row, so a limit exists whose count lies between NUM_DVS_POINTS and
// RP_FILL, and the lowest NUM_DVS_POINTS representatives below it are the lowest of all.  Slower, never truncated.
#include "common.h"
#include "../../include/gdmae_hip.h"

#include <math.h>

namespace {

constexpr int RP_BLOCK = 256;
constexpr int RP_WAVES = RP_BLOCK / GD_WAVE;
constexpr int RP_SLOTS = 4096;                 // LDS table slots (power of two)
constexpr int RP_FILL = 3072;                  // distinct voxels one pass accepts (+ at most RP_BLOCK in flight < RP_SLOTS)
constexpr int RP_MAX_DVS = 1024;               // NUM_DVS_POINTS the FPS arrays are sized for
constexpr int RP_MAX_FPS = 4096;               // NUM_FPS_POINTS the slot list is sized for
constexpr unsigned long long RP_EMPTY = ~0ull;

struct RpGrid {
  float x0, y0, x1, y1;      // xy range of the point filter (inclusive)
  float lo_x, lo_y;          // patch grid origin
  int X, Y;                  // patches per axis
};

__global__ __launch_bounds__(256) void k_point_cells(const float* __restrict__ points, long long n, int cols, int batch, RpGrid g,
                                                     int* __restrict__ point_cell, int* __restrict__ cell_count) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* p = points + i * cols;
  const float bf = p[0], x = p[1], y = p[2];
  const int b = (int)bf;
  int cell = -1;
  if ((float)b == bf && b >= 0 && b < batch && x >= g.x0 && x <= g.x1 && y >= g.y0 && y <= g.y1) {
    int px = (int)(x - g.lo_x), py = (int)(y - g.lo_y);
    px = min(max(px, 0), g.X - 1);
    py = min(max(py, 0), g.Y - 1);
    cell = (b * g.Y + py) * g.X + px;
    atomicAdd(cell_count + cell, 1);
  }
  point_cell[i] = cell;
}

struct RpLoad {
  const int* c;
  __device__ int operator()(long long i) const { return c[i]; }
};
struct RpStore {
  int* start;
  int* cursor;
  __device__ void operator()(long long i, int ex, int) const {
    start[i] = ex;
    cursor[i] = ex;
  }
};

__global__ __launch_bounds__(256) void k_fill_cells(const int* __restrict__ point_cell, long long n, int* __restrict__ cursor,
                                                    int* __restrict__ csr) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int cell = point_cell[i];
  if (cell >= 0) csr[atomicAdd(cursor + cell, 1)] = (int)i;
}

// span of patches [x0, x1] x [y0, y1] (truncated, not clipped) covered by the bounding box of the enlarged RoI's rotated corners
__global__ __launch_bounds__(256) void k_roi_spans(const float* __restrict__ rois, int n_rois_total, int roi_cols, float ex, float ey,
                                                   RpGrid g, int4* __restrict__ spans) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rois_total) return;
  const float* box = rois + (long long)r * roi_cols;
  const float cx = box[0], cy = box[1], hx = (box[3] + ex) / 2, hy = (box[4] + ey) / 2, angle = box[6];
  const float c = cosf(angle), s = sinf(angle);
  const float qx[4] = {cx - hx, cx + hx, cx + hx, cx - hx};
  const float qy[4] = {cy - hy, cy - hy, cy + hy, cy + hy};
  float ax0 = 0.f, ay0 = 0.f, ax1 = 0.f, ay1 = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float nx = (qx[k] - cx) * c + (qy[k] - cy) * (-s) + cx;
    const float ny = (qx[k] - cx) * s + (qy[k] - cy) * c + cy;
    if (k == 0) {
      ax0 = ax1 = nx;
      ay0 = ay1 = ny;
    } else {
      ax0 = fminf(ax0, nx);
      ay0 = fminf(ay0, ny);
      ax1 = fmaxf(ax1, nx);
      ay1 = fmaxf(ay1, ny);
    }
  }
  // float -> int truncates towards zero; values beyond the grid saturate and are clipped by the walk
  const float lim = 1.0e6f;
  int4 sp;
  sp.x = (int)fminf(fmaxf(ax0 - g.lo_x, -lim), lim);
  sp.y = (int)fminf(fmaxf(ay0 - g.lo_y, -lim), lim);
  sp.z = (int)fminf(fmaxf(ax1 - g.lo_x, -lim), lim);
  sp.w = (int)fminf(fmaxf(ay1 - g.lo_y, -lim), lim);
  spans[r] = sp;
}

struct RpBox {
  float cx, cy, cz, dx, dy, dz, cosa, sina;      // enlarged sizes, rotation by -heading
  double res;
  int out_x, out_y, out_z;
};

__device__ __forceinline__ unsigned rp_hash(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 29;
  return (unsigned)k;
}

// one pass over the RoI's points with row < limit: distinct voxels -> (s_key, s_row = lowest row), count in *s_cnt, *s_over set when
// the table refused a point
__device__ __forceinline__ void rp_walk(const float* __restrict__ points, int cols, const int* __restrict__ cell_start,
                                        const int* __restrict__ csr, const int4* __restrict__ spans_b, int r, int b, const RpGrid& g,
                                        const RpBox& B, int boxes_per_patch, int limit, unsigned long long* s_key, int* s_row, int* s_cnt,
                                        int* s_over) {
  const int lane = threadIdx.x & (GD_WAVE - 1), wave = threadIdx.x / GD_WAVE;
  const int4 sp = spans_b[r];
  const int x0 = max(sp.x, 0), x1 = min(sp.z, g.X - 1), y0 = max(sp.y, 0), y1 = min(sp.w, g.Y - 1);
  if (x1 < x0 || y1 < y0) return;
  const int nx = x1 - x0 + 1;
  const long long np = (long long)nx * (y1 - y0 + 1);
  for (long long p = wave; p < np; p += RP_WAVES) {
    const int px = x0 + (int)(p % nx), py = y0 + (int)(p / nx);
    const int cell = (b * g.Y + py) * g.X + px;
    const int beg = cell_start[cell], end = cell_start[cell + 1];
    if (beg == end) continue;                                   // (wave-uniform)
    // position of this RoI in the patch's RoI list: the RoIs below it whose span covers the patch
    int rank = 0;
    for (int q0 = 0; q0 < r; q0 += GD_WAVE) {
      const int q = q0 + lane;
      bool cov = false;
      if (q < r) {
        const int4 s = spans_b[q];
        cov = s.x <= px && px <= s.z && s.y <= py && py <= s.w;
      }
      rank += __popcll(__ballot(cov));
    }
    if (rank >= boxes_per_patch) continue;
    for (int i = beg + lane; i < end; i += GD_WAVE) {
      const int row = csr[i];
      if (row >= limit) continue;
      const float* pt = points + (long long)row * cols;
      const float x = pt[1], y = pt[2], z = pt[3];
      if (fabsf(z - B.cz) > B.dz / 2.0f) continue;
      const float sx = x - B.cx, sy = y - B.cy;
      const float lx = sx * B.cosa + sy * (-B.sina);
      const float ly = sx * B.sina + sy * B.cosa;
      const double margin = (double)1e-5f;
      if (!((double)fabsf(lx) < (double)B.dx / 2.0 + margin && (double)fabsf(ly) < (double)B.dy / 2.0 + margin)) continue;
      const float lz = z - B.cz;
      int xi = (int)((double)(lx + B.dx / 2) / B.res);
      int yi = (int)((double)(ly + B.dy / 2) / B.res);
      int zi = (int)((double)(lz + B.dz / 2) / B.res);
      xi = min(max(xi, 0), B.out_x - 1);
      yi = min(max(yi, 0), B.out_y - 1);
      zi = min(max(zi, 0), B.out_z - 1);
      const unsigned long long key = ((unsigned long long)(xi & 0x1FFFFF) << 42) | ((unsigned long long)(yi & 0x1FFFFF) << 21) |
                                     (unsigned long long)(zi & 0x1FFFFF);
      if (*(volatile int*)s_cnt >= RP_FILL) {
        *s_over = 1;
        continue;
      }
      unsigned slot = rp_hash(key) & (RP_SLOTS - 1);
      while (true) {
        const unsigned long long prev = atomicCAS(s_key + slot, RP_EMPTY, key);
        if (prev == RP_EMPTY) atomicAdd(s_cnt, 1);
        if (prev == RP_EMPTY || prev == key) {
          atomicMin(s_row + slot, row);
          break;
        }
        slot = (slot + 1) & (RP_SLOTS - 1);
      }
    }
  }
}

__global__ __launch_bounds__(RP_BLOCK) void k_roi_pool(const float* __restrict__ points, long long n_points, int cols,
                                                       const float* __restrict__ rois, int n_rois, int roi_cols, RpGrid g, float ex,
                                                       float ey, float ez, int num_dvs, int num_fps, float lambda, float delta,
                                                       int boxes_per_patch, const int* __restrict__ cell_start,
                                                       const int* __restrict__ csr, const int4* __restrict__ spans,
                                                       int* __restrict__ pooled_idx, int* __restrict__ pooled_num,
                                                       float* __restrict__ feats_local, float* __restrict__ xyz_global) {
  __shared__ unsigned long long s_key[RP_SLOTS];      // table keys; afterwards: candidate rows [0, 4096) and FPS slots [4096, 8192) as int
  __shared__ int s_row[RP_SLOTS];                     // table rows; afterwards: candidate x, y, z (3 x RP_MAX_DVS floats)
  __shared__ int s_cnt, s_over, s_n;
  __shared__ float s_bv[2][RP_WAVES];
  __shared__ int s_bi[2][RP_WAVES];
  const int tid = threadIdx.x, lane = tid & (GD_WAVE - 1), wave = tid / GD_WAVE;
  const int br = blockIdx.x, b = br / n_rois, r = br % n_rois;
  const float* roi = rois + (long long)br * roi_cols;
  RpBox B;
  B.cx = roi[0];
  B.cy = roi[1];
  B.cz = roi[2];
  B.dx = roi[3] + ex;
  B.dy = roi[4] + ey;
  B.dz = roi[5] + ez;
  const float heading = roi[6];
  B.cosa = cosf(-heading);
  B.sina = sinf(-heading);
  {
    const float v = lambda * expf(-sqrtf(B.cx * B.cx + B.cy * B.cy + B.cz * B.cz) / delta);
    B.res = fmax(0.02, (double)v);
    B.out_x = (int)((double)B.dx / B.res);
    B.out_y = (int)((double)B.dy / B.res);
    B.out_z = (int)((double)B.dz / B.res);
  }
  const int4* spans_b = spans + (long long)b * n_rois;

  // ---- distinct voxels of the in-box points (lowest row each); bisection on a row limit when the table overflows
  int lo = 0, hi = (int)n_points, limit = (int)n_points;
  while (true) {
    for (int i = tid; i < RP_SLOTS; i += RP_BLOCK) {
      s_key[i] = RP_EMPTY;
      s_row[i] = INT_MAX;
    }
    if (tid == 0) {
      s_cnt = 0;
      s_over = 0;
      s_n = 0;
    }
    __syncthreads();
    rp_walk(points, cols, cell_start, csr, spans_b, r, b, g, B, boxes_per_patch, limit, s_key, s_row, &s_cnt, &s_over);
    __syncthreads();
    const int cnt = s_cnt, over = s_over;
    __syncthreads();
    if (!over) {
      if (limit == (int)n_points || cnt >= num_dvs) break;
      lo = limit;
    } else {
      hi = limit;
    }
    limit = lo + (hi - lo) / 2;
  }

  // ---- candidate rows, ascending
  int* cand = (int*)s_key;
  int* slots = cand + RP_SLOTS;
  {
    int mine[RP_SLOTS / RP_BLOCK];
#pragma unroll
    for (int k = 0; k < RP_SLOTS / RP_BLOCK; ++k) mine[k] = s_row[k * RP_BLOCK + tid];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RP_SLOTS / RP_BLOCK; ++k)
      if (mine[k] != INT_MAX) cand[atomicAdd(&s_n, 1)] = mine[k];
    __syncthreads();
  }
  const int cnt = s_n;
  int P = 1;
  while (P < cnt) P <<= 1;
  for (int i = cnt + tid; i < P; i += RP_BLOCK) cand[i] = INT_MAX;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += RP_BLOCK) {
        const int o = i ^ j;
        if (o > i) {
          const int a = cand[i], c = cand[o];
          if ((a > c) == ((i & k) == 0)) {
            cand[i] = c;
            cand[o] = a;
          }
        }
      }
      __syncthreads();
    }
  const int num = min(cnt, num_dvs);
  if (tid == 0) pooled_num[br] = num;

  // ---- farthest-point sampling over the num lowest rows
  float* cx_ = (float*)s_row;
  float* cy_ = cx_ + RP_MAX_DVS;
  float* cz_ = cy_ + RP_MAX_DVS;
  for (int i = tid; i < num; i += RP_BLOCK) {
    const float* pt = points + (long long)cand[i] * cols;
    cx_[i] = pt[1];
    cy_[i] = pt[2];
    cz_[i] = pt[3];
  }
  if (tid == 0) slots[0] = 0;
  __syncthreads();
  constexpr int PER = RP_MAX_DVS / RP_BLOCK;
  float mind[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) mind[j] = INFINITY;
  const int rounds = min(num_fps, num);
  int cur = 0;
  for (int s = 1; s < rounds; ++s) {
    const float x1 = cx_[cur], y1 = cy_[cur], z1 = cz_[cur];
    float best = -1.f;
    int besti = INT_MAX;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = j * RP_BLOCK + tid;
      if (i < num) {
        const float ddx = cx_[i] - x1, ddy = cy_[i] - y1, ddz = cz_[i] - z1;
        const float d = (ddx * ddx + ddy * ddy) + ddz * ddz;
        if (d < mind[j]) mind[j] = d;
        if (mind[j] > best) {
          best = mind[j];
          besti = i;
        }
      }
    }
#pragma unroll
    for (int off = GD_WAVE / 2; off > 0; off >>= 1) {
      const float ov = __shfl_xor(best, off, GD_WAVE);
      const int oi = __shfl_xor(besti, off, GD_WAVE);
      if (ov > best || (ov == best && oi < besti)) {
        best = ov;
        besti = oi;
      }
    }
    const int par = s & 1;
    if (lane == 0) {
      s_bv[par][wave] = best;
      s_bi[par][wave] = besti;
    }
    __syncthreads();
    best = s_bv[par][0];
    besti = s_bi[par][0];
#pragma unroll
    for (int w = 1; w < RP_WAVES; ++w) {
      const float ov = s_bv[par][w];
      const int oi = s_bi[par][w];
      if (ov > best || (ov == best && oi < besti)) {
        best = ov;
        besti = oi;
      }
    }
    cur = besti < num ? besti : 0;
    if (tid == 0) slots[s] = cur;
  }
  __syncthreads();

  // ---- outputs: slot s >= num repeats slot s % num; an empty RoI gives zero rows
  const int C = cols - 4, F = 3 + C + 6;
  const float hx = roi[3] / 2, hy = roi[4] / 2, hz = roi[5] / 2;
  for (int s = tid; s < num_fps; s += RP_BLOCK) {
    const long long o = (long long)br * num_fps + s;
    float* f = feats_local + o * F;
    float* gx = xyz_global + o * 3;
    if (num == 0) {
      pooled_idx[o] = 0;
      for (int k = 0; k < F; ++k) f[k] = 0.f;
      gx[0] = gx[1] = gx[2] = 0.f;
      continue;
    }
    const int c = slots[s < num ? s : s % num];
    const int row = cand[c];
    const float* pt = points + (long long)row * cols;
    const float x = pt[1], y = pt[2], z = pt[3];
    pooled_idx[o] = row;
    gx[0] = x;
    gx[1] = y;
    gx[2] = z;
    const float sx = x - B.cx, sy = y - B.cy;
    f[0] = sx * B.cosa + sy * (-B.sina);
    f[1] = sx * B.sina + sy * B.cosa;
    f[2] = z - B.cz;
    for (int k = 0; k < C; ++k) f[3 + k] = pt[4 + k];
    f[3 + C + 0] = -hx;
    f[3 + C + 1] = -hy;
    f[3 + C + 2] = -hz;
    f[3 + C + 3] = hx;
    f[3 + C + 4] = hy;
    f[3 + C + 5] = hz;
  }
}

struct RpLayout {
  int X, Y;
  long long cells;
  size_t off_count, off_start, off_cursor, off_pcell, off_csr, off_spans, off_scan, total;
};

RpGrid rp_grid(const float* range_xy, const float* patch_lo, int X, int Y) {
  RpGrid g;
  g.x0 = range_xy[0];
  g.y0 = range_xy[1];
  g.x1 = range_xy[2];
  g.y1 = range_xy[3];
  g.lo_x = patch_lo[0];
  g.lo_y = patch_lo[1];
  g.X = X;
  g.Y = Y;
  return g;
}

RpLayout rp_layout(long long n_points, int batch, int n_rois, int X, int Y) {
  RpLayout L;
  L.X = X;
  L.Y = Y;
  L.cells = (long long)batch * X * Y;
  const size_t np = (size_t)(n_points > 0 ? n_points : 1);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += gd_align(bytes);
    return o;
  };
  L.off_count = take((size_t)(L.cells + 1) * 4);
  L.off_start = take((size_t)(L.cells + 1) * 4);
  L.off_cursor = take((size_t)(L.cells + 1) * 4);
  L.off_pcell = take(np * 4);
  L.off_csr = take(np * 4);
  L.off_spans = take((size_t)(batch > 0 ? batch : 1) * (n_rois > 0 ? n_rois : 1) * sizeof(int4));
  L.off_scan = take(gd_scan_ws_elems(L.cells + 1) * 4);
  L.total = off;
  return L;
}

}  // namespace

extern "C" size_t gdmae_roi_dfvs_pool_workspace_bytes(long long n_points, int batch, int n_rois, int patches_x, int patches_y) {
  if (patches_x <= 0 || patches_y <= 0 || batch <= 0) return 256;
  return rp_layout(n_points, batch, n_rois, patches_x, patches_y).total;
}

extern "C" int gdmae_roi_dfvs_pool(const float* points, long long n_points, int n_cols, const float* rois, int batch, int n_rois,
                                   int roi_cols, const float* range_xy, const float* patch_lo, int patches_x, int patches_y,
                                   const float* extra_width, int num_dvs_points, int num_fps_points,
                                   int hash_size, float lambda, float delta, int boxes_per_patch, int phases, int* pooled_idx,
                                   int* pooled_num, float* feats_local, float* xyz_global, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  (void)hash_size;      // the reference's probe table size: the voxel table here lives in LDS and drops nothing
  hipStream_t st = (hipStream_t)stream;
  GD_REQUIRE(n_cols >= 4 && roi_cols >= 7, "roi_dfvs_pool: points need [b, x, y, z, ...] columns, rois 7");
  GD_REQUIRE(n_points >= 0 && n_points < (1ll << 31) / n_cols, "roi_dfvs_pool: point count");
  GD_REQUIRE(num_dvs_points >= 1 && num_dvs_points <= RP_MAX_DVS, "roi_dfvs_pool: NUM_DVS_POINTS must be in [1, 1024]");
  GD_REQUIRE(num_fps_points >= 1 && num_fps_points <= RP_MAX_FPS, "roi_dfvs_pool: NUM_FPS_POINTS must be in [1, 4096]");
  GD_REQUIRE(boxes_per_patch >= 1, "roi_dfvs_pool: NUM_BOXES_PER_PATCH");
  GD_REQUIRE(phases >= 1 && phases <= 3, "roi_dfvs_pool: phases is a mask of 1 (patch CSR) and 2 (pooling)");
  if (batch <= 0 || n_rois <= 0) return 0;
  GD_REQUIRE(patches_x > 0 && patches_y > 0 && (long long)batch * patches_x * patches_y < (1ll << 30), "roi_dfvs_pool: patch grid");
  const RpGrid g = rp_grid(range_xy, patch_lo, patches_x, patches_y);
  const RpLayout L = rp_layout(n_points, batch, n_rois, patches_x, patches_y);
  GD_REQUIRE(workspace_bytes >= L.total, "roi_dfvs_pool: workspace too small");
  char* ws = (char*)workspace;
  int* count = (int*)(ws + L.off_count);
  int* start = (int*)(ws + L.off_start);
  int* cursor = (int*)(ws + L.off_cursor);
  int* pcell = (int*)(ws + L.off_pcell);
  int* csr = (int*)(ws + L.off_csr);
  int4* spans = (int4*)(ws + L.off_spans);
  int* scan_ws = (int*)(ws + L.off_scan);
  if (phases & 1) {
    GD_CHECK(hipMemsetAsync(count, 0, (size_t)(L.cells + 1) * 4, st));
    if (n_points > 0) {
      hipLaunchKernelGGL(k_point_cells, dim3(gd_div_up(n_points, 256)), dim3(256), 0, st, points, n_points, n_cols, batch, g, pcell,
                         count);
      GD_LAUNCH_CHECK();
    }
    // cells + 1 entries: the last one (count 0) receives the total, so that start[cell + 1] closes every cell
    if (int rc = gd_device_scan<int>(L.cells + 1, RpLoad{count}, RpStore{start, cursor}, (int*)nullptr, scan_ws, st)) return rc;
    if (n_points > 0) {
      hipLaunchKernelGGL(k_fill_cells, dim3(gd_div_up(n_points, 256)), dim3(256), 0, st, pcell, n_points, cursor, csr);
      GD_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_roi_spans, dim3(gd_div_up((long long)batch * n_rois, 256)), dim3(256), 0, st, rois, batch * n_rois, roi_cols,
                       extra_width[0], extra_width[1], g, spans);
    GD_LAUNCH_CHECK();
  }
  if (phases & 2) {
    hipLaunchKernelGGL(k_roi_pool, dim3(batch * n_rois), dim3(RP_BLOCK), 0, st, points, n_points, n_cols, rois, n_rois, roi_cols, g,
                       extra_width[0], extra_width[1], extra_width[2], num_dvs_points, num_fps_points, lambda, delta, boxes_per_patch,
                       (const int*)start, (const int*)csr, (const int4*)spans, pooled_idx, pooled_num, feats_local, xyz_global);
    GD_LAUNCH_CHECK();
  }
  return 0;
}
