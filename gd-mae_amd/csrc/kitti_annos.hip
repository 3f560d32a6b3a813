// KITTI annos of the padded detections of F frames in one launch (reference KittiDataset.generate_prediction_dicts with
// box_utils.boxes3d_lidar_to_kitti_camera, boxes3d_kitti_camera_to_imageboxes and Calibration.lidar_to_rect / rect_to_img).
//   k_kitti_annos    a workgroup of 64 threads per (frame, 64 rows), one thread per row: the lidar box goes to rectified camera
//                    coordinates through V2C and R0, its eight corners through P2 (divided by the corner's rect z, as the reference
//                    divides) to the clipped image box; alpha, the copied score / lidar box / label and the clean_data flags of every
//                    (evaluated class, difficulty).  fp32 inputs, fp64 arithmetic in the order of evaluation.kitti_annos_numpy, every
//                    result rounded once to fp32; the flags are decided on the ROUNDED image box with an fp32 subtraction, which is
//                    what kitti_clean_data decides on fp32 annos.  A workgroup never spans two frames, so the 36 calibration floats
//                    are wave-uniform.  Rows at or beyond num[f] write nothing; a row writes at dt_off[f] + row (compact).
// No atomics, no workspace, no host synchronisation.
#include "common.h"

namespace {
constexpr int kKaMaxRows = 1024;      // detections per frame: the cap of csrc/kitti_eval.hip
constexpr int kKaMaxNames = 16;       // entries of the label -> KITTI class map
constexpr int kKaMaxClasses = 6;      // evaluated classes
constexpr int kKaCalib = 36;          // P2 (12), R0 (9), V2C (12), image height, image width, one pad

struct KaArgs {
  const float* boxes;
  int box_stride;
  const float* scores;
  const long long* labels;
  const int* num;
  const float* calib;
  const int* dt_off;
  int F, rows, ND, n_names, n_classes;
  int class_map[kKaMaxNames];         // 1-based label - 1 -> KITTI class int, -1: a name that is no KITTI class
  int classes[kKaMaxClasses];
  float *bbox, *geo, *alpha, *score, *boxes_lidar;
  signed char* ignored;
  int* label;
};

// min / max that hand a NaN on, as numpy's min, max and clip do in the statement (fmin / fmax would drop it: a corner with 0 / 0)
__device__ inline double ka_min(double a, double b) { return a != a ? a : (b < a || b != b ? b : a); }
__device__ inline double ka_max(double a, double b) { return a != a ? a : (b > a || b != b ? b : a); }

__global__ __launch_bounds__(GD_WAVE) void k_kitti_annos(KaArgs A, int blocks_per_frame) {
  const int f = blockIdx.x / blocks_per_frame, row = (blockIdx.x - f * blocks_per_frame) * GD_WAVE + threadIdx.x;
  const int o0 = A.dt_off[f];
  const int n = min(min(A.num[f], A.dt_off[f + 1] - o0), A.rows);
  if (row >= n || o0 < 0 || o0 + row >= A.ND) return;
  const size_t o = (size_t)o0 + row, in = (size_t)f * A.rows + row;
  const float* b = A.boxes + in * A.box_stride;
  const float* cal = A.calib + (size_t)f * kKaCalib;
  const float *P = cal, *R = cal + 12, *V = cal + 21;
  const double x = b[0], y = b[1], z = b[2], l = b[3], w = b[4], h = b[5], heading = b[6];
  const double zb = z - h / 2.0;
  double cam[3], loc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) cam[i] = (double)V[i * 4 + 0] * x + (double)V[i * 4 + 1] * y + (double)V[i * 4 + 2] * zb + (double)V[i * 4 + 3];
#pragma unroll
  for (int i = 0; i < 3; ++i) loc[i] = (double)R[i * 3 + 0] * cam[0] + (double)R[i * 3 + 1] * cam[1] + (double)R[i * 3 + 2] * cam[2];
  const double ry = -heading - 3.14159265358979323846 / 2.0;
  const double c = cos(ry), s = sin(ry);
  double u0 = INFINITY, v0 = INFINITY, u1 = -INFINITY, v1 = -INFINITY;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    // the reference's corner order: x = l/2 (+ + - - + + - -), z = w/2 (+ - - + + - - +), y = 0 (corners 0 .. 3) / -h (4 .. 7)
    const double xc = ((k & 3) < 2 ? l : -l) / 2.0, zc = ((k & 3) == 0 || (k & 3) == 3 ? w : -w) / 2.0, yc = k < 4 ? 0.0 : -h;
    const double X = loc[0] + (xc * c + zc * s), Y = loc[1] + yc, Z = loc[2] + (-xc * s + zc * c);
    const double u = ((double)P[0] * X + (double)P[1] * Y + (double)P[2] * Z + (double)P[3]) / Z;
    const double v = ((double)P[4] * X + (double)P[5] * Y + (double)P[6] * Z + (double)P[7]) / Z;
    u0 = ka_min(u0, u); u1 = ka_max(u1, u); v0 = ka_min(v0, v); v1 = ka_max(v1, v);
  }
  const double xmax = (double)cal[34] - 1.0, ymax = (double)cal[33] - 1.0;
  float bb[4];
  bb[0] = (float)ka_min(ka_max(u0, 0.0), xmax);
  bb[1] = (float)ka_min(ka_max(v0, 0.0), ymax);
  bb[2] = (float)ka_min(ka_max(u1, 0.0), xmax);
  bb[3] = (float)ka_min(ka_max(v1, 0.0), ymax);
#pragma unroll
  for (int i = 0; i < 4; ++i) A.bbox[o * 4 + i] = bb[i];
  float* g = A.geo + o * 7;
  g[0] = (float)loc[0]; g[1] = (float)loc[1]; g[2] = (float)loc[2];
  g[3] = b[3]; g[4] = b[5]; g[5] = b[4];                       // dimensions = (dx, dz, dy): the reference's l, h, w
  g[6] = (float)ry;
  A.alpha[o] = (float)(-atan2(-y, x) + ry);
  A.score[o] = A.scores[in];
#pragma unroll
  for (int i = 0; i < 7; ++i) A.boxes_lidar[o * 7 + i] = b[i];
  const long long lab = A.labels[in];
  A.label[o] = (int)lab;
  int own = -1;                                                // a label outside 1 .. n_names is no class
#pragma unroll
  for (int i = 0; i < kKaMaxNames; ++i)
    if (lab == i + 1 && i < A.n_names) own = A.class_map[i];
  const float height = fabsf(bb[3] - bb[1]);                    // fp32 subtraction of the rounded box: kitti_clean_data on fp32 annos
  for (int ci = 0; ci < A.n_classes; ++ci) {
    const signed char base = own >= 0 && own == A.classes[ci] ? 0 : -1;
    A.ignored[((size_t)ci * 3 + 0) * A.ND + o] = height < 40.f ? 1 : base;
    A.ignored[((size_t)ci * 3 + 1) * A.ND + o] = height < 25.f ? 1 : base;
    A.ignored[((size_t)ci * 3 + 2) * A.ND + o] = height < 25.f ? 1 : base;
  }
}
}  // namespace

extern "C" int gdmae_kitti_annos(const float* boxes, int box_stride, const float* scores, const long long* labels, const int* num,
                                 const float* calib, const int* dt_off, int n_frames, int rows, int n_det, const int* class_map,
                                 int n_names, const int* classes, int n_classes, float* bbox, float* geo, float* alpha, float* score,
                                 signed char* ignored_dt, float* boxes_lidar, int* label, void* stream) {
  GD_REQUIRE(n_frames >= 0, "kitti_annos: negative frame count");
  GD_REQUIRE(rows >= 1 && rows <= kKaMaxRows, "kitti_annos: 1 .. 1024 rows per frame");
  GD_REQUIRE(box_stride >= 7, "kitti_annos: boxes of at least 7 columns");
  GD_REQUIRE(n_det >= 0, "kitti_annos: negative detection count");
  GD_REQUIRE(class_map && n_names >= 1 && n_names <= kKaMaxNames, "kitti_annos: a class map of 1 .. 16 names (host)");
  GD_REQUIRE(classes && n_classes >= 1 && n_classes <= kKaMaxClasses, "kitti_annos: 1 .. 6 evaluated classes (host)");
  GD_REQUIRE((long long)n_frames * gd_div_up(rows, GD_WAVE) <= 0x7fffffffLL, "kitti_annos: too many frames for one launch");
  GD_REQUIRE(boxes && scores && labels && num && calib && dt_off, "kitti_annos: null input pointer");
  GD_REQUIRE(bbox && geo && alpha && score && ignored_dt && boxes_lidar && label, "kitti_annos: null output pointer");
  if (n_frames == 0 || n_det == 0) return 0;                   // nothing to write
  KaArgs A;
  A.boxes = boxes; A.box_stride = box_stride; A.scores = scores; A.labels = labels; A.num = num; A.calib = calib; A.dt_off = dt_off;
  A.F = n_frames; A.rows = rows; A.ND = n_det; A.n_names = n_names; A.n_classes = n_classes;
  for (int i = 0; i < kKaMaxNames; ++i) A.class_map[i] = i < n_names ? class_map[i] : -1;
  for (int i = 0; i < kKaMaxClasses; ++i) A.classes[i] = i < n_classes ? classes[i] : -2;
  A.bbox = bbox; A.geo = geo; A.alpha = alpha; A.score = score; A.boxes_lidar = boxes_lidar; A.ignored = ignored_dt; A.label = label;
  const int bpf = gd_div_up(rows, GD_WAVE);
  hipLaunchKernelGGL(k_kitti_annos, dim3(n_frames * bpf), dim3(GD_WAVE), 0, (hipStream_t)stream, A, bpf);
  GD_LAUNCH_CHECK();
  return 0;
}
