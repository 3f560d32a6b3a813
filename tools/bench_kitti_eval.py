"""``evaluation.kitti_eval`` on a synthetic set at KITTI-val scale: 3769 frames, 4 - 12 GT rows and 10 - 50 detections per
frame, the classes Car, Pedestrian, Cyclist (54 combinations).  The whole call is timed - the host's flags, the upload, the five
launches with the sort between them, the one read and the result text - with five runs of device events around calls that end in a
synchronise; the host share (``kitti_clean_data`` and the anno concatenation) is timed by the wall clock next to it.

The reference evaluator needs numba and is not part of this package, so the only comparison here is the package's own numpy
statement ``kitti_eval_numpy`` (pure-Python fp64 clipping) on the first 40 frames, scaled by 3769 / 40 and labelled as such: it is an
estimate of the statement, not a measurement of the reference.

    python tools/bench_kitti_eval.py"""
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd")]
from gdmae_hip import evaluation  # noqa: E402

assert torch.cuda.is_available(), "bench_kitti_eval needs a GPU"
FRAMES, SUBSET = 3769, 40
CLASSES = ['Car', 'Pedestrian', 'Cyclist']
NAMES = np.array(['Car', 'Car', 'Car', 'Pedestrian', 'Pedestrian', 'Cyclist', 'Van', 'DontCare', 'Truck', 'Person_sitting'])
DIMS = {'Car': (3.9, 1.56, 1.6), 'Pedestrian': (0.8, 1.75, 0.6), 'Cyclist': (1.76, 1.73, 0.6), 'Van': (5.0, 2.2, 1.9), 'DontCare': (-1, -1, -1),
        'Truck': (8.0, 3.2, 2.6), 'Person_sitting': (0.8, 1.3, 0.6)}
rng = np.random.RandomState(3)


def rows(names, f):
    n = len(names)
    dims = np.array([DIMS[str(k)] for k in names], np.float64).reshape(n, 3) * rng.uniform(0.9, 1.1, (n, 3))
    x1, y1 = rng.uniform(0, 1100, n), rng.uniform(100, 250, n)
    return dict(name=names, truncated=rng.choice([0.0, 0.0, 0.2, 0.4], n).astype(f), occluded=rng.choice([0, 0, 1, 2, 3], n),
                alpha=rng.uniform(-np.pi, np.pi, n).astype(f), bbox=np.stack([x1, y1, x1 + rng.uniform(30, 140, n), y1 + rng.uniform(15, 90, n)], 1).astype(f),
                dimensions=dims.astype(f), location=np.stack([rng.uniform(-35, 35, n), rng.uniform(1.4, 1.9, n), rng.uniform(5, 70, n)], 1).astype(f),
                rotation_y=rng.uniform(-np.pi, np.pi, n).astype(f))


def frame():
    g = rows(NAMES[rng.randint(0, len(NAMES), rng.randint(4, 13))], np.float64)
    n_dt = int(rng.randint(10, 51))
    g['location'][g['name'] == 'DontCare'] = -1000.0
    real = np.nonzero(g['name'] != 'DontCare')[0]
    near = real[rng.randint(0, len(real), n_dt // 2)] if len(real) else real      # half of the detections jitter a GT row, half are anywhere
    d = rows(np.array(CLASSES)[rng.randint(0, 3, n_dt)], np.float32)
    for k in ('bbox', 'dimensions', 'location', 'rotation_y', 'alpha'):
        d[k][:len(near)] = g[k][near]
    d['name'][:len(near)] = np.where(np.isin(g['name'][near], CLASSES), g['name'][near], 'Car')
    d['bbox'][:len(near)] += rng.normal(0, 4, (len(near), 4)).astype(np.float32)
    d['location'][:len(near)] += rng.normal(0, 0.25, (len(near), 3)).astype(np.float32)
    d['rotation_y'][:len(near)] += rng.normal(0, 0.1, len(near)).astype(np.float32)
    d['score'] = rng.uniform(0.05, 1.0, n_dt).astype(np.float32)
    return g, d


t0 = time.perf_counter()
frames = [frame() for _ in range(FRAMES)]
gt_annos, dt_annos = [f[0] for f in frames], [f[1] for f in frames]
print(f"{FRAMES} frames, {sum(len(a['name']) for a in gt_annos)} GT rows, {sum(len(a['name']) for a in dt_annos)} detections "
      f"(built in {time.perf_counter() - t0:.1f} s)", flush=True)


def run_hip():
    return evaluation.kitti_eval(gt_annos, dt_annos, CLASSES)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


for _ in range(2):
    result, ret = run_hip()
print(result.split("Pedestrian")[0], flush=True)
runs = []
for r in range(5):
    ms, _ = timed(run_hip)
    runs.append(ms)
    print(f"run {r}: kitti_eval {ms:.1f} ms", flush=True)
host = []
for r in range(3):
    t0 = time.perf_counter()
    evaluation.kitti_clean_data(gt_annos, dt_annos, [0, 1, 2])
    evaluation.kitti_geometry(gt_annos, False), evaluation.kitti_geometry(dt_annos, True)
    host.append((time.perf_counter() - t0) * 1e3)
print(f"kitti_eval: median {statistics.median(runs):.1f} ms per call, of which the host's flags and concatenation (wall clock, measured "
      f"apart) {statistics.median(host):.1f} ms; the split over the five launches and the sort was not measured", flush=True)
t0 = time.perf_counter()
evaluation.kitti_eval_numpy(gt_annos[:SUBSET], dt_annos[:SUBSET], CLASSES)
sub = time.perf_counter() - t0
print(f"kitti_eval_numpy (the fp64 statement, pure Python) on the first {SUBSET} frames: {sub:.2f} s; scaled by {FRAMES} / {SUBSET}: "
      f"{sub * FRAMES / SUBSET:.0f} s for the set (an estimate, not a measurement; the reference evaluator was not run)", flush=True)
