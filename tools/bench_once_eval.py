"""``evaluation.once_eval`` on a synthetic set at ONCE-val scale: 3321 frames, 10 - 40 GT rows and 100 - 500 predictions per
frame, the five class names (Vehicle / Pedestrian / Cyclist under the superclass rule, 4 distance bands: 12 combinations).  The
whole call is timed - the name codes, the concatenation and upload, the five launches with the sort between them, the one read and
the table text - with five runs of device events around calls that end in a synchronise; the host share (names to codes and the
concatenation of the annos) is timed by the wall clock next to it.

No time is targeted: the reference evaluator needs numba with a CUDA target and is not part of this package.  The only comparison is
the package's own numpy statement ``once_eval_numpy`` (pure-Python fp64 clipping) on the first 40 frames, scaled by 3321 / 40 and
labelled as such: it is an estimate of the statement, not a measurement of the reference.

    python tools/bench_once_eval.py"""
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd")]
from gdmae_hip import evaluation  # noqa: E402

assert torch.cuda.is_available(), "bench_once_eval needs a GPU"
FRAMES, SUBSET = 3321, 40
CLASSES = ['Car', 'Bus', 'Truck', 'Pedestrian', 'Cyclist']
NAMES = np.array(['Car', 'Car', 'Car', 'Car', 'Bus', 'Truck', 'Pedestrian', 'Pedestrian', 'Cyclist', 'Cyclist'])
DIMS = {'Car': (4.4, 1.9, 1.6), 'Bus': (11.0, 2.9, 3.2), 'Truck': (7.5, 2.6, 3.0), 'Pedestrian': (0.8, 0.7, 1.7), 'Cyclist': (1.9, 0.8, 1.6)}
rng = np.random.RandomState(3)


def rows(names, f):
    n = len(names)
    dims = np.array([DIMS[str(k)] for k in names], np.float64).reshape(n, 3) * rng.uniform(0.9, 1.1, (n, 3))
    r, phi = rng.uniform(3, 75, n), rng.uniform(-np.pi, np.pi, n)
    return dict(name=names, boxes_3d=np.concatenate([np.stack([r * np.cos(phi), r * np.sin(phi), rng.uniform(-1.2, -0.4, n)], 1), dims,
                                                     rng.uniform(-np.pi, np.pi, (n, 1))], 1).astype(f))


def frame():
    g = rows(NAMES[rng.randint(0, len(NAMES), rng.randint(10, 41))], np.float64)
    n_pred = int(rng.randint(100, 501))
    near = rng.randint(0, len(g['name']), min(n_pred // 4, 60))          # some predictions jitter a GT row, the others are anywhere
    p = rows(NAMES[rng.randint(0, len(NAMES), n_pred)], np.float32)
    p['boxes_3d'][:len(near)] = g['boxes_3d'][near]
    p['name'][:len(near)] = g['name'][near]
    p['boxes_3d'][:len(near), :3] += rng.normal(0, 0.15, (len(near), 3)).astype(np.float32)
    p['boxes_3d'][:len(near), 6] += rng.normal(0, 0.05, len(near)).astype(np.float32)
    p['score'] = rng.uniform(0.1, 1.0, n_pred).astype(np.float32)
    return g, p


t0 = time.perf_counter()
frames = [frame() for _ in range(FRAMES)]
gt_annos, pred_annos = [f[0] for f in frames], [f[1] for f in frames]
print(f"{FRAMES} frames, {sum(len(a['name']) for a in gt_annos)} GT rows, {sum(len(a['name']) for a in pred_annos)} predictions "
      f"(built in {time.perf_counter() - t0:.1f} s)", flush=True)


def run_hip():
    return evaluation.once_eval(gt_annos, pred_annos, CLASSES)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


for _ in range(2):
    ret_str, ret = run_hip()
print(ret_str, flush=True)
runs = []
for r in range(5):
    ms, _ = timed(run_hip)
    runs.append(ms)
    print(f"run {r}: once_eval {ms:.1f} ms", flush=True)
host = []
for r in range(3):
    t0 = time.perf_counter()
    names, _ = evaluation.once_name_codes(evaluation.once_classes(CLASSES, True), True)
    for annos in (gt_annos, pred_annos):
        evaluation.once_codes_of([evaluation._once_names(a) for a in annos], names), evaluation.once_boxes(annos)
    evaluation._cat([a['score'] for a in pred_annos], None, np.float32)
    host.append((time.perf_counter() - t0) * 1e3)
print(f"once_eval: median {statistics.median(runs):.1f} ms per call, of which the host's name codes and concatenation (wall clock, "
      f"measured apart) {statistics.median(host):.1f} ms; the split over the five launches and the sort was not measured", flush=True)
t0 = time.perf_counter()
evaluation.once_eval_numpy(gt_annos[:SUBSET], pred_annos[:SUBSET], CLASSES)
sub = time.perf_counter() - t0
print(f"once_eval_numpy (the fp64 statement, pure Python) on the first {SUBSET} frames: {sub:.2f} s; scaled by {FRAMES} / {SUBSET}: "
      f"{sub * FRAMES / SUBSET:.0f} s for the set (an estimate, not a measurement; the reference evaluator was not run)", flush=True)
