"""The KITTI annos of the detections on the device at KITTI-val scale: 3769 frames in batches of 8, 10 - 50 detections per
frame (about 30) in the padded layout of ``detect`` (500 rows), three calibrations, the classes Car, Pedestrian, Cyclist.  Two pairs,
each measured in this process on the same data, alternating, five runs, medians:

  (a) per batch: ``KittiDetections.update`` against ``padded_to_pred_dicts`` + ``kitti_annos_numpy`` per sample (the reference's
      route: one read of the counts, then ``.cpu().numpy()`` sample by sample).  Each run is the loop over all 472 batches, timed by
      the host clock around work that ends in a synchronise, divided by the number of batches;
  (b) ``kitti_eval`` from the record (the one read of the counts and the one ``gdmae_kitti_annos`` launch included: the record's
      cache is dropped before every run) against ``kitti_eval`` from ``to_annos()`` of the same record (the anno list is built
      before the clock starts, as a caller of the reference's evaluator has it).

    python tools/bench_kitti_annos.py"""
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd"), os.path.join(REPO, "tests")]
from gdmae_hip import evaluation  # noqa: E402
from pcdet.models.detectors.detector3d_template import Detector3DTemplate  # noqa: E402
import kitti_annos_reference as ka  # noqa: E402

assert torch.cuda.is_available(), "bench_kitti_annos needs a GPU"
FRAMES, B, ROWS, RUNS = 3769, 8, 500, 5
CLASSES = ['Car', 'Pedestrian', 'Cyclist']
DEV = torch.device("cuda")
rng = np.random.RandomState(5)


def lidar_rows(n):
    """boxes in front of the camera (fp32), labels"""
    labels = rng.randint(1, 4, n).astype(np.int64)
    dims = np.array([ka.DIMS[CLASSES[k - 1]] for k in labels]).reshape(n, 3) * rng.uniform(0.9, 1.1, (n, 3))
    x = rng.uniform(6.0, 70.0, n)
    boxes = np.concatenate([np.stack([x, rng.uniform(-0.5, 0.5, n) * x, rng.uniform(-1.0, -0.5, n)], 1), dims, rng.uniform(-np.pi, np.pi, (n, 1))], 1)
    return boxes.astype(np.float32), labels


t0 = time.perf_counter()
gt_annos, frames = [], []
for f in range(FRAMES):
    ci = f % 3
    gb, gl = lidar_rows(int(rng.randint(4, 13)))
    g = evaluation.kitti_annos_numpy(gb, np.ones(len(gl), np.float32), gl, ka.CALIBS[ci], ka.SHAPES[ci], CLASSES)
    g = {k: g[k] for k in ('name', 'alpha', 'bbox', 'dimensions', 'location', 'rotation_y')}
    g['truncated'], g['occluded'] = rng.choice([0.0, 0.0, 0.2, 0.4], len(gl)), rng.choice([0, 0, 1, 2, 3], len(gl))
    gt_annos.append(g)
    n = int(rng.randint(10, 51))
    db, dl = lidar_rows(n)
    near = rng.randint(0, len(gl), n // 2)                       # half of the detections jitter a GT box, half are anywhere
    db[:len(near)] = gb[near] + rng.normal(0, 0.15, (len(near), 7)).astype(np.float32)
    dl[:len(near)] = gl[near]
    frames.append(dict(boxes=db, scores=rng.uniform(0.05, 1.0, n).astype(np.float32), labels=dl, calib=ci))
batches = []
for s in range(0, FRAMES, B):
    fr = frames[s:s + B]
    boxes, scores, labels = np.zeros((len(fr), ROWS, 7), np.float32), np.zeros((len(fr), ROWS), np.float32), np.zeros((len(fr), ROWS), np.int64)
    for b, d in enumerate(fr):
        k = len(d['scores'])
        boxes[b, :k], scores[b, :k], labels[b, :k] = d['boxes'], d['scores'], d['labels']
    up = lambda a: torch.from_numpy(a).to(DEV)      # noqa: E731
    out = {'pred_boxes': up(boxes), 'pred_scores': up(scores), 'pred_labels': up(labels), 'num': up(np.array([len(d['scores']) for d in fr], np.int32))}
    batches.append((out, ka.batch_dict(fr, first_id=s)))
print(f"{FRAMES} frames in {len(batches)} batches of {B}, {sum(len(a['name']) for a in gt_annos)} GT rows, "
      f"{sum(len(d['scores']) for d in frames)} detections (built in {time.perf_counter() - t0:.1f} s)", flush=True)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def loop_record():
    det = evaluation.KittiDetections(CLASSES, DEV, rows=ROWS)
    for out, bd in batches:
        det.update(out, bd)
    return det


def loop_numpy():
    annos = []
    for out, bd in batches:
        for b, d in enumerate(Detector3DTemplate.padded_to_pred_dicts(out)):
            annos.append(evaluation.kitti_annos_numpy(d['pred_boxes'], d['pred_scores'], d['pred_labels'], bd['calib'][b], bd['image_shape'][b], CLASSES))
    return annos


det = loop_record()                                              # warm-up of both routes and of every launch below
loop_numpy()
annos = det.to_annos()
for _ in range(2):
    first = evaluation.kitti_eval(gt_annos, det, CLASSES)
    second = evaluation.kitti_eval(gt_annos, annos, CLASSES)
assert first[0] == second[0], "the two routes of (b) do not give the same result text"
print(first[0].split("Pedestrian")[0], flush=True)

a_rec, a_np, b_rec, b_annos, fin = [], [], [], [], []
for r in range(RUNS):
    ms, det = wall(loop_record)
    a_rec.append(ms / len(batches))
    ms, _ = wall(loop_numpy)
    a_np.append(ms / len(batches))
    ms, _ = wall(det.finish)
    fin.append(ms)
    annos = det.to_annos()
    det._invalidate()
    ms, _ = wall(lambda: evaluation.kitti_eval(gt_annos, det, CLASSES))
    b_rec.append(ms)
    ms, _ = wall(lambda: evaluation.kitti_eval(gt_annos, annos, CLASSES))
    b_annos.append(ms)
    print(f"run {r}: (a) update {a_rec[-1] * 1e3:.0f} us / batch, per-sample numpy route {a_np[-1] * 1e3:.0f} us / batch; finish {fin[-1]:.2f} ms; "
          f"(b) kitti_eval from the record {b_rec[-1]:.1f} ms, from to_annos() {b_annos[-1]:.1f} ms", flush=True)
med = statistics.median
print(f"(a) per batch of {B}: KittiDetections.update median {med(a_rec) * 1e3:.0f} us (min {min(a_rec) * 1e3:.0f}, max {max(a_rec) * 1e3:.0f}); "
      f"padded_to_pred_dicts + kitti_annos_numpy per sample median {med(a_np) * 1e3:.0f} us (min {min(a_np) * 1e3:.0f}, max {max(a_np) * 1e3:.0f})")
print(f"    finish (one read of {FRAMES} counts, one launch) median {med(fin):.2f} ms")
print(f"(b) kitti_eval from the record median {med(b_rec):.1f} ms (min {min(b_rec):.1f}, max {max(b_rec):.1f}); from to_annos() median "
      f"{med(b_annos):.1f} ms (min {min(b_annos):.1f}, max {max(b_annos):.1f})")
