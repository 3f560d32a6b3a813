"""RoI point pooling of the two-stage detector (gdmae_roi_dfvs_pool) at the workload's own shape, per phase.

    python tools/bench_roi_pool.py [--batch 8] [--rois 500] [--repeats 20] [--warmup 3]

8 x ~180 k synthetic points (the config-B cloud generator) and 500 seeded RoIs per sample: vehicle / pedestrian / cyclist sized
boxes centred on points of the cloud, so that they hold points as first-stage proposals do.  Phase 1 builds the patch -> point
lists and the RoI spans, phase 2 pools (one workgroup per RoI); both are timed with device events around ``--repeats`` calls
after ``--warmup`` calls, the median over the repeats is reported.  One JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd")]

from gdmae_hip import configs, synth  # noqa: E402
from pcdet.ops.patch_ops import patch_ops_utils as po  # noqa: E402


def seeded_rois(pts, B, M, seed=9):
    rng = np.random.default_rng(seed)
    size = {0: (4.7, 2.1, 1.7), 1: (0.9, 0.85, 1.75), 2: (1.8, 0.85, 1.75)}
    rois = np.zeros((B, M, 7), np.float32)
    for b in range(B):
        own = pts[pts[:, 0] == b]
        own = own[own[:, 3] > 0.3]                       # off the ground plane: walls and clutter
        c = own[rng.integers(0, own.shape[0], M), 1:4]
        cls = rng.integers(0, 3, M)
        rois[b, :, 0:2] = c[:, 0:2] + rng.normal(0, 0.3, (M, 2))
        rois[b, :, 2] = 0.9
        rois[b, :, 3:6] = np.array([size[int(k)] for k in cls]) * rng.uniform(0.8, 1.25, (M, 3))
        rois[b, :, 6] = rng.uniform(-np.pi, np.pi, M)
    return rois


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rois", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    cfg = configs.graphrcnn_head_cfg().DFVS_CONFIG
    _, ds, skw = configs.named_config("B")
    pts = synth.synth_batch(100, a.batch, ds.point_cloud_range, **skw)
    rois = seeded_rois(pts, a.batch, a.rois)
    points, boxes = torch.from_numpy(pts).cuda(), torch.from_numpy(rois).cuda()
    r = ds.point_cloud_range
    lo, shape = po.patch_grid(r)
    args = (points, boxes, [r[0], r[1], r[3], r[4]], lo, shape, cfg.NUM_DVS_POINTS, cfg.NUM_FPS_POINTS, cfg.HASH_SIZE, cfg.LAMBDA, cfg.DELTA,
            cfg.POOL_EXTRA_WIDTH, cfg.NUM_BOXES_PER_PATCH)

    def timed(phases):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = po.roi_dfvs_pool_hip(*args, phases=phases)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), out
    for _ in range(a.warmup):
        timed(3)
    res = {}
    for name, ph in (("patch_lists_ms", 1), ("pool_ms", 2), ("both_ms", 3)):
        res[name] = round(statistics.median(timed(ph)[0] for _ in range(a.repeats)), 4)
    num = timed(3)[1][1]
    res.update(batch=a.batch, rois_per_sample=a.rois, points=int(pts.shape[0]), pooled_mean=round(float(num.float().mean()), 1),
               pooled_max=int(num.max()), empty_rois=int((num == 0).sum()), full_fps_rois=int((num >= cfg.NUM_FPS_POINTS).sum()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
