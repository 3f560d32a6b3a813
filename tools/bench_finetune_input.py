"""Fine-tune input pipeline measurement: GpuFinetuneInputPipeline on 8 synthetic Waymo-shape frames (gdmae_hip/synth.py
clouds, about 40 seeded GT boxes each, a synthetic GT database) - device time of the whole call and of its two launches, the device
time of gdmae_augment_collate on the same frames (the floor: it moves the same bytes), and the numpy statement's CPU time per
batch.  Device events, median of 20 calls after 3 warm-up calls.  Prints one JSON line.  There is no gate on the numbers.

    python tools/bench_finetune_input.py [--list gd_mae|iou|ts]

--list: the augmentor list of waymo_models/gd_mae.yaml (default), gd_mae_iou.yaml (+ random_world_drop) or gd_mae_ts.yaml
(+ random_world_translation and random_world_drop), built by input_pipeline.finetune_input_pipeline.  With iou and ts every frame of the
batch drops (q = 0.9) and, with ts, is translated: the most work the list can ask for; the drop plan's launches are timed on their own."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd"), os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import finetune_input_aug_reference as far  # noqa: E402
import finetune_input_reference as fr  # noqa: E402
from gdmae_hip import configs  # noqa: E402
from gdmae_hip import input_pipeline as ip  # noqa: E402
from gdmae_hip import lib as L  # noqa: E402
from gdmae_hip import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--list", choices=["gd_mae", "iou", "ts"], default="gd_mae")
LIST = ap.parse_args().list
AUG = {"gd_mae": lambda: list(ip.FINETUNE_AUG_CONFIG), "iou": lambda: configs.waymo_iou_finetune_data_cfg()[0],
       "ts": lambda: configs.waymo_two_stage_data_cfg()[0]}[LIST]()
B, F, WARM, REPS = 8, 5, 3, 20
CLASS_NAMES = ["Vehicle", "Pedestrian", "Cyclist"]
SIZES = {"Vehicle": (4.6, 2.0, 1.7), "Pedestrian": (0.9, 0.8, 1.75), "Cyclist": (1.8, 0.8, 1.7), "Sign": (0.4, 0.4, 2.0)}
rng = np.array([-74.88, -74.88, -2, 74.88, 74.88, 4.0], np.float32)
g = np.random.default_rng(0)


def rand_boxes(names):
    n = len(names)
    size = np.array([SIZES[k] for k in names]).reshape(n, 3) * g.uniform(0.85, 1.15, (n, 3))
    return np.concatenate([g.uniform(-70, 70, (n, 2)), g.uniform(0.0, 1.0, (n, 1)), size, g.uniform(-np.pi, np.pi, (n, 1))], 1).astype(np.float32)


frames = [synth.synth_frame(100 + b, rng, features=F) for b in range(B)]
gt_names, gt_boxes = [], []
for b in range(B):
    nv, npd, nc = int(g.integers(4, 20)), int(g.integers(2, 16)), int(g.integers(0, 4))
    names = ["Vehicle"] * nv + ["Pedestrian"] * npd + ["Cyclist"] * nc + ["Sign"] * max(40 - nv - npd - nc, 0)
    gt_names.append(names)
    gt_boxes.append(rand_boxes(names))
db_names = ["Vehicle"] * 300 + ["Pedestrian"] * 200 + ["Cyclist"] * 100
db_boxes = rand_boxes(db_names)
counts = np.where(np.asarray(db_names) == "Vehicle", g.integers(50, 800, len(db_names)), g.integers(20, 200, len(db_names)))
off = np.concatenate([[0], np.cumsum(counts)])
db_pts = np.concatenate([np.concatenate([g.uniform(-0.5, 0.5, (c, 3)) * bx[3:6], g.uniform(0, 1, (c, 2))], 1) for c, bx in zip(counts, db_boxes)]).astype(np.float32)
db = ip.GtDatabase(db_pts, np.stack([off[:-1], off[1:]], 1), db_boxes, db_names, counts, np.zeros(len(db_names)))

pipe = ip.finetune_input_pipeline(rng, CLASS_NAMES, AUG, db)
pipe.time_kernels = True
np.random.seed(0)
state = ip.sampler_state(pipe.sampler_cfg, pipe.database, CLASS_NAMES)
candidates = [ip.draw_candidates(state, n) for n in gt_names]
params = [ip.draw_world_params(ip.SSL_AUG_CONFIG) for _ in range(B)]
if LIST != "gd_mae":
    params = [dict(p, drop_q=1 - 0.1, drop_seed=int(g.integers(0, 2 ** 63))) for p in params]
if LIST == "ts":
    params = [dict(p, translate=g.normal(0, 0.2, 3)) for p in params]


SPREAD = {}


def median_ms(fn, per_call=None):
    """Device events around every call; -> median over REPS calls after WARM warm-up calls (and of per_call()'s figures)."""
    t, extra = [], []
    for i in range(WARM + REPS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        if i >= WARM:
            t.append(s.elapsed_time(e))
            if per_call:
                extra.append(per_call())
    if extra:                                # the run-to-run spread of the figures: [min, max] over the REPS calls
        SPREAD.update(call=[round(min(t), 3), round(max(t), 3)], launches=np.round(np.stack([np.min(extra, 0), np.max(extra, 0)], 1), 4).tolist())
    return float(np.median(t)), (np.median(np.asarray(extra), 0).tolist() if extra else None)


out = {}


def call():
    out["o"] = pipe(frames, gt_boxes, gt_names, params=params, candidates=candidates)


def launch_times():
    """[select, drop plan, collate]"""
    pe = getattr(pipe, "plan_events", None)
    plan = pe[0].elapsed_time(pe[1]) if pe else 0.0
    return [pipe.kernel_events[0].elapsed_time(pipe.kernel_events[1]), plan, pipe.kernel_events[1].elapsed_time(pipe.kernel_events[2]) - plan]


call_ms, (select_ms, plan_ms, collate_ms) = median_ms(call, launch_times)
o = out["o"]
n_valid = int(sum(v.sum() for v in o["sampled_valid"]))
n_cand = int(sum(len(v) for v in o["sampled_valid"]))

# the floor: gdmae_augment_collate on the same frames, resident on the device
dev = o["points"].device
n_raw = sum(f.shape[0] for f in frames)
raw = torch.from_numpy(np.concatenate(frames)).to(dev)
foff = torch.from_numpy(np.concatenate([[0], np.cumsum([f.shape[0] for f in frames])]).astype(np.int32)).to(dev)
tab = torch.from_numpy(ip.params_table(params)).to(dev)
buf = torch.empty(n_raw, 1 + F, device=dev)
kept = torch.empty(B + 1, dtype=torch.int32, device=dev)
ws = torch.empty(L.load().gdmae_augment_collate_workspace_bytes(n_raw), dtype=torch.uint8, device=dev)
floor_ms, _ = median_ms(lambda: L.call("gdmae_augment_collate", L.ptr(raw), n_raw, F, L.ptr(foff), B, L.ptr(tab), L.host_f32(pipe.xy_range),
                                       L.ptr(buf), L.ptr(kept), L.ptr(ws), L.stream()))

# the numpy statement of the same batch on the host
dbp = pipe.database
cands = []
for c in candidates:
    ents = np.concatenate([dbp.class_index[n][i] for n, i in c]) if c else np.zeros(0, np.int64)
    cands.append({"boxes": dbp.boxes[ents], "names": dbp.names[ents].tolist(), "group": [CLASS_NAMES.index(n) for n in dbp.names[ents]],
                  "points": [dbp.points[dbp.offsets[e, 0]:dbp.offsets[e, 1]] for e in ents]} if len(ents) else None)
t0 = time.perf_counter()
if LIST == "gd_mae":
    st = fr.pipeline(frames, gt_boxes, gt_names, CLASS_NAMES, rng, params, cands=cands, n_groups=3, perms=None)
else:
    st = far.pipeline(frames, gt_boxes, gt_names, CLASS_NAMES, rng, params, cands=cands, n_groups=3, translation=LIST == "ts")
cpu_ms = (time.perf_counter() - t0) * 1e3
agree = [v.tolist() for v in st["valid"]] == [v.tolist() for v in o["sampled_valid"]] and st["num_gt"] == o["num_gt"] \
    and st["points"].shape[0] == o["points"].shape[0] and (LIST == "gd_mae" or (st["drop_n"] == o["drop_n"] and st["drop_k"] == o["drop_k"]))
n_rows = n_raw + sum(int(dbp.offsets[e, 1] - dbp.offsets[e, 0]) for c in candidates for n, i in c for e in dbp.class_index[n][i])
scan_launches = 1 if n_rows <= 65536 else 3                  # gd_device_scan: one workgroup's loop, or reduce + spine + apply
launches = {"select": 1, "drop_plan": 0 if LIST == "gd_mae" else 13, "collate": 1 + scan_launches}      # memsets counted; plan: 1 + 6 x (histogram + pick)

print(json.dumps({"list": LIST, "launches": launches, "drop_plan_ms": round(plan_ms, 4),
                  "min_max_call_ms": SPREAD["call"], "min_max_select_plan_collate_ms": SPREAD["launches"], "drop_k": o.get("drop_k"),
                  "workload": f"{B} frames, {n_raw} scene points, {F} features, {sum(len(n) for n in gt_names)} GT boxes, {n_cand} candidates ({n_valid} valid)",
                  "kept_points": int(o["points"].shape[0]), "kept_boxes": o["num_gt"],
                  "call_device_ms_incl_staging_h2d_shuffle": round(call_ms, 3), "select_kernel_ms": round(select_ms, 4),
                  "collate_kernel_ms": round(collate_ms, 4), "floor_augment_collate_ms": round(floor_ms, 4),
                  "numpy_statement_cpu_ms_per_batch": round(cpu_ms, 1), "statement_counts_agree": bool(agree)}))
