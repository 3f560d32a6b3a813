"""Anchor head of the KITTI fine-tune config: fused HIP path against the module's op-by-op torch path on one device.

    python tools/bench_anchor_head.py [--batches 2 16] [--pairs 5] [--calls 10] [--step]

Per batch size: head forward + target assignment + loss + backward (``spatial_features_2d`` in, its gradient and the six
parameter gradients out), ms per call.  The two paths alternate: ``--pairs`` run pairs of ``--calls`` calls each after a warm-up,
medians over the pairs (the scheme of tools/bench_inference.py).  Launch counts come from the profiler in a run of its own
(``rocprofv3 --kernel-trace --stats -- python tools/bench_anchor_head.py --batches 2 --pairs 1 --calls 1 --only fused``).
``--eval``: the evaluation path (decode + score selection + NMS) instead.  ``--step``: one full PointPillar training step (forward, backward, optimizer) at B = 16 in frames / s.  One JSON line per result."""
import argparse
import json
import logging
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd"), os.path.join(REPO, "tests")]

from gdmae_hip import configs, optim, synth  # noqa: E402


def boxes(B, n=24, seed=3):
    rng = np.random.default_rng(seed)
    pcr = configs.KITTI['point_cloud_range']
    out = np.zeros((B, n, 8), dtype=np.float32)
    size = {1: (3.9, 1.6, 1.56), 2: (0.8, 0.6, 1.73), 3: (1.76, 0.6, 1.73)}
    for b in range(B):
        m = int(rng.integers(n // 2, n - 1))
        cls = rng.integers(1, 4, m)
        out[b, :m, 0] = rng.uniform(pcr[0] + 1, pcr[3] - 1, m)
        out[b, :m, 1] = rng.uniform(pcr[1] + 1, pcr[4] - 1, m)
        out[b, :m, 2] = rng.uniform(-1.5, 0.5, m)
        out[b, :m, 3:6] = np.array([size[int(c)] for c in cls]) * rng.uniform(0.8, 1.3, (m, 3))
        out[b, :m, 6] = rng.uniform(-np.pi, np.pi, m)
        out[b, :m, 7] = cls
    return out


def head_call(head, sf, gt, fused):
    head.fused = fused
    for p in head.parameters():
        p.grad = None
    x = sf.detach().requires_grad_(True)
    head({"spatial_features_2d": x, "gt_boxes": gt, "batch_size": sf.shape[0]})
    loss, _ = head.get_loss()
    loss.backward()
    return loss


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def bench_head(B, pairs, calls, only):
    from pcdet.models.dense_heads import AnchorHeadSingle
    dev = torch.device("cuda:0")
    ds = configs.SyntheticDatasetInfo(**configs.KITTI)
    torch.manual_seed(1)
    head = AnchorHeadSingle(model_cfg=configs.anchor_head_cfg(), input_channels=128, num_class=3, class_names=ds.class_names,
                            grid_size=ds.grid_size, point_cloud_range=ds.point_cloud_range, predict_boxes_when_training=False).to(dev).train()
    sf = (torch.randn(B, 128, 248, 216, device=dev) * 0.5).contiguous(memory_format=torch.channels_last)
    gt = torch.from_numpy(boxes(B)).to(dev)
    modes = [m for m in (("fused", True), ("torch", False)) if only in (None, m[0])]
    for name, f in modes:                                   # warm-up: algorithm selection of the GEMM front end, allocator
        for _ in range(3):
            head_call(head, sf, gt, f)
    res = {name: [] for name, _ in modes}
    for _ in range(pairs):
        for name, f in modes:
            res[name].append(timed(lambda: head_call(head, sf, gt, f), calls))
    out = {"bench": "anchor_head_train", "B": B, "pairs": pairs, "calls": calls}
    for name in res:
        out[name + "_ms"] = round(statistics.median(res[name]), 3)
        out[name + "_ms_all"] = [round(v, 3) for v in res[name]]
    if len(res) == 2:
        out["torch_over_fused"] = round(out["torch_ms"] / out["fused_ms"], 2)
    print(json.dumps(out), flush=True)


def bench_eval(B, pairs, calls):
    """Evaluation: head forward (decode) + post_processing (score selection, top-k, rotated NMS), fused against torch ops."""
    from pcdet.models.dense_heads import AnchorHeadSingle
    from pcdet.models.detectors import PointPillar
    dev = torch.device("cuda:0")
    cfg, ds = configs.kitti_finetune_cfg()
    torch.manual_seed(1)
    head = AnchorHeadSingle(model_cfg=cfg.DENSE_HEAD, input_channels=128, num_class=3, class_names=ds.class_names, grid_size=ds.grid_size,
                            point_cloud_range=ds.point_cloud_range, predict_boxes_when_training=False).to(dev).eval()
    with torch.no_grad():
        head.conv_cls.weight.mul_(8.0)                      # spread the scores: a few thousand anchors pass SCORE_THRESH = 0.3
        head.conv_cls.bias.fill_(-4.0)
    det = PointPillar.__new__(PointPillar)
    torch.nn.Module.__init__(det)
    det.model_cfg, det.num_class = cfg, 3
    sf = (torch.randn(B, 128, 248, 216, device=dev) * 0.5).contiguous(memory_format=torch.channels_last)
    kept = {}

    def call(fused):
        head.fused = det.fused_select = fused
        with torch.no_grad():
            dd = head({"spatial_features_2d": sf, "batch_size": B})
            pd, _ = det.post_processing(dd)
        kept[fused] = [int(p["pred_boxes"].shape[0]) for p in pd]
        return dd
    dd = None
    for f in (True, False):
        for _ in range(3):
            dd = call(f)
    n_sel = (torch.sigmoid(dd["batch_cls_preds"]).max(-1)[0] >= 0.3).sum(1).tolist()
    res = {True: [], False: []}
    for _ in range(pairs):
        for f in (True, False):
            res[f].append(timed(lambda: call(f), calls))
    out = {"bench": "anchor_head_eval", "B": B, "pairs": pairs, "calls": calls, "above_threshold": n_sel, "final_boxes": kept[True],
           "final_boxes_torch": kept[False], "fused_ms": round(statistics.median(res[True]), 3), "torch_ms": round(statistics.median(res[False]), 3),
           "fused_ms_all": [round(v, 3) for v in res[True]], "torch_ms_all": [round(v, 3) for v in res[False]]}
    print(json.dumps(out), flush=True)


def bench_step(B, steps=6, warmup=3):
    from pcdet.models import build_network, model_fn_decorator
    dev = torch.device("cuda:0")
    cfg, ds = configs.kitti_finetune_cfg()
    torch.manual_seed(3)
    net = build_network(cfg, 3, ds, logging.getLogger("bench")).to(dev).train()
    net.sync_loss_scalar = False
    opt = optim.FlatAdamOneCycle(net, configs.optimization_cfg(B), total_steps=steps + warmup + 1)
    pts = synth.synth_batch(77, B, ds.point_cloud_range, beams=32, azimuths=600, extra=800, features=4)
    gt = boxes(B)
    fn = model_fn_decorator()

    def step(i):
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ret = fn(net, {"points": pts.copy(), "gt_boxes": gt.copy(), "batch_size": B})
        ret.loss.backward()
        opt.step(i)
    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(warmup + i)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    print(json.dumps({"bench": "pointpillar_train_step", "B": B, "ms_per_step": round(dt * 1e3, 2), "frames_per_s": round(B / dt, 1)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[2, 16])
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--only", choices=["fused", "torch"], default=None)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--eval", action="store_true", help="evaluation path instead: decode + post_processing, fused against torch ops")
    a = ap.parse_args()
    for B in a.batches:
        if a.eval:
            bench_eval(B, a.pairs, a.calls)
        else:
            bench_head(B, a.pairs, a.calls, a.only)
    if a.step:
        bench_step(16)
