"""Inference timing of the config-D detector on one GPU: the engine (gdmae_hip.inference.compile_detector) against the model's own
evaluation path (model.eval() under bf16 autocast and torch.no_grad()), same process, same seeded synthetic KITTI-shape frames, the
two alternating, warm-up excluded, events around the timed loop and one sync after it.

    python tools/bench_inference.py [--batches 1 8] [--runs 5] [--calls 10] [--warmup 3] [--path both|engine|parent]

Prints every run pair, the medians, frames/s, the kernel-launch count of one engine call and of one parent call (torch profiler,
device activity), and the bytes of the encoder's backward-only side outputs one engine call writes.  --path engine | parent runs one
path only (for a kernel trace of its own)."""
import argparse
import logging
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd")]
from gdmae_hip import configs, inference, synth  # noqa: E402
from gdmae_hip import encoder as genc  # noqa: E402
from pcdet.models import build_network  # noqa: E402


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    except Exception as ex:      # the tracer is optional: the timing does not depend on it
        return f"unavailable ({type(ex).__name__})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--path", default="both", choices=["both", "engine", "parent"])
    ap.add_argument("--no-launch-count", action="store_true", help="skip the in-process tracer (when an external kernel trace runs)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg, ds, skw = configs.named_config("D")
    torch.manual_seed(3)
    net = build_network(cfg, len(ds.class_names), ds, logging.getLogger("bench")).to(dev).eval()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():        # running statistics that are not the (0, 1) initialisation
        for m in net.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    eng = inference.compile_detector(net)
    for B in args.batches:
        pts = torch.from_numpy(synth.synth_batch(100 + B, B, ds.point_cloud_range, **skw)).to(dev)

        def engine():
            return eng({"points": pts, "batch_size": B})

        def parent():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                return net({"points": pts, "batch_size": B})
        paths = [("engine", engine), ("parent", parent)]
        if args.path != "both":
            paths = [p for p in paths if p[0] == args.path]
        for _, fn in paths:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        res = {name: [] for name, _ in paths}
        for r in range(args.runs):
            for name, fn in paths:
                res[name].append(timed(fn, args.calls))
            print(f"batch {B} run {r}: " + "  ".join(f"{name} {res[name][-1]:.3f} ms" for name, _ in paths), flush=True)
        for name, fn in paths:
            med = statistics.median(res[name])
            print(f"batch {B} {name}: median {med:.3f} ms per call, {B / med * 1e3:.1f} frames/s, launches per call {'-' if args.no_launch_count else launches(fn)}", flush=True)
        if len(paths) == 2:
            print(f"batch {B}: engine / parent median = {statistics.median(res['engine']) / statistics.median(res['parent']):.3f}", flush=True)
        if args.path != "parent" and not args.no_launch_count:
            maps = eng.head_maps({"points": pts, "batch_size": B})
            # backward-only side outputs of gdmae_encoder_stage_fwd (gdmae_encoder_layer_bytes: the `saved` block per layer)
            from pcdet.models.backbones_3d.spt_backbone import stage_plan_args
            from gdmae_hip import plan as gplan
            vox = gplan.voxelize(pts, net.vfe.point_cloud_range, net.vfe.voxel_size, net.vfe.grid_size, B)
            ep = gplan.encoder_plan(vox, *stage_plan_args(net.backbone_3d.model_cfg.SST_BLOCK_LIST), keep_frac=None)
            tot = 0
            for si, (blk, sp) in enumerate(zip(net.backbone_3d.sst_blocks, ep.stages)):
                l0 = blk.encoder_blocks[0].encoder_list[0]
                nl = sum(len(b.encoder_list) for b in blk.encoder_blocks)
                sb, _, _ = genc._layer_bytes(sp.n_tok, blk.d_model, l0.linear1.weight.shape[0], l0.win_attn.self_attn.num_heads, 1)
                tot += nl * sb
                print(f"batch {B} stage {si + 1}: {sp.n_tok} tokens, d = {blk.d_model}, {nl} layers x {sb / 1e6:.2f} MB saved block")
            print(f"batch {B}: N = {vox.N} points, M = {vox.M} pillars, encoder backward-only side outputs {tot / 1e6:.1f} MB per call "
                  f"(upper bound: the whole saved blocks)", flush=True)
            del maps


if __name__ == "__main__":
    main()
