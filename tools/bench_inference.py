"""Inference timing of a fine-tuned detector on one GPU: the engine (gdmae_hip.inference.compile_detector) against the model's own
evaluation path (model.eval() under bf16 autocast - and in fp32 with --fp32 - and torch.no_grad()), same process, same seeded
synthetic KITTI-shape frames, the paths alternating, warm-up excluded, events around the timed loop and one sync after it.

    python tools/bench_inference.py [--config D|kitti|ts] [--batches 1 8] [--runs 5] [--calls 10] [--warmup 3]
                                    [--path both|engine|parent|detect]

--config D: the CenterPoint detector of config D (0.16 m pillars).  --config kitti: the PointPillar / AnchorHeadSingle detector of
the shipped KITTI fine-tune config (configs.kitti_finetune_cfg(), 0.32 m pillars), conv_cls.bias set so that the scores straddle
SCORE_THRESH; this run also times the head alone on the engine's bf16 BEV map: gdmae_anchor_head_infer (two launches) against the
row product on the library GEMM + gdmae_anchor_decode + gdmae_anchor_select.

--config ts: the two-stage GraphRCNN detector of configs.waymo_two_stage_cfg() (Waymo-shape grid and cloud, CenterHead with
multi_class_nms over three classes, then the RoI head); it has engine paths only.  --path detect: ``engine.detect`` (the batched
CenterHead tail; with --config kitti the batched anchor-head tail) against ``engine(batch_dict)`` (the
op-by-op tail: what the engine call has been since the engines were added), alternating; then the two tails alone on the same head
maps (--config kitti: on the same survivors of the head), with their launch counts.

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


def head_alone(eng, net, pts, B, args):
    """The anchor head alone on the engine's bf16 BEV map: the two-launch inference entry against the parent's evaluation head (row
    product on the library GEMM under bf16 autocast, gdmae_anchor_decode, gdmae_anchor_select)."""
    from gdmae_hip import lib as L
    hd = net.dense_head
    with torch.no_grad(), torch.autocast("cuda", enabled=False):
        x2 = eng._trunk({"points": pts, "batch_size": B})[1]
    sf2 = x2.permute(0, 3, 1, 2)
    thresh = float(net.model_cfg.POST_PROCESSING.SCORE_THRESH)

    def new():
        with torch.no_grad():
            return eng._head(x2, False)[0]

    def old():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            d = hd({"spatial_features_2d": sf2, "batch_size": B})
        cls = d["batch_cls_preds"]
        n, C = cls.shape[1], cls.shape[2]
        idx = torch.empty(B, n, dtype=torch.int32, device=cls.device)
        score = torch.empty(B, n, dtype=torch.float32, device=cls.device)
        label = torch.empty(B, n, dtype=torch.int32, device=cls.device)
        count = torch.empty(B, dtype=torch.int32, device=cls.device)
        L.call("gdmae_anchor_select", L.ptr(cls), B, n, C, 0, thresh, L.ptr(idx), L.ptr(score), L.ptr(label), L.ptr(count), L.stream())
        return count
    for fn in (new, old):
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    print(f"batch {B} head alone: survivors per sample, new {new().tolist()}  parent {old().tolist()}", flush=True)
    res = {"new": [], "parent": []}
    for r in range(args.runs):
        res["new"].append(timed(new, args.calls))
        res["parent"].append(timed(old, args.calls))
        print(f"batch {B} head run {r}: new {res['new'][-1]:.3f} ms  parent {res['parent'][-1]:.3f} ms", flush=True)
    a, b = statistics.median(res["new"]), statistics.median(res["parent"])
    print(f"batch {B} head alone: new {a:.3f} ms, parent (gemm + decode + select) {b:.3f} ms, new / parent = {a / b:.3f}", flush=True)


def tails_alone(eng, net, pts, B, args):
    """The CenterHead tail alone on the engine's head maps: generate_predicted_boxes (op-by-op: per sample and class a mask gather, a
    sort, a two-launch NMS and a host read) against generate_predicted_boxes_batched (sigmoid, top-K and three launches)."""
    hd = net.dense_head
    maps = eng.head_maps({"points": pts, "batch_size": B})

    def old():
        with torch.no_grad(), torch.autocast("cuda", enabled=False):
            return hd.generate_predicted_boxes(B, maps)

    def new():
        with torch.no_grad(), torch.autocast("cuda", enabled=False):
            return hd.generate_predicted_boxes_batched(B, maps)
    for fn in (new, old):
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    print(f"batch {B} tail alone: boxes per sample, batched {new()['num'].tolist()}  op-by-op {[int(d['pred_boxes'].shape[0]) for d in old()]}",
          flush=True)
    res = {"new": [], "old": []}
    for r in range(args.runs):
        res["new"].append(timed(new, args.calls))
        res["old"].append(timed(old, args.calls))
        print(f"batch {B} tail run {r}: batched {res['new'][-1]:.3f} ms  op-by-op {res['old'][-1]:.3f} ms", flush=True)
    a, b = statistics.median(res["new"]), statistics.median(res["old"])
    print(f"batch {B} tail alone: batched {a:.3f} ms ({launches(new)} launches), op-by-op {b:.3f} ms ({launches(old)} launches), "
          f"batched / op-by-op = {a / b:.3f}", flush=True)


def anchor_tails_alone(eng, net, pts, B, args):
    """The anchor-head tail alone on the same ``_head`` output: the host read of the counts + the ``finish_sample`` loop (per sample a
    top-k, three gathers, a sort, a two-launch NMS and a host read) against ``finish_batch`` (three launches)."""
    with torch.no_grad(), torch.autocast("cuda", enabled=False):
        x2 = eng._trunk({"points": pts, "batch_size": B})[1]
        count, score, label, box, _ = eng._head(x2, False)

    def old():
        with torch.no_grad(), torch.autocast("cuda", enabled=False):
            counts = count.tolist()
            recall, preds = {}, []
            for b in range(B):
                n = counts[b]
                pred, recall = net.finish_sample(box[b, :n], score[b, :n], label[b, :n].long(), recall, b, {"batch_size": B})
                preds.append(pred)
            return preds

    def new():
        with torch.no_grad(), torch.autocast("cuda", enabled=False):
            return net.finish_batch(count, score, label, box)
    for fn in (new, old):
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    print(f"batch {B} tail alone: survivors per sample {count.tolist()}; boxes per sample, batched {new()['num'].tolist()}  "
          f"op-by-op {[int(d['pred_boxes'].shape[0]) for d in old()]}", flush=True)
    res = {"new": [], "old": []}
    for r in range(args.runs):
        res["new"].append(timed(new, args.calls))
        res["old"].append(timed(old, args.calls))
        print(f"batch {B} tail run {r}: batched {res['new'][-1]:.3f} ms  op-by-op {res['old'][-1]:.3f} ms", flush=True)
    a, b = statistics.median(res["new"]), statistics.median(res["old"])
    print(f"batch {B} tail alone: batched {a:.3f} ms ({launches(new)} launches), op-by-op {b:.3f} ms ({launches(old)} launches), "
          f"batched / op-by-op = {a / b:.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="D", choices=["D", "kitti", "ts"])
    ap.add_argument("--fp32", action="store_true", help="also time the parent's fp32 evaluation path")
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--path", default="both", choices=["both", "engine", "parent", "detect"])
    ap.add_argument("--no-launch-count", action="store_true", help="skip the in-process tracer (when an external kernel trace runs)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.config == "kitti":
        cfg, ds = configs.kitti_finetune_cfg()
        skw = dict(beams=32, azimuths=600, extra=800, features=4)
    elif args.config == "ts":
        cfg, ds = configs.waymo_two_stage_cfg()
        skw = dict(beams=64, azimuths=2650, extra=10400, features=5)
        if args.path != "detect":
            ap.error("--config ts has engine paths only: use --path detect")
    else:
        cfg, ds, skw = configs.named_config("D")
    torch.manual_seed(3)
    net = build_network(cfg, len(ds.class_names), ds, logging.getLogger("bench")).to(dev).eval()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():        # running statistics that are not the (0, 1) initialisation
        for m in net.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
        if args.config == "kitti":      # scores on both sides of SCORE_THRESH instead of the 0.01 prior of init_weights: the best-class
            # logit of this seeded model without the bias spans -0.19 ... 0.33 (quartiles -0.11 / 0.08 / 0.27), the threshold is -0.847
            net.dense_head.conv_cls.bias.fill_(-1.03)
    eng = inference.compile_detector(net)
    for B in args.batches:
        pts = torch.from_numpy(synth.synth_batch(100 + B, B, ds.point_cloud_range, **skw)).to(dev)

        def engine():
            return eng({"points": pts, "batch_size": B})

        def parent():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                return net({"points": pts, "batch_size": B})
        def parent_fp32():
            with torch.no_grad():
                return net({"points": pts, "batch_size": B})
        def detect():
            return eng.detect({"points": pts, "batch_size": B})
        paths = [("engine", engine), ("parent", parent)]
        if args.path == "detect":
            paths = [("detect", detect), ("engine", engine)]
        elif args.path != "both":
            paths = [p for p in paths if p[0] == args.path]
        if args.fp32 and args.path != "engine":
            paths.append(("parent_fp32", parent_fp32))
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
        for other in ("parent", "parent_fp32"):
            if "engine" in res and other in res:
                print(f"batch {B}: engine / {other} median = {statistics.median(res['engine']) / statistics.median(res[other]):.3f}", flush=True)
        if args.config == "kitti" and args.path == "both":
            head_alone(eng, net, pts, B, args)
        if args.path == "detect":
            print(f"batch {B}: detect / engine median = {statistics.median(res['detect']) / statistics.median(res['engine']):.3f}", flush=True)
            (anchor_tails_alone if args.config == "kitti" else tails_alone)(eng, net, pts, B, args)
            continue
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
