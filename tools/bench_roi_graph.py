"""Second stage behind the pooling (gdmae_roi_graph_forward) at the workload's own shape, next to the torch modules it replaces.

    python tools/bench_roi_graph.py [--batch 8] [--rois 500] [--repeats 20] [--warmup 3]

The cloud and the RoIs of tools/bench_roi_pool.py: 8 x ~180 k synthetic points, 500 seeded RoIs per sample.  Three times, device
events around ``--repeats`` calls after ``--warmup`` calls, the median reported: the pooling (gdmae_roi_dfvs_pool), the fp32 torch
head on the pooled tensors (``pooled_to_features`` + ``heads``: the exact mode's graph network, shared layer and two heads) and the
two launches of gdmae_roi_graph_forward on the same tensors (which also decode the boxes and fuse the scores).  One JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd"), os.path.join(REPO, "tools")]

from bench_roi_pool import seeded_rois  # noqa: E402
from gdmae_hip import configs, inference, synth  # noqa: E402
from gdmae_hip import lib as L  # noqa: E402
from pcdet.models.roi_heads.graphrcnn_head import GraphRCNNHead  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rois", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    _, ds, skw = configs.named_config("B")
    pts = synth.synth_batch(100, a.batch, ds.point_cloud_range, **skw)
    B, M = a.batch, a.rois
    points = torch.from_numpy(pts).cuda()
    rois = torch.from_numpy(seeded_rois(pts, B, M)).cuda()
    scores = torch.rand(B, M, generator=torch.Generator().manual_seed(1)).cuda()
    torch.manual_seed(0)
    head = GraphRCNNHead(input_channels=pts.shape[1] - 4, model_cfg=configs.graphrcnn_head_cfg(), point_cloud_range=ds.point_cloud_range,
                         num_class=1).cuda().eval()
    r = head.pc_range
    lib = L.load()
    packed = torch.empty(lib.gdmae_roi_graph_packed_bytes(), dtype=torch.uint8, device="cuda")
    with torch.no_grad():
        L.call("gdmae_roi_graph_pack", L.ptr(inference.fold_roi_head(head)), L.ptr(packed), L.stream())
    T = B * M
    out = [torch.empty(T, c, dtype=torch.float32, device="cuda") for c in (1, 7, 7, 1)]
    ws = torch.empty(lib.gdmae_roi_graph_workspace_bytes(T), dtype=torch.uint8, device="cuda")

    def pool():
        return head.roilocal_dfvs_pool3d_layer.pool(points, rois, range_xy=[r[0], r[1], r[3], r[4]])
    _, num, feats, _ = pool()

    def torch_head():
        with torch.no_grad():
            f = feats * (num.view(-1) > 0).unsqueeze(-1).unsqueeze(-1)
            return head.heads(head.pooled_to_features(f, B, M), B, M)

    def kernels():
        L.call("gdmae_roi_graph_forward", L.ptr(feats), L.ptr(num), L.ptr(rois), 7, L.ptr(scores), B, M, 1, L.ptr(packed), L.ptr(out[0]),
               L.ptr(out[1]), L.ptr(out[2]), L.ptr(out[3]), None, L.ptr(ws), ws.numel(), L.stream())

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])
    res = {}
    for name, fn in (("pool_ms", pool), ("torch_head_ms", torch_head), ("roi_graph_ms", kernels)):
        for _ in range(a.warmup):
            timed(fn)
        res[name] = round(statistics.median(timed(fn) for _ in range(a.repeats)), 4)
    cls_t, reg_t = torch_head()
    kernels()
    torch.cuda.synchronize()
    res.update(torch_over_kernels=round(res["torch_head_ms"] / res["roi_graph_ms"], 2), batch=B, rois_per_sample=M, points=int(pts.shape[0]),
               pooled_mean=round(float(num.float().mean()), 1), empty_rois=int((num == 0).sum()),
               cls_dev=float((cls_t - out[0]).abs().max()), reg_dev=float((reg_t - out[1]).abs().max()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
