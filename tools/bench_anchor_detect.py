"""gdmae_anchor_detect alone at B = 2, A = 321,408, NMS_PRE_MAXSIZE 4096: count = A and count = 107,000 (the selection path: one
workgroup streams the sample's scores) against count = 4096 (the sort path on the same candidates); pairwise distinct scores and sparse
boxes, so that all three calls hand the same 4096 candidates to the NMS.  Five runs of 20 calls, device events, the cases alternating.

    python tools/bench_anchor_detect.py"""
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd")]
from gdmae_hip import lib as L  # noqa: E402

dev = torch.device("cuda:0")
Bn, A = 2, 321408
g = torch.Generator().manual_seed(1)
score = torch.stack([torch.linspace(0.05, 0.95, A)[torch.randperm(A, generator=g)] for _ in range(Bn)]).to(dev)
# the sort-path input: the 4096 best rows first, so that both calls hand the same candidates to the NMS
order = torch.sort(score, dim=1, descending=True)[1]
label = torch.ones(Bn, A, dtype=torch.int32, device=dev)
u = torch.rand(Bn, A, 7, generator=g)
box = torch.stack([u[..., 0] * 2000, u[..., 1] * 2000, u[..., 2], 1 + 3 * u[..., 3], 0.8 + 1.2 * u[..., 4], 1 + u[..., 5], u[..., 6]], dim=-1).to(dev)
score_s = torch.gather(score, 1, order).contiguous()
box_s = torch.gather(box, 1, order[..., None].expand(-1, -1, 7)).contiguous()
ws = torch.empty(L.load().gdmae_anchor_detect_workspace_bytes(Bn, 4096), dtype=torch.uint8, device=dev)
o = [torch.empty(Bn, 500, 7, device=dev), torch.empty(Bn, 500, device=dev), torch.empty(Bn, 500, dtype=torch.int64, device=dev),
     torch.empty(Bn, dtype=torch.int32, device=dev)]


def run(count, sc, bx):
    L.call("gdmae_anchor_detect", L.ptr(count), L.ptr(sc), L.ptr(label), L.ptr(bx), Bn, A, 4096, 500, 0.01, 500, *[L.ptr(x) for x in o], L.ptr(ws),
           L.stream())


def timed(fn, calls=20):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


cases = {"count = A (selection)": (torch.full((Bn,), A, dtype=torch.int32, device=dev), score, box),
         "count = 107,000 (selection)": (torch.full((Bn,), 107000, dtype=torch.int32, device=dev), score, box),
         "count = 4096 (sort only)": (torch.full((Bn,), 4096, dtype=torch.int32, device=dev), score_s, box_s)}
res = {k: [] for k in cases}
for k, v in cases.items():
    for _ in range(3):
        run(*v)
    torch.cuda.synchronize()
    print(k, "num", o[3].tolist(), flush=True)
for r in range(5):
    for k, v in cases.items():
        res[k].append(timed(lambda: run(*v)))
    print(f"run {r}: " + "  ".join(f"{k} {res[k][-1] * 1e3:.1f} us" for k in cases), flush=True)
for k in cases:
    print(f"{k}: median {statistics.median(res[k]) * 1e3:.1f} us per call (B = 2, three launches)", flush=True)
