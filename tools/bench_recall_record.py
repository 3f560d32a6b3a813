"""gdmae_recall_record alone at B = 8, n = 500 predicted boxes, M = 500 RoIs and about 100 GT boxes per sample, T = 3,
against the per-sample ``Detector3DTemplate.generate_recall_record`` loop on the same device tensors (nonzero + int() to trim the GT
rows, two pair matrices through ``boxes_iou3d_gpu``, two .item() reads per threshold).  The library's side ends in the one host read of
``RecallRecord.result()`` so that both sides deliver the same Python dict.  Five runs of 20 calls each, device events around calls that
end in a synchronise, the two cases alternating.

    python tools/bench_recall_record.py"""
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd")]
from gdmae_hip import evaluation  # noqa: E402
from pcdet.models.detectors.detector3d_template import Detector3DTemplate  # noqa: E402

assert torch.cuda.is_available(), "bench_recall_record needs a GPU"
dev = torch.device("cuda:0")
Bn, N, M, G, NGT = 8, 500, 500, 128, 100
THRESH = [0.3, 0.5, 0.7]
rng = np.random.RandomState(1)
SIZES = np.array([[4.6, 2.0, 1.7], [0.9, 0.8, 1.75], [1.8, 0.8, 1.7]])


def around(gt_b, n_live, k_near, k_far, rows, spread):
    """k_near boxes around GT boxes at every overlap, k_far anywhere, the rest of ``rows`` zero"""
    out = np.zeros((rows, 7), np.float32)
    src = rng.randint(0, n_live, k_near)
    out[:k_near] = gt_b[src, :7]
    out[:k_near, 0:2] += rng.normal(0, 1, (k_near, 1)) * rng.uniform(0, spread, (k_near, 2))
    out[:k_near, 6] += rng.normal(0, 0.1, k_near)
    far = rng.randint(1, 4, k_far)
    out[k_near:k_near + k_far, 0:2] = rng.uniform(-70, 70, (k_far, 2))
    out[k_near:k_near + k_far, 2] = 0.9
    out[k_near:k_near + k_far, 3:6] = SIZES[far - 1]
    out[k_near:k_near + k_far, 6] = rng.uniform(-np.pi, np.pi, k_far)
    return out


def scene():
    gt = np.zeros((Bn, G, 8), np.float32)
    pred, rois = np.zeros((Bn, N, 7), np.float32), np.zeros((Bn, M, 7), np.float32)
    for b in range(Bn):
        n = NGT + int(rng.randint(-8, 9))
        cls = rng.randint(1, 4, n)
        gt[b, :n, 0:2] = rng.uniform(-70, 70, (n, 2))
        gt[b, :n, 2] = rng.uniform(0.5, 1.2, n)
        gt[b, :n, 3:6] = SIZES[cls - 1] * rng.uniform(0.9, 1.1, (n, 3))
        gt[b, :n, 6] = rng.uniform(-np.pi, np.pi, n)
        gt[b, :n, 7] = cls
        rois[b] = around(gt[b], n, 330, 150, M, 1.2)          # the last 20 rows stay padded
        pred[b] = around(gt[b], n, 330, 150, N, 0.6)
    t = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    num = torch.full((Bn,), 480, dtype=torch.int32, device=dev)
    return t(pred), num, t(rois), num.clone(), t(gt)


pred, pred_num, rois, roi_num, gt_boxes = scene()
record = evaluation.RecallRecord(THRESH, dev)


def run_hip():
    record.reset()
    record.update(pred, pred_num, gt_boxes, rois=rois, roi_num=roi_num)
    return record.result()


def run_loop():
    dd = {'gt_boxes': gt_boxes, 'rois': rois}                 # all M RoI rows, as post_processing_without_nms passes them
    out = {}
    for b in range(Bn):
        out = Detector3DTemplate.generate_recall_record(pred[b, :480], out, b, data_dict=dd, thresh_list=THRESH)
    return out


def timed(fn, calls=20):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


cases = {"gdmae_recall_record (2 launches + 1 read)": run_hip, "per-sample generate_recall_record loop": run_loop}
for k, fn in cases.items():
    for _ in range(3):
        o = fn()
    torch.cuda.synchronize()
    print(k, o, flush=True)
res = {k: [] for k in cases}
for r in range(5):
    for k, fn in cases.items():
        res[k].append(timed(fn))
    print(f"run {r}: " + "  ".join(f"{k} {res[k][-1] * 1e3:.1f} us" for k in cases), flush=True)
for k in cases:
    print(f"{k}: median {statistics.median(res[k]) * 1e3:.1f} us per call (B = {Bn}, n = {N}, M = {M}, ~{NGT} GT boxes, T = {len(THRESH)})", flush=True)
