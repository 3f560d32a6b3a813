"""gdmae_roi_targets alone at B = 8, M = 500 RoIs and about 100 GT boxes per sample, R = 128, against a per-sample,
per-class torch loop on ``boxes_iou3d_gpu`` that restates the reference's ProposalTargetLayer + canonical transformation (mask
gathers, nonzero, .item(), host-drawn permutations between the device calls).  Both sides include their host-side draws and the
copy of the uniform numbers to the device.  Five runs of 20 calls each, device events around calls that end in a synchronise, the
two cases alternating.

    python tools/bench_roi_targets.py"""
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd")]
from gdmae_hip import configs  # noqa: E402
from pcdet.models.dense_heads.anchor_head_single import limit_period  # noqa: E402
from pcdet.models.roi_heads import proposal_targets as pt  # noqa: E402
from pcdet.models.roi_heads.roi_head_template import rotate_points_along_z  # noqa: E402
from pcdet.ops.iou3d_nms.iou3d_nms_utils import boxes_iou3d_gpu  # noqa: E402

assert torch.cuda.is_available(), "bench_roi_targets needs a GPU"
dev = torch.device("cuda:0")
Bn, M, G, NGT = 8, 500, 128, 100
cfg = configs.graphrcnn_head_cfg().TARGET_CONFIG
P = pt.sampler_params(cfg)
R = P['R']
rng = np.random.RandomState(1)
SIZES = np.array([[4.6, 2.0, 1.7], [0.9, 0.8, 1.75], [1.8, 0.8, 1.7]])


def scene():
    gt = np.zeros((Bn, G, 8), np.float32)
    rois, labels = np.zeros((Bn, M, 7), np.float32), np.zeros((Bn, M), np.int64)
    for b in range(Bn):
        n = NGT + int(rng.randint(-8, 9))
        cls = rng.randint(1, 4, n)
        gt[b, :n, 0:2] = rng.uniform(-70, 70, (n, 2))
        gt[b, :n, 2] = rng.uniform(0.5, 1.2, n)
        gt[b, :n, 3:6] = SIZES[cls - 1] * rng.uniform(0.9, 1.1, (n, 3))
        gt[b, :n, 6] = rng.uniform(-np.pi, np.pi, n)
        gt[b, :n, 7] = cls
        src = rng.randint(0, n, 330)                                     # RoIs around GT boxes, at every overlap
        rois[b, :330] = gt[b, src, :7]
        rois[b, :330, 0:2] += rng.normal(0, 1, (330, 1)) * rng.uniform(0, 1.2, (330, 2))
        rois[b, :330, 6] += rng.normal(0, 0.1, 330)
        labels[b, :330] = cls[src]
        far = rng.randint(1, 4, 150)                                     # RoIs anywhere; the last 20 rows stay padded
        rois[b, 330:480, 0:2] = rng.uniform(-70, 70, (150, 2))
        rois[b, 330:480, 2] = 0.9
        rois[b, 330:480, 3:6] = SIZES[far - 1]
        rois[b, 330:480, 6] = rng.uniform(-np.pi, np.pi, 150)
        labels[b, 330:480] = far
    t = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    return t(rois), torch.rand(Bn, M, device=dev), t(labels), t(gt)


rois, scores, labels, gt_boxes = scene()


def run_hip():
    u_fg = torch.from_numpy(rng.random_sample((Bn, M)).astype(np.float32)).to(dev)
    u_bg = torch.from_numpy(rng.random_sample((Bn, R)).astype(np.float32)).to(dev)
    return pt.roi_targets_hip(rois, scores, labels, gt_boxes, u_fg, u_bg, P)


def subsample(max_overlaps):
    """subsample_rois / sample_bg_inds of the reference layer, with its host reads"""
    fg_inds = (max_overlaps >= min(P['reg_fg'], P['cls_fg'])).nonzero().view(-1)
    easy = (max_overlaps < P['cls_bg_lo']).nonzero().view(-1)
    hard = ((max_overlaps < P['reg_fg']) & (max_overlaps >= P['cls_bg_lo'])).nonzero().view(-1)
    n_fg, n_bg = fg_inds.numel(), hard.numel() + easy.numel()

    def bg(num):
        if hard.numel() > 0 and easy.numel() > 0:
            h = min(int(num * cfg.HARD_BG_RATIO), len(hard))
            return torch.cat([hard[torch.randint(0, hard.numel(), (h,), device=dev)], easy[torch.randint(0, easy.numel(), (num - h,), device=dev)]])
        lst = hard if hard.numel() > 0 else easy
        return lst[torch.randint(0, lst.numel(), (num,), device=dev)]
    if n_fg > 0 and n_bg > 0:
        f = min(P['fg_per_image'], n_fg)
        perm = torch.from_numpy(np.random.permutation(n_fg)).to(dev).long()
        return torch.cat((fg_inds[perm[:f]], bg(R - f)))
    if n_fg > 0:
        return fg_inds[torch.from_numpy(np.floor(np.random.rand(R) * n_fg)).to(dev).long()]
    return bg(R)


def run_loop():
    out_rois, out_gt, out_iou = rois.new_zeros(Bn, R, 7), rois.new_zeros(Bn, R, 8), rois.new_zeros(Bn, R)
    out_scores, out_labels, out_idx = rois.new_zeros(Bn, R), labels.new_zeros(Bn, R), labels.new_zeros(Bn, R)
    for b in range(Bn):
        cur_gt = gt_boxes[b]
        k = len(cur_gt) - 1
        while k > 0 and cur_gt[k].sum() == 0:
            k -= 1
        cur_gt = cur_gt[:k + 1]
        gl = cur_gt[:, -1].long()
        max_overlaps, assign = rois.new_zeros(M), labels.new_zeros(M)
        for c in range(gl.min().item(), gl.max().item() + 1):
            rm, gm = labels[b] == c, gl == c
            if rm.sum() > 0 and gm.sum() > 0:
                iou = boxes_iou3d_gpu(rois[b][rm], cur_gt[gm][:, :7])
                best, arg = torch.max(iou, dim=1)
                max_overlaps[rm] = best
                assign[rm] = gm.nonzero().view(-1)[arg]
        idx = subsample(max_overlaps)
        out_rois[b], out_labels[b], out_iou[b], out_scores[b] = rois[b][idx], labels[b][idx], max_overlaps[idx], scores[b][idx]
        out_gt[b], out_idx[b] = cur_gt[assign[idx]], idx
    reg_valid = (out_iou > P['reg_fg']).long()
    fg, bgm = out_iou > P['cls_fg'], out_iou < P['cls_bg']
    cls_labels = fg.float()
    mid = ~fg & ~bgm
    cls_labels[mid] = (out_iou[mid] - P['cls_bg']) / (P['cls_fg'] - P['cls_bg'])
    src = out_gt.clone()
    ry = limit_period(out_rois[:, :, 6], offset=0.5, period=np.pi * 2)
    out_gt[:, :, 0:3] = out_gt[:, :, 0:3] - out_rois[:, :, 0:3]
    out_gt[:, :, 6] = out_gt[:, :, 6] - ry
    out_gt = rotate_points_along_z(out_gt.view(-1, 1, 8), -ry.view(-1)).view(Bn, -1, 8)
    out_gt[:, :, 6] = limit_period(out_gt[:, :, 6], offset=0.5, period=np.pi)
    return dict(rois=out_rois, gt_of_rois=out_gt, gt_of_rois_src=src, gt_iou_of_rois=out_iou, roi_scores=out_scores, roi_labels=out_labels,
                roi_indices=out_idx, reg_valid_mask=reg_valid, rcnn_cls_labels=cls_labels)


def timed(fn, calls=20):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


cases = {"gdmae_roi_targets (2 launches)": run_hip, "per-sample, per-class torch loop": run_loop}
for k, fn in cases.items():
    for _ in range(3):
        o = fn()
    torch.cuda.synchronize()
    print(k, "fg rows", int(o['reg_valid_mask'].sum()), "mean overlap", round(float(o['gt_iou_of_rois'].mean()), 4), flush=True)
res = {k: [] for k in cases}
for r in range(5):
    for k, fn in cases.items():
        res[k].append(timed(fn))
    print(f"run {r}: " + "  ".join(f"{k} {res[k][-1] * 1e3:.1f} us" for k in cases), flush=True)
for k in cases:
    print(f"{k}: median {statistics.median(res[k]) * 1e3:.1f} us per call (B = {Bn}, M = {M}, ~{NGT} GT boxes, R = {R})", flush=True)
