"""GPU: the shipped two-stage config end to end in eval mode on a small synthetic Waymo-range batch; the second stage on the HIP
pooling against the same second stage on the CPU restatement of the pooling, fed the same RoIs.  Measured GPU-vs-CPU deviation of
the second stage: 1.144e-5 on the boxes, 5.96e-8 on the scores; the test asserts 4 x these."""
import copy
import logging

import numpy as np
import pytest
import torch

from gdmae_hip import configs, synth
from pcdet.models import build_network

pytestmark = pytest.mark.gpu

# measured on an MI355X (this test prints the figures): largest |GPU - CPU| of the fp32 torch graph network + heads over the 35 RoIs
# of the batch below, on boxes (metres / radians; 1.5 fp32 ulp of a 74 m coordinate) and on scores (one ulp of 0.5); the same with
# one and with sixteen CPU threads.  The pooled features of the two runs differ by 4.8e-7, indices and counts not at all.
MEASURED_BOX_DEV = 1.144e-5
MEASURED_SCORE_DEV = 5.96e-8


def _model(seed=5):
    cfg, ds = configs.waymo_two_stage_cfg()
    torch.manual_seed(seed)
    net = build_network(cfg, len(ds.class_names), ds, logging.getLogger("t"))
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                c = m.num_features
                m.running_mean.copy_(torch.randn(c, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(c, generator=g) * 1.0 + 0.5)
                m.weight.copy_(1.0 + 0.2 * torch.randn(c, generator=g))
                m.bias.copy_(0.2 * torch.randn(c, generator=g))
        # fresh reg_layers weights are N(0, 0.001): give the refinement something to do
        net.roi_head.reg_layers.weight.copy_(torch.randn(net.roi_head.reg_layers.weight.shape, generator=g) * 0.05)
        # first-stage boxes standing on the ground and large enough (12 x 6 x 3 m) to hold points of a 16-beam cloud wherever a
        # cell is occupied: the second stage is what this test is about
        sep = net.dense_head.heads_list[0]
        for name, bias in (("dim", np.log([12.0, 6.0, 3.0])), ("center_z", [0.9]), ("center", [0.0, 0.0])):
            conv = getattr(sep, name)[-1]
            conv.weight.mul_(0.02)
            conv.bias.copy_(torch.tensor(np.asarray(bias), dtype=torch.float32))
    return net.cuda().eval(), ds


def test_two_stage_eval_matches_cpu_pooling_second_stage():
    net, ds = _model()
    B = 2
    pts = synth.synth_batch(31, B, ds.point_cloud_range, beams=16, azimuths=1100, extra=3000, features=5)
    assert 30000 < pts.shape[0] < 50000
    points = torch.from_numpy(pts).cuda()
    with torch.no_grad():
        # Bias the heat map so that a few dozen cells pass SCORE_THRESH, where the cloud is dense.  Far from any point the BEV
        # features are one constant vector; the final heat-map convolution gets 1 x 1 weights along the direction in which the
        # cells with at least 20 points within 1.3 m differ from it, orthogonal to the vector itself: empty ground scores exactly
        # the bias, dense cells score highest, and the bias puts the 60th best cell on the threshold.
        d = {"points": points, "batch_size": B}
        for m in net.module_list[:3]:
            d = m(d)
        sep = net.dense_head.heads_list[0]
        act = sep.hm[0](net.dense_head.shared_conv(d["spatial_features_2d"].float()))          # (B, 64, H, W) input of the final conv
        H, W = act.shape[2:]
        r0, vs = ds.point_cloud_range, ds.voxel_size
        cx = ((points[:, 1] - float(r0[0])) / vs[0]).long().clamp(0, W - 1)
        cy = ((points[:, 2] - float(r0[1])) / vs[1]).long().clamp(0, H - 1)
        cnt = torch.bincount((points[:, 0].long() * H + cy) * W + cx, minlength=B * H * W).view(B, 1, H, W).float()
        busy = torch.nn.functional.avg_pool2d(cnt, 9, stride=1, padding=4) * 81 >= 20
        far = torch.nn.functional.avg_pool2d(cnt, 41, stride=1, padding=20) == 0
        far[:, :, :24], far[:, :, -24:], far[:, :, :, :24], far[:, :, :, -24:] = False, False, False, False      # off the map border
        assert int(far.sum()) > 1000
        a0 = act.permute(0, 2, 3, 1)[far[:, 0]].double()
        print("empty-ground activation spread", float((a0 - a0.median(0)[0]).abs().max()), "over", a0.shape[0], "cells")
        a0 = a0.median(0)[0]
        u = act.permute(0, 2, 3, 1)[busy[:, 0]].double().mean(0) - a0
        u = u - (u @ a0) * a0 / (a0 @ a0)
        w = (50.0 * u / u.norm() * torch.tensor([1.0, 0.9, 0.8], dtype=torch.float64, device=u.device)[:, None]).float()
        final = sep.hm[-1]
        final.weight.zero_()
        final.weight[:, :, 1, 1] = w
        logits = torch.einsum("bchw,kc->bkhw", act, w)
        kth = torch.topk(logits.reshape(-1), 60)[0][-1]
        thr = net.dense_head.model_cfg.POST_PROCESSING.SCORE_THRESH
        assert float(kth) > 0.5 and int(busy.sum()) > 200          # empty ground scores 0 +- rounding
        final.bias.fill_(float(np.log(thr / (1 - thr))) - float(kth))
        bd = {"points": points, "batch_size": B}
        preds, recall = net(bd)
    rois, roi_scores, roi_labels = bd["rois"], bd["roi_scores"], bd["roi_labels"]
    n_roi = (roi_labels != 0).sum(dim=1)
    print("RoIs per sample", n_roi.tolist(), "padded to", rois.shape[1], "first RoIs", rois[0, :3].cpu().numpy().round(2).tolist())
    assert 24 <= int(n_roi.sum()) <= 60 and rois.shape[1] <= 500 and bd["has_class_labels"] is True
    # shapes follow the reference: one dict per sample, at most 500 rows, labels from the first stage, padded rows dropped
    assert len(preds) == B and recall == {}
    for b in range(B):
        n = int(n_roi[b])
        assert preds[b]["pred_boxes"].shape == (n, 7) and preds[b]["pred_scores"].shape == (n,) and n <= 500
        assert torch.equal(preds[b]["pred_labels"], roi_labels[b][roi_labels[b] != 0])
        assert bool(torch.isfinite(preds[b]["pred_boxes"]).all()) and bool(((preds[b]["pred_scores"] > 0) & (preds[b]["pred_scores"] <= 1)).all())
    # the second stage again: the head on the CPU (numpy pooling, torch GNN), same RoIs
    head_cpu = copy.deepcopy(net.roi_head).cpu().eval()
    with torch.no_grad():
        bd2 = head_cpu({"points": points.cpu(), "batch_size": B, "rois": rois.cpu(), "roi_scores": roi_scores.cpu(),
                        "roi_labels": roi_labels.cpu(), "has_class_labels": True, "cls_preds_normalized": True})
        preds2, _ = net.post_processing(bd2)
    # the pooled points themselves: HIP against the numpy statement, exactly
    r = net.roi_head.pc_range
    with torch.no_grad():
        idx_g, num_g, feats_g, _ = net.roi_head.roilocal_dfvs_pool3d_layer.pool(points, rois[..., :7].contiguous(), range_xy=[r[0], r[1], r[3], r[4]])
        idx_c, num_c, feats_c, _ = head_cpu.roilocal_dfvs_pool3d_layer.pool(points.cpu(), rois[..., :7].cpu(), range_xy=[r[0], r[1], r[3], r[4]])
    print("pooled points per RoI", num_g[roi_labels != 0].tolist()[:80])
    assert int((num_g[roi_labels != 0] >= 8).sum()) >= 12 and int(num_g.sum()) >= 400
    same = torch.equal(num_g.cpu(), num_c) and torch.equal(idx_g.cpu(), idx_c)
    print("pooling identical:", same, "feature deviation", float((feats_g.cpu() - feats_c).abs().max()))
    box_dev = max(float((preds[b]["pred_boxes"].cpu() - preds2[b]["pred_boxes"]).abs().max()) for b in range(B))
    score_dev = max(float((preds[b]["pred_scores"].cpu() - preds2[b]["pred_scores"]).abs().max()) for b in range(B))
    moved = max(float((preds[b]["pred_boxes"] - rois[b][roi_labels[b] != 0][:, :7]).abs().max()) for b in range(B))
    print(f"GPU-vs-CPU second stage: boxes {box_dev:.3e} scores {score_dev:.3e}; refinement moves boxes by up to {moved:.3f}")
    assert same
    assert moved > 1e-2
    for b in range(B):
        assert torch.equal(preds[b]["pred_labels"].cpu(), preds2[b]["pred_labels"])
    assert box_dev <= 4 * MEASURED_BOX_DEV and score_dev <= 4 * MEASURED_SCORE_DEV
