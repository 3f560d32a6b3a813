"""Golden for the second stage of the shipped two-stage config (tools/cfgs/waymo_models/gd_mae_ts.yaml): the reference's
GraphRCNNHead (pcdet/models/roi_heads/graphrcnn_head.py:12-302 on roi_head_template.py:11-254) built UNMODIFIED from the yaml
section, with seeded weights and BatchNorm running statistics (tests/roi_head_seed.py: no weights are stored), run in eval mode
on the CPU from seeded pooled tensors to rcnn_cls / rcnn_reg / batch_cls_preds / batch_box_preds.  Build container only (reads
the reference tree); holds none of its text.

Stand-ins: what the reference head imports but cannot load here - the ``patch_ops_cuda`` extension and the image fusion layer
(``PointSample``) - are empty stubs; ``roipool3d_gpu`` is replaced by the seeded pooled tensors (the pooling itself is the
subject of tests/test_roi_pool_*.py); ``Tensor.cuda`` is the identity while the head is constructed (its loss code weights).

B = 2, M = 6, K = 256.  RoI kinds: one empty RoI (num = 0), one RoI with num = 40 and repeat-padded slots, RoIs with distinct
points.  The generator asserts that the gap between every point's 8th and 9th neighbour distance exceeds 1e-4 relative (or that
the two are copies of one point), so that another matmul rounding cannot flip a neighbour."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd"), HERE, os.path.join(REPO, "tests")]
import make_golden as mg  # noqa: E402
import make_golden_head as mgh  # noqa: E402

rh, configs = mg.rh, mg.configs

SEED, B, M, K, C = 51, 2, 6, 256, 2
EMPTY, SPARSE, SPARSE_NUM = (0, 4), (1, 1), 40


def golden_inputs():
    """rois (B, M, 7), roi_scores (B, M) in (0, 1), roi_labels (B, M) 1..3, feats_local (B M, K, 3 + C + 6), pooled_num (B M)"""
    rng = np.random.default_rng(SEED)
    rois = np.zeros((B, M, 7), np.float32)
    rois[..., 0:2] = rng.uniform(-60, 60, (B, M, 2))
    rois[..., 2] = rng.uniform(0, 1.5, (B, M))
    rois[..., 3:6] = rng.uniform([1.0, 0.8, 1.2], [5.0, 2.2, 2.2], (B, M, 3))
    rois[..., 6] = rng.uniform(-np.pi, np.pi, (B, M))
    scores = rng.uniform(0.1, 0.95, (B, M)).astype(np.float32)
    labels = rng.integers(1, 4, (B, M)).astype(np.int64)
    feats = np.zeros((B * M, K, 3 + C + 6), np.float32)
    num = np.full((B, M), K, np.int32)
    for b in range(B):
        for r in range(M):
            o = b * M + r
            half = rois[b, r, 3:6] / 2
            n = K
            if (b, r) == EMPTY:
                num[b, r] = 0
                feats[o] = rng.normal(size=(K, 3 + C + 6))          # whatever the pooling left: the head zeroes it
                continue
            if (b, r) == SPARSE:
                n = num[b, r] = SPARSE_NUM
            feats[o, :n, :3] = rng.uniform(-1, 1, (n, 3)) * (half + 0.4)
            for _ in range(100):                                    # redraw the points whose 8th / 9th neighbours are too close to call
                bad = ~neighbour_gaps_ok(feats[o, :n, :3])
                if not bad.any():
                    break
                feats[o, :n, :3][bad] = rng.uniform(-1, 1, (int(bad.sum()), 3)) * (half + 0.4)
            feats[o, :n, 3:3 + C] = rng.uniform(0, 1, (n, C))
            feats[o, n:] = feats[o, np.arange(n, K) % n]
            feats[o, :, 3 + C:3 + C + 3] = -half
            feats[o, :, 3 + C + 3:] = half
    return rois, scores, labels, feats, num.reshape(-1)


def neighbour_gaps_ok(xyz, k=8, rel=2e-4):
    """per point: the gap between its k-th and (k + 1)-th neighbour distance is > rel (relative), or both are copies of one point"""
    x = xyz.astype(np.float64)
    d = ((x[:, None] - x[None]) ** 2).sum(-1)
    order = np.argsort(d, axis=1, kind='stable')
    dk, dk1 = np.take_along_axis(d, order[:, k - 1:k], 1)[:, 0], np.take_along_axis(d, order[:, k:k + 1], 1)[:, 0]
    same = (x[order[:, k - 1]] == x[order[:, k]]).all(-1)
    return same | ((dk1 - dk) / np.maximum(dk1, 1e-12) > rel)


def assert_neighbour_gaps(feats, num):
    for o in range(feats.shape[0]):
        assert num[o] == 0 or neighbour_gaps_ok(feats[o, :, :3], rel=1e-4).all(), o


def install_roi_head_stubs():
    mgh.install_head_stubs()
    for name in ["pcdet.models.roi_heads", "pcdet.models.roi_heads.target_assigner", "pcdet.ops.patch_ops"]:
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = [os.path.join(rh.REF, *name.split("."))]
            sys.modules[name] = m
    cuda = types.ModuleType("pcdet.ops.patch_ops.patch_ops_cuda")
    sys.modules["pcdet.ops.patch_ops.patch_ops_cuda"] = cuda
    sys.modules["pcdet.ops.patch_ops"].patch_ops_cuda = cuda
    fl = types.ModuleType("pcdet.models.fusion_layers")
    fl.PointSample = type("PointSample", (torch.nn.Module,), {})
    sys.modules["pcdet.models.fusion_layers"] = fl


def main():
    install_roi_head_stubs()
    ycfg = rh.load_yaml_cfg("cfgs/waymo_models/gd_mae_ts.yaml")
    mc = ycfg.MODEL
    ours, ds = configs.waymo_two_stage_cfg()
    assert mg.to_plain(mc) == mg.to_plain(ours), "MODEL section drifted from the reference yaml"
    assert mg.to_plain(mc.ROI_HEAD) == mg.to_plain(configs.graphrcnn_head_cfg())
    assert list(ycfg.DATA_CONFIG.POINT_CLOUD_RANGE) == list(configs.WAYMO['point_cloud_range'])
    assert list(ycfg.CLASS_NAMES) == configs.WAYMO['class_names']
    gh = rh.ref("pcdet.models.roi_heads.graphrcnn_head")
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        head = gh.GraphRCNNHead(input_channels=128, model_cfg=mc.ROI_HEAD, point_cloud_range=ds.point_cloud_range,
                                voxel_size=ds.voxel_size, backbone_channels=None, num_class=1)
    finally:
        torch.Tensor.cuda = real_cuda

    class Wrap(torch.nn.Module):
        def __init__(s):
            super().__init__()
            s.roi_head = head
    net = Wrap()
    from roi_head_seed import seeded_roi_head_state
    missing = net.load_state_dict(seeded_roi_head_state(net, SEED), strict=False)
    assert all(k.endswith("num_batches_tracked") for k in missing.missing_keys), missing
    rois, scores, labels, feats, num = golden_inputs()
    assert_neighbour_gaps(feats, num)
    net.eval()
    head.roipool3d_gpu = lambda bd: (torch.from_numpy(feats.copy()), torch.from_numpy(feats[..., :3].copy()), torch.from_numpy(num.copy()))
    caught = {}
    head.cls_layers.register_forward_hook(lambda m, i, o: caught.__setitem__('cls', o))
    head.reg_layers.register_forward_hook(lambda m, i, o: caught.__setitem__('reg', o))
    with torch.no_grad():
        bd = head({'batch_size': B, 'rois': torch.from_numpy(rois.copy()), 'roi_scores': torch.from_numpy(scores.copy()),
                   'roi_labels': torch.from_numpy(labels.copy()), 'cls_preds_normalized': True, 'has_class_labels': True})
    sd = net.state_dict()
    keys = sorted(sd.keys())
    z = {"seed": np.int64(SEED), "rois": rois, "roi_scores": scores, "roi_labels": labels, "feats_local": feats, "pooled_num": num,
         "rcnn_cls": caught['cls'].permute(0, 2, 1).reshape(B * M, -1).numpy(), "rcnn_reg": caught['reg'].permute(0, 2, 1).reshape(B * M, -1).numpy(),
         "batch_cls_preds": bd['batch_cls_preds'].numpy(), "batch_box_preds": bd['batch_box_preds'].numpy(),
         "state_keys": np.array(keys), "state_shapes": np.array([list(sd[k].shape) + [0] * (4 - sd[k].dim()) for k in keys])}
    assert bd['cls_preds_normalized'] is True and np.isfinite(z["batch_box_preds"]).all()
    path = os.path.join(HERE, "roi_head_b2.npz")
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB", "scores", z["batch_cls_preds"].reshape(-1).round(3).tolist())
    print("reg", np.abs(z["rcnn_reg"]).max(), "cls", z["rcnn_cls"].reshape(-1).round(3).tolist())


if __name__ == "__main__":
    main()
