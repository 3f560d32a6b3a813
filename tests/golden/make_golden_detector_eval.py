"""Evaluation-mode golden of the fine-tune detector: the reference's DynVFE -> SPTBackbone -> SSTBEVBackbone -> CenterHead
(unmodified, through ref_harness, the module chain and seeded weights of make_golden_detector.py) with BatchNorm RUNNING statistics.

1. one train-mode forward on seeded batch A with every BatchNorm's momentum set to 1.0: the running statistics become that batch's
   statistics (with the shipped momentum 0.01 they would stay within 1 % of (0, 1) and a test could not tell folded from unfolded);
2. .eval(), one forward on a DIFFERENT seeded batch B up to the head maps (the reference's box decoding needs its CUDA NMS extension:
   the golden ends where detector_kitti_b2.npz ends);
3. stored: batch B's points, every BatchNorm buffer, voxel_coords, samples (make_golden.sample) of the pillar features, both dense maps
   and every head map, and the head maps' values at the per-class top-64 heat-map cells.
Build container only (reads /root/reference)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd"), HERE, os.path.join(REPO, "tests")]
import make_golden as mg  # noqa: E402
import make_golden_head as mh  # noqa: E402

rh, configs, synth, orc = mg.rh, mg.configs, mg.synth, mg.orc
HEAD_MAPS = ("hm", "center", "center_z", "dim", "rot")


def main():
    mh.install_head_stubs()
    from head_seed import seeded_head_state
    seed, seed_b, B, F = 41, 43, 2, 4
    y3 = rh.load_yaml_cfg("cfgs/kitti_models/gd_mae.yaml").MODEL
    y2 = rh.load_yaml_cfg("cfgs/waymo_models/gd_mae.yaml").MODEL
    ds = configs.SyntheticDatasetInfo(**configs.KITTI)
    class_names = ['Vehicle', 'Pedestrian', 'Cyclist']
    pcr = np.asarray(ds.point_cloud_range, dtype=np.float32)
    skw = dict(beams=24, azimuths=300, extra=500, features=F)
    pts_a = torch.from_numpy(synth.synth_batch(seed, B, ds.point_cloud_range, **skw))
    pts_b = torch.from_numpy(synth.synth_batch(seed_b, B, ds.point_cloud_range, **skw))
    dyn = rh.ref("pcdet.models.backbones_3d.vfe.dyn_vfe")
    spt = rh.ref("pcdet.models.backbones_3d.spt_backbone")
    bev = rh.ref("pcdet.models.backbones_2d.sst_bev_backbone")
    ch = rh.ref("pcdet.models.dense_heads.center_head")
    vfe = dyn.DynVFE(model_cfg=y3.VFE, num_point_features=F, voxel_size=ds.voxel_size, point_cloud_range=ds.point_cloud_range,
                     grid_size=ds.grid_size)
    bb = spt.SPTBackbone(model_cfg=y3.BACKBONE_3D, input_channels=vfe.get_output_feature_dim(), grid_size=ds.grid_size,
                         voxel_size=ds.voxel_size, point_cloud_range=ds.point_cloud_range)
    b2d = bev.SSTBEVBackbone(model_cfg=y2.BACKBONE_2D, input_channels=128)
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        head = ch.CenterHead(model_cfg=y2.DENSE_HEAD, input_channels=b2d.num_bev_features, num_class=3, class_names=class_names,
                             grid_size=np.asarray(ds.grid_size), point_cloud_range=pcr, voxel_size=list(ds.voxel_size),
                             predict_boxes_when_training=False)
    finally:
        torch.Tensor.cuda = real_cuda

    class Net(torch.nn.Module):
        def __init__(s):
            super().__init__()
            s.vfe, s.backbone_3d, s.backbone_2d, s.dense_head = vfe, bb, b2d, head

    class Front(torch.nn.Module):
        def __init__(s):
            super().__init__()
            s.vfe, s.backbone_3d = vfe, bb

    class Back(torch.nn.Module):
        def __init__(s):
            super().__init__()
            s.backbone_2d, s.dense_head = b2d, head
    net, front, back = Net(), Front(), Back()
    shapes = {k: tuple(v.shape) for k, v in front.named_parameters()}
    front.load_state_dict(orc.seeded_state_dict(shapes, seed=seed), strict=False)
    back.load_state_dict(seeded_head_state(back, seed), strict=False)
    bns = {k: m for k, m in net.named_modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)}
    for m in bns.values():
        m.momentum = 1.0
    # 1. train-mode forward on batch A: running statistics := batch statistics
    net.train()
    with torch.no_grad():
        bd = bb(vfe({"points": pts_a.clone(), "batch_size": B}))
        bd["gt_boxes"] = torch.from_numpy(mh.synth_boxes(np.random.default_rng(seed), B, 24, pcr, 3))
        head(b2d(bd))
    # 2. eval forward on batch B, up to the head maps
    net.eval()
    with torch.no_grad():
        bd = b2d(bb(vfe({"points": pts_b.clone(), "batch_size": B})))
        x = head.shared_conv(bd["spatial_features_2d"])
        pd = head.heads_list[0](x)
    z = {"seed": np.int64(seed), "batch_size": np.int64(B), "num_point_features": np.int64(F), "points": pts_b.numpy(),
         "voxel_coords": bd["voxel_coords"].numpy().astype(np.int32),
         "front_names": np.array(sorted(shapes)),
         "front_shapes": np.array([list(shapes[k]) + [0] * (4 - len(shapes[k])) for k in sorted(shapes)])}
    for k, m in bns.items():
        z["bn/" + k + ".running_mean"] = m.running_mean.numpy().astype(np.float32)
        z["bn/" + k + ".running_var"] = m.running_var.numpy().astype(np.float32)
    z["pillar_features_s"], z["pillar_features_c"] = mg.sample(bd["pillar_features"])
    z["spatial_features_s"], z["spatial_features_c"] = mg.sample(bd["spatial_features"])
    z["spatial_features_2d_s"], z["spatial_features_2d_c"] = mg.sample(bd["spatial_features_2d"])
    hm = pd["hm"]
    Bn, C, H, W = hm.shape
    top = torch.topk(hm.reshape(Bn, C, H * W), 64, dim=2).indices          # (B, C, 64) cells
    z["top_cells"] = top.numpy().astype(np.int32)
    for name in HEAD_MAPS:
        m = pd[name]
        z[name + "_s"], z[name + "_c"] = mg.sample(m)
        flat = m.reshape(Bn, m.shape[1], H * W)
        z[name + "_top"] = torch.stack([flat[b][:, top[b].reshape(-1)] for b in range(Bn)]).numpy().astype(np.float32)   # (B, c, C * 64)
    # decoder background: an empty site of branch i holds relu(b_i); the test needs channels where that is not zero
    sf_dense_share = []
    for i, blk in enumerate(bb.deblocks):
        bn = blk[1]
        a = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        b = bn.bias.double() - a * bn.running_mean.double()
        sf_dense_share.append(float((b > 0).double().mean()))
    z["deblock_positive_bias_share"] = np.array(sf_dense_share)
    n_sites = B * int(ds.grid_size[0]) * int(ds.grid_size[1])
    empty_share = 1.0 - bd["voxel_coords"].shape[0] / n_sites
    assert min(sf_dense_share) > 0.05 and empty_share > 0.5, (sf_dense_share, empty_share)
    path = os.path.join(HERE, "detector_eval_kitti_b2.npz")
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB; pillars", bd["voxel_coords"].shape[0],
          "share of deblock channels with b_i > 0 per branch", sf_dense_share, "share of empty full-resolution sites %.3f" % empty_share,
          "running_var range", min(float(m.running_var.min()) for m in bns.values()), max(float(m.running_var.max()) for m in bns.values()))


if __name__ == "__main__":
    main()
