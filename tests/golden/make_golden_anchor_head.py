"""Golden for the anchor head of the shipped KITTI fine-tune config: the reference's AnchorHeadSingle
(pcdet/models/dense_heads/anchor_head_single.py:7-75 on anchor_head_template.py:11-266, AxisAlignedTargetAssigner, ResidualCoder,
the focal / smooth-L1 / direction losses of pcdet/utils/loss_utils.py) run UNMODIFIED on a seeded BEV map and seeded ground-truth
boxes: forward + target assignment + get_loss + backward in training mode, and the evaluation-mode batch_cls_preds /
batch_box_preds.  Build container only (reads the reference tree); holds none of its text.

Stand-ins as in make_golden_head.py (``install_head_stubs``, ``Tensor.cuda`` as the identity while the head is constructed: the
reference moves its anchors and loss code weights to the GPU in __init__).  The reference's NMS is a CUDA extension, so final
boxes are not part of this fixture.

The matched ground-truth row of a positive anchor is a local of the reference's assign_targets_single; it is recovered here from
what the reference returns: the regression target decoded against the anchor is the matched box, the nearest row of gt_boxes[b]
(distance < 1e-3 asserted) is its index."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd"), HERE]
import make_golden as mg  # noqa: E402
import make_golden_head as mgh  # noqa: E402

rh, configs = mg.rh, mg.configs

SEED, BOX_SEED, B, N_MAX = 41, 3, 2, 24


def golden_boxes():
    """synth_boxes(rng(3), B = 2, 24 rows, KITTI range, 3 classes); sample 1 holds no Cyclist (its class-3 boxes become Pedestrians)."""
    pcr = np.array(configs.KITTI['point_cloud_range'], dtype=np.float32)
    gt = mgh.synth_boxes(np.random.default_rng(BOX_SEED), B, N_MAX, pcr, 3)
    gt[1, gt[1, :, 7] == 3, 7] = 2
    return gt


def main():
    mgh.install_head_stubs()
    ycfg = rh.load_yaml_cfg("cfgs/kitti_models/gd_mae.yaml")
    mc = ycfg.MODEL
    ours, ds = configs.kitti_finetune_cfg()
    assert mg.to_plain(mc) == mg.to_plain(ours), "MODEL section drifted from the reference yaml"
    assert mg.to_plain(mc.DENSE_HEAD) == mg.to_plain(configs.anchor_head_cfg())
    assert list(ycfg.DATA_CONFIG.POINT_CLOUD_RANGE) == list(configs.KITTI['point_cloud_range'])
    assert [list(p.VOXEL_SIZE) for p in ycfg.DATA_CONFIG.DATA_PROCESSOR if p.NAME == 'calculate_grid_size'] == [configs.KITTI['voxel_size']]
    assert list(ycfg.CLASS_NAMES) == configs.KITTI['class_names']
    ah = rh.ref("pcdet.models.dense_heads.anchor_head_single")
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        head = ah.AnchorHeadSingle(model_cfg=mc.DENSE_HEAD, input_channels=128, num_class=3, class_names=ds.class_names, grid_size=ds.grid_size,
                                   point_cloud_range=ds.point_cloud_range, predict_boxes_when_training=False)
    finally:
        torch.Tensor.cuda = real_cuda

    class Wrap(torch.nn.Module):
        def __init__(s):
            super().__init__()
            s.dense_head = head
    net = Wrap()
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    from head_seed import seeded_head_state
    net.load_state_dict(seeded_head_state(net, SEED), strict=False)
    H, W = int(ds.grid_size[1]), int(ds.grid_size[0])
    sf = torch.randn(B, 128, H, W, generator=torch.Generator().manual_seed(SEED + 1)) * 0.5
    sf.requires_grad_(True)
    gt = torch.from_numpy(golden_boxes())
    net.train()
    head({"spatial_features_2d": sf, "gt_boxes": gt.clone(), "batch_size": B})
    fr = head.forward_ret_dict
    loss, tb = head.get_loss()
    loss.backward()
    labels, reg = fr['box_cls_labels'], fr['box_reg_targets']
    anchors = torch.cat(head.anchors, dim=-3).view(-1, 7)
    pos, ign = (labels > 0).nonzero(), (labels < 0).nonzero()
    pos_reg = reg[pos[:, 0], pos[:, 1]]
    dec = head.box_coder.decode_torch(pos_reg, anchors[pos[:, 1]])
    d = (dec[:, None, :] - gt[pos[:, 0], :, :7]).abs().sum(-1)
    assert float(d.min(dim=1)[0].max()) < 1e-3
    bins = head.get_direction_target(anchors.view(1, -1, 7).repeat(B, 1, 1), reg, one_hot=False, dir_offset=mc.DENSE_HEAD.DIR_OFFSET,
                                     num_bins=mc.DENSE_HEAD.NUM_DIR_BINS)
    names = sorted(k for k, _ in net.named_parameters())
    gp = dict(net.named_parameters())
    sd = net.state_dict()
    z = {"seed": np.int64(SEED), "box_seed": np.int64(BOX_SEED), "batch_size": np.int64(B), "gt_boxes": gt.numpy(),
         "loss": np.float64(float(loss)), "loss_cls": np.float64(tb['rpn_loss_cls']), "loss_loc": np.float64(tb['rpn_loss_loc']),
         "loss_dir": np.float64(tb['rpn_loss_dir']),
         "pos_index": pos.numpy().astype(np.int32), "pos_label": labels[pos[:, 0], pos[:, 1]].numpy().astype(np.int32),
         "ign_index": ign.numpy().astype(np.int32), "n_background": np.int64(int((labels == 0).sum())),
         "pos_gt_row": d.argmin(dim=1).numpy().astype(np.int32), "pos_reg_targets": pos_reg.numpy(),
         "pos_dir_bin": bins[pos[:, 0], pos[:, 1]].numpy().astype(np.int32),
         "param_names": np.array(names), "grad_norm": np.array([float(gp[k].grad.double().norm()) for k in names]),
         "state_keys": np.array(sorted(sd.keys())),
         "state_shapes": np.array([list(sd[k].shape) + [0] * (4 - sd[k].dim()) for k in sorted(sd.keys())])}
    z["sf_grad_s"], z["sf_grad_c"] = mg.sample(sf.grad)
    for k in ("cls_preds", "box_preds", "dir_cls_preds"):
        z[f"{k}_s"], z[f"{k}_c"] = mg.sample(fr[k])
    net.eval()
    with torch.no_grad():
        dd = head({"spatial_features_2d": sf.detach(), "batch_size": B})
    assert dd['cls_preds_normalized'] is False
    for k in ("batch_cls_preds", "batch_box_preds"):
        z[f"{k}_s"], z[f"{k}_c"] = mg.sample(dd[k])
        z[f"{k}_shape"] = np.array(dd[k].shape)
    path = os.path.join(HERE, "anchor_head_b2.npz")
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB  loss", float(loss), tb, "positives", pos.shape[0], "ignored", ign.shape[0],
          "background", int((labels == 0).sum()))


if __name__ == "__main__":
    main()
