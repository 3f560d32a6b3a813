"""CPU: the anchor head of the shipped KITTI fine-tune config (PointPillar + AnchorHeadSingle) - registry, state dict, refusals,
and the op-by-op torch path against the golden captured from the UNMODIFIED reference head (tests/golden/make_golden_anchor_head.py).
Bound: the project's fp32 parity bound, 1e-4 relative; labels, matched boxes and direction bins must agree exactly."""
import copy
import logging
import os

import numpy as np
import pytest
import torch

from gdmae_hip import configs
from helpers import GOLDEN, assert_sampled_close, seeded_head_state

RTOL = 1e-4


def golden():
    return dict(np.load(os.path.join(GOLDEN, "anchor_head_b2.npz")))


def build_head(cfg=None):
    from pcdet.models.dense_heads import AnchorHeadSingle
    ds = configs.SyntheticDatasetInfo(**configs.KITTI)
    head = AnchorHeadSingle(model_cfg=cfg if cfg is not None else configs.anchor_head_cfg(), input_channels=128, num_class=3,
                            class_names=ds.class_names, grid_size=ds.grid_size, point_cloud_range=ds.point_cloud_range,
                            predict_boxes_when_training=False, voxel_size=ds.voxel_size, backbone_channels=None)

    class Wrap(torch.nn.Module):
        def __init__(s):
            super().__init__()
            s.dense_head = head
    return Wrap()


def seeded(z):
    net = build_head()
    net.load_state_dict(seeded_head_state(net, int(z["seed"])), strict=False)
    sf = torch.randn(int(z["batch_size"]), 128, 248, 216, generator=torch.Generator().manual_seed(int(z["seed"]) + 1)) * 0.5
    return net, sf


def check_targets(z, t, rtol=RTOL):
    """labels / matched rows / direction bins identical to the golden, regression targets within rtol."""
    labels = t['box_cls_labels'].cpu()
    pos, ign = (labels > 0).nonzero().numpy(), (labels < 0).nonzero().numpy()
    assert np.array_equal(pos, z["pos_index"]) and np.array_equal(ign, z["ign_index"])
    assert int((labels == 0).sum()) == int(z["n_background"])
    p0, p1 = torch.from_numpy(pos[:, 0]), torch.from_numpy(pos[:, 1])
    assert np.array_equal(labels[p0, p1].numpy(), z["pos_label"])
    assert np.array_equal(t['gt_ids'].cpu()[p0, p1].numpy(), z["pos_gt_row"])
    reg = t['box_reg_targets'].cpu()
    err = np.abs(reg[p0, p1].numpy() - z["pos_reg_targets"]).max() / np.abs(z["pos_reg_targets"]).max()
    print("regression targets: rel-max-err %.3e over %d positives" % (err, pos.shape[0]))
    assert err <= rtol
    assert int((reg.abs().sum(-1) != 0).sum()) <= pos.shape[0]          # zero elsewhere
    return p0, p1


def test_registry_state_dict_and_refusals():
    from pcdet.models import build_network, dense_heads, detectors
    assert "PointPillar" in detectors.__all__ and "AnchorHeadSingle" in dense_heads.__all__
    z = golden()
    cfg, ds = configs.kitti_finetune_cfg()
    assert tuple(int(v) for v in ds.grid_size) == (216, 248, 1)
    det = build_network(cfg, 3, ds, logging.getLogger("t"))
    assert type(det).__name__ == "PointPillar"
    assert [type(m).__name__ for m in det.module_list] == ["DynVFE", "SPTBackbone", "SSTBEVBackbone", "AnchorHeadSingle"]
    ours = {"dense_head." + k: tuple(v.shape) for k, v in det.dense_head.state_dict().items()}
    ref = {str(k): tuple(int(x) for x in s if x) for k, s in zip(z["state_keys"], z["state_shapes"])}
    assert ours == ref
    assert ours["dense_head.conv_cls.weight"] == (18, 128, 1, 1) and ours["dense_head.conv_box.weight"] == (42, 128, 1, 1)
    assert ours["dense_head.conv_dir_cls.weight"] == (12, 128, 1, 1)
    head = det.dense_head
    assert [tuple(a.shape) for a in head.anchors] == [(1, 248, 216, 1, 2, 7)] * 3 and head.num_anchors_per_location == 6
    assert abs(float(head.conv_cls.bias[0]) + np.log(99.0)) < 1e-6 and float(head.conv_box.weight.std()) < 2e-3     # init_weights

    def bad(edit):
        c = copy.deepcopy(configs.anchor_head_cfg())
        edit(c)
        with pytest.raises(NotImplementedError):
            build_head(c)
    bad(lambda c: c.TARGET_ASSIGNER_CONFIG.__setitem__('NAME', 'ATSS'))
    bad(lambda c: c.__setitem__('USE_MULTIHEAD', True))
    bad(lambda c: c.TARGET_ASSIGNER_CONFIG.__setitem__('POS_FRACTION', 0.5))
    bad(lambda c: c.TARGET_ASSIGNER_CONFIG.__setitem__('MATCH_HEIGHT', True))
    bad(lambda c: c.TARGET_ASSIGNER_CONFIG.__setitem__('NORM_BY_NUM_EXAMPLES', True))
    bad(lambda c: c.TARGET_ASSIGNER_CONFIG.__setitem__('BOX_CODER', 'PreviousResidualDecoder'))
    bad(lambda c: c.TARGET_ASSIGNER_CONFIG.__setitem__('BOX_CODER_CONFIG', {'encode_angle_by_sincos': True}))
    bad(lambda c: c.LOSS_CONFIG.__setitem__('REG_LOSS_TYPE', 'WeightedL1Loss'))
    # post_processing: the branches outside the shipped config raise by name
    bd = {'batch_size': 1, 'batch_cls_preds': torch.zeros(1, 4, 3), 'batch_box_preds': torch.zeros(1, 4, 7), 'cls_preds_normalized': False}
    with pytest.raises(NotImplementedError):
        det.post_processing({**bd, 'has_class_labels': True})
    with pytest.raises(NotImplementedError):
        det.post_processing({**bd, 'batch_cls_preds': [torch.zeros(1, 4, 3)]})
    c2 = copy.deepcopy(cfg)
    c2.POST_PROCESSING.NMS_CONFIG['MULTI_CLASSES_NMS'] = True
    with pytest.raises(NotImplementedError):
        build_network(c2, 3, ds, logging.getLogger("t")).post_processing(bd)
    from gdmae_hip import inference
    with pytest.raises(NotImplementedError, match="CenterPoint"):
        inference.compile_detector(det)


def test_torch_path_matches_reference_golden():
    z = golden()
    net, sf = seeded(z)
    head = net.dense_head
    sf.requires_grad_(True)
    gt = torch.from_numpy(z["gt_boxes"])
    assert not bool((gt[1, :, 7] == 3).any()) and bool((gt[0, :, 7] == 3).any())       # one sample without a Cyclist
    net.train()
    head({"spatial_features_2d": sf, "gt_boxes": gt.clone(), "batch_size": 2})
    fr = head.forward_ret_dict
    p0, p1 = check_targets(z, fr)
    bins = head.direction_bins_torch(fr['box_reg_targets'])
    assert np.array_equal(bins[p0, p1].numpy(), z["pos_dir_bin"])
    loss, tb = head.get_loss()
    assert set(tb) == {"rpn_loss_cls", "rpn_loss_loc", "rpn_loss_dir"}
    for name, v in (("loss", loss), ("loss_cls", tb["rpn_loss_cls"]), ("loss_loc", tb["rpn_loss_loc"]), ("loss_dir", tb["rpn_loss_dir"])):
        rel = abs(float(v) - float(z[name])) / abs(float(z[name]))
        print("%s %.7g golden %.7g rel %.2e" % (name, float(v), float(z[name]), rel))
        assert rel <= RTOL, name
    loss.backward()
    for k in ("cls_preds", "box_preds", "dir_cls_preds"):
        assert_sampled_close(fr[k], z[k + "_s"], z[k + "_c"], RTOL, k)
    assert_sampled_close(sf.grad, z["sf_grad_s"], z["sf_grad_c"], RTOL, "input gradient")
    gp = dict(net.named_parameters())
    for k, ref in zip(z["param_names"], z["grad_norm"]):
        got = float(gp[str(k)].grad.double().norm())
        assert abs(got - ref) <= RTOL * abs(ref), (k, got, ref)
    net.eval()
    with torch.no_grad():
        dd = head({"spatial_features_2d": sf.detach(), "batch_size": 2})
    assert dd['cls_preds_normalized'] is False
    for k in ("batch_cls_preds", "batch_box_preds"):
        assert tuple(dd[k].shape) == tuple(z[k + "_shape"])
        s, c = z[k + "_s"], z[k + "_c"]
        from helpers import sample
        got = sample(dd[k])[0]
        print("%s: rel-max-err %.3e" % (k, np.abs(got - s).max() / np.abs(s).max()))
        assert_sampled_close(dd[k], s, c, RTOL, k)
    assert tuple(dd["batch_cls_preds"].shape) == (2, 321408, 3) and tuple(dd["batch_box_preds"].shape) == (2, 321408, 7)
    # the torch path alone selects at least 100 boxes per sample at the config's score threshold (the GPU tests rely on it)
    sel = (torch.sigmoid(dd["batch_cls_preds"]).max(-1)[0] >= 0.3).sum(1)
    assert int(sel.min()) >= 100, sel


def test_anchor_order_is_class_major_then_rotation():
    head = build_head().dense_head
    a = head.all_anchors().view(248, 216, 6, 7)
    assert torch.equal(a[3, 5, :, 3], torch.tensor([3.9, 3.9, 0.8, 0.8, 1.76, 1.76]))
    assert torch.equal(a[3, 5, :, 6], torch.tensor([0, 1.57, 0, 1.57, 0, 1.57]))
    assert "anchors_0" not in head.state_dict() and head.anchors[0].device.type == "cpu"


def test_abi_declares_binds_and_exports_the_anchor_entry_points():
    import re
    from gdmae_hip import lib as L
    names = ["gdmae_anchor_targets_workspace_bytes", "gdmae_anchor_targets", "gdmae_anchor_loss_rows", "gdmae_anchor_loss_fwd",
             "gdmae_anchor_loss_bwd", "gdmae_anchor_decode", "gdmae_anchor_select"]
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "gdmae_hip.h")).read()
    lib = L.load()
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, header) and n in L.SIGNATURES and hasattr(lib, n), n
    assert lib.gdmae_anchor_targets_workspace_bytes(2, 3, 24) >= 2 * 3 * 24 * 28 and lib.gdmae_anchor_loss_rows() == 1024
