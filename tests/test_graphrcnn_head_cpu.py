"""CPU: the two-stage detector of the shipped gd_mae_ts config builds, its RoI head has the reference's state_dict and
reproduces the reference head's outputs (tests/golden/roi_head_b2.npz), ``post_processing`` has the ``NMS: False`` branch,
and what is not built raises by name."""
import copy
import logging
import os

import numpy as np
import pytest
import torch

from gdmae_hip import configs
from pcdet.models import build_network
from roi_head_seed import seeded_roi_head_state

HERE = os.path.dirname(os.path.abspath(__file__))


def golden():
    return np.load(os.path.join(HERE, "golden", "roi_head_b2.npz"))


@pytest.fixture(scope="module")
def detector():
    cfg, ds = configs.waymo_two_stage_cfg()
    return build_network(cfg, 3, ds, logging.getLogger("t")).eval()


def seed_roi_head(det, seed):
    class Wrap(torch.nn.Module):
        def __init__(s):
            super().__init__()
            s.roi_head = det.roi_head
    w = Wrap()
    missing = w.load_state_dict(seeded_roi_head_state(w, seed), strict=False)
    assert all(k.endswith("num_batches_tracked") for k in missing.missing_keys)


def test_build_registry_and_state_dict(detector):
    from pcdet.models import detectors, roi_heads
    assert "GraphRCNN" in detectors.__all__ and "GraphRCNNHead" in roi_heads.__all__
    assert type(detector).__name__ == "GraphRCNN"
    assert [type(m).__name__ for m in detector.module_list] == ["DynVFE", "SPTBackbone", "SSTBEVBackbone", "CenterHead", "GraphRCNNHead"]
    assert detector.dense_head.predict_boxes_when_training
    z = golden()
    ours = {"roi_head." + k: tuple(v.shape) for k, v in detector.roi_head.state_dict().items()}
    ref = {str(k): tuple(int(x) for x in s if x) for k, s in zip(z["state_keys"], z["state_shapes"])}
    assert ours == ref
    for k in ("attn_gnn_layer.edge_layes.0.0.weight", "attn_gnn_layer.calib.3.bias", "attn_gnn_layer.expansion.0.weight",
              "attn_gnn_layer.reduction.1.running_var", "attn_gnn_layer.shortcut.norm2.weight", "shared_fc_layer.0.weight",
              "cls_layers.bias", "reg_layers.weight"):
        assert "roi_head." + k in ours, k
    assert ours["roi_head.attn_gnn_layer.edge_layes.0.0.weight"] == (32, 22, 1, 1) and ours["roi_head.reg_layers.weight"] == (7, 256, 1)
    # xavier init, the reference's std for reg_layers, zero biases
    cfg, ds = configs.waymo_two_stage_cfg()
    torch.manual_seed(0)
    fresh = build_network(cfg, 3, ds, logging.getLogger("t")).roi_head
    assert float(fresh.reg_layers.weight.detach().std()) < 2e-3 and not fresh.reg_layers.bias.any() and not fresh.cls_layers.bias.any()
    w = fresh.shared_fc_layer[0].weight
    assert abs(float(w.detach().std()) - (2.0 / (256 + 256)) ** 0.5) < 0.1 * (2.0 / 512) ** 0.5
    # the config object is not consumed by building (the reference pops IN_DIM from it)
    assert cfg.ROI_HEAD.ATTN_GNN_CONFIG.IN_DIM == 11


def test_head_matches_the_reference_fixture(detector):
    """GNN -> shared layer -> heads -> decoded boxes and sqrt(sigmoid(cls) * roi_score) against the reference head on the same
    seeded weights and pooled tensors.  Measured deviation from the fixture on the CPU: 0 with the thread count the fixture was
    written with, and single-threaded (another GEMM blocking) 1.8e-6 on rcnn_cls, 1.7e-6 on rcnn_reg, 7.7e-6 on the boxes
    (one fp32 ulp of a 64 m coordinate) and 1.2e-7 on the scores; the bounds are 4 x these."""
    z = golden()
    seed_roi_head(detector, int(z["seed"]))
    head = detector.roi_head
    B, M = z["rois"].shape[:2]
    feats, num = torch.from_numpy(z["feats_local"]), torch.from_numpy(z["pooled_num"])
    assert B == 2 and M == 6 and feats.shape == (12, 256, 11) and int((num == 0).sum()) == 1 and int((num == 40).sum()) == 1
    head.roipool3d_gpu = lambda bd: (feats.clone(), feats[..., :3].clone(), num.clone())
    try:
        with torch.no_grad():
            f = feats * (num > 0)[:, None, None]
            cls, reg = head.heads(head.pooled_to_features(f, B, M), B, M)
            bd = head({'batch_size': B, 'rois': torch.from_numpy(z["rois"]), 'roi_scores': torch.from_numpy(z["roi_scores"]),
                       'roi_labels': torch.from_numpy(z["roi_labels"]), 'cls_preds_normalized': True, 'has_class_labels': True})
    finally:
        del head.roipool3d_gpu
    dev = {k: float(np.abs(v.numpy() - z[k]).max()) for k, v in
           (("rcnn_cls", cls), ("rcnn_reg", reg), ("batch_cls_preds", bd["batch_cls_preds"]), ("batch_box_preds", bd["batch_box_preds"]))}
    print("deviation from the fixture:", dev, "threads", torch.get_num_threads())
    assert dev["rcnn_cls"] <= 4 * 1.8e-6 and dev["rcnn_reg"] <= 4 * 1.7e-6
    assert dev["batch_box_preds"] <= 4 * 7.7e-6 and dev["batch_cls_preds"] <= 4 * 1.2e-7
    assert bd["cls_preds_normalized"] is True and bd["batch_cls_preds"].shape == (B, M, 1) and bd["batch_box_preds"].shape == (B, M, 7)


def test_post_processing_without_nms(detector):
    B, M = 2, 5
    g = torch.Generator().manual_seed(3)
    boxes = torch.rand(B, M, 7, generator=g) * 4 + 1
    cls = torch.rand(B, M, 1, generator=g)
    labels = torch.tensor([[1, 3, 2, 0, 0], [2, 2, 0, 1, 3]])
    gt = torch.zeros(B, 3, 8)
    gt[0, 0, :7], gt[0, 0, 7] = boxes[0, 3], 1          # matched only by a box whose padded label drops it from the output
    gt[1, 0, :7], gt[1, 0, 7] = boxes[1, 1], 2
    bd = {'batch_size': B, 'batch_cls_preds': cls, 'batch_box_preds': boxes, 'cls_preds_normalized': True, 'has_class_labels': True,
          'roi_labels': labels, 'rois': boxes.clone(), 'gt_boxes': gt}
    import pcdet.ops.iou3d_nms.iou3d_nms_utils as iu
    seen = []

    def fake_iou(a, b):
        seen.append(a.shape[0])
        return (a[:, None, :3] - b[None, :, :3]).abs().sum(-1).lt(1e-6).float()
    real, iu.boxes_iou3d_gpu = iu.boxes_iou3d_gpu, fake_iou
    try:
        preds, recall = detector.post_processing(bd)
    finally:
        iu.boxes_iou3d_gpu = real
    assert len(preds) == B
    for b in range(B):
        ok = labels[b] != 0
        assert torch.equal(preds[b]['pred_labels'], labels[b][ok])                 # labels from roi_labels, padded rows dropped
        assert torch.equal(preds[b]['pred_boxes'], boxes[b][ok]) and torch.equal(preds[b]['pred_scores'], cls[b, :, 0][ok])
    assert seen == [M, M, M, M]                                                    # recall on ALL boxes (rcnn and roi), both samples
    assert recall['gt_num'] == 2 and recall['recall_rcnn_0.5'] == 2 and recall['recall_roi_0.5'] == 2
    # scores: the maximum over the classes; labels from the best class without has_class_labels
    cls3 = torch.rand(B, M, 3, generator=g)
    p2, _ = detector.post_processing({'batch_size': B, 'batch_cls_preds': cls3, 'batch_box_preds': boxes, 'cls_preds_normalized': True})
    assert torch.equal(p2[0]['pred_scores'], cls3[0].max(-1)[0]) and torch.equal(p2[0]['pred_labels'], cls3[0].argmax(-1) + 1)
    p3, _ = detector.post_processing({'batch_size': B, 'batch_cls_preds': cls3, 'batch_box_preds': boxes, 'cls_preds_normalized': False})
    assert torch.equal(p3[1]['pred_scores'], torch.sigmoid(cls3[1]).max(-1)[0])


def test_refusals_by_name(detector):
    cfg, ds = configs.waymo_two_stage_cfg()
    log = logging.getLogger("t")

    def bad(edit, match):
        c = copy.deepcopy(cfg)
        edit(c)
        with pytest.raises(NotImplementedError, match=match):
            build_network(c, 3, ds, log)
    bad(lambda c: c.ROI_HEAD.__setitem__('IMG_CONFIG', {'IN_DIM': 64, 'MLPS': [32]}), "IMG_CONFIG")
    bad(lambda c: c.ROI_HEAD.ATTN_GNN_CONFIG.__setitem__('USE_FEATS_DIS', True), "USE_FEATS_DIS")
    bad(lambda c: c.ROI_HEAD.NMS_CONFIG.__setitem__('TEST', {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 1024,
                                                             'NMS_POST_MAXSIZE': 100, 'NMS_THRESH': 0.7}), "NMS_CONFIG.TEST")
    bad(lambda c: c.ROI_HEAD.TARGET_CONFIG.__setitem__('BOX_CODER', 'PreviousResidualDecoder'), "BOX_CODER")
    c = copy.deepcopy(cfg)
    c.ROI_HEAD.NMS_CONFIG['TEST'] = None            # a real None is as good as the yaml's string
    build_network(c, 3, ds, log)
    with pytest.raises(NotImplementedError, match="training"):
        copy.deepcopy(detector).train()({'batch_size': 1})
    with pytest.raises(NotImplementedError, match="training"):
        copy.deepcopy(detector.roi_head).train()({'batch_size': 1, 'rois': torch.zeros(1, 1, 7)})
    with pytest.raises(NotImplementedError):
        detector.roi_head.get_loss()
    with pytest.raises(NotImplementedError):
        detector.roi_head.assign_targets({})
    with pytest.raises(NotImplementedError, match="rois"):
        detector.roi_head.proposal_layer({'batch_size': 1}, nms_config=None)
    # existing refusals of post_processing stay: has_class_labels with NMS on, list-valued predictions, batch_index, raw scores
    kcfg, kds = configs.kitti_finetune_cfg()
    pp = build_network(kcfg, 3, kds, log)
    bd = {'batch_size': 1, 'batch_cls_preds': torch.zeros(1, 4, 3), 'batch_box_preds': torch.zeros(1, 4, 7), 'cls_preds_normalized': False}
    with pytest.raises(NotImplementedError, match="has_class_labels"):
        pp.post_processing({**bd, 'has_class_labels': True})
    for extra in ({'batch_cls_preds': [torch.zeros(1, 4, 3)]}, {'batch_index': torch.zeros(4)}):
        with pytest.raises(NotImplementedError):
            detector.post_processing({**bd, **extra})
    c = copy.deepcopy(cfg)
    c.POST_PROCESSING['OUTPUT_RAW_SCORE'] = True
    with pytest.raises(NotImplementedError, match="OUTPUT_RAW_SCORE"):
        build_network(c, 3, ds, log).post_processing(bd)
    from gdmae_hip import inference
    with pytest.raises(NotImplementedError):
        inference.compile_detector(detector)
