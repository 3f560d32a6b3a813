"""Golden for second-stage training of the shipped two-stage config (tools/cfgs/waymo_models/gd_mae_ts.yaml): the reference's
GraphRCNNHead built UNMODIFIED from the yaml section (as in make_golden_roi_head.py: same stubs), its ``assign_targets``
(roi_head_template.py:104-127 on target_assigner/proposal_target_layer.py:13-230) on a crafted batch and its ``get_loss``
(roi_head_template.py:129-224) on seeded ``rcnn_cls`` / ``rcnn_reg``.  Build container only (reads the reference tree); holds none
of its text.

Stand-ins: ``boxes_iou3d_gpu`` of the (absent) ``iou3d_nms_cuda`` extension is the fp64 oracle of oracle/iou3d_oracle.py (height
overlap and union as the reference forms them), ``np.random.seed`` / ``torch.manual_seed`` are fixed, ``Tensor.cuda`` is the
identity while the head is constructed.

B = 2, M = 160 (padded rows included), 11 and 9 GT boxes of three classes in a table of 12 rows, R = 128.  Sample 0 has more fg
RoIs than fg_per_image = 64, sample 1 fewer.  The batch comes from the scene builder of tests/roi_targets_reference.py, which
asserts its margins (IoU thresholds, best / second-best GT, heading wrap points).  The fixture holds the inputs, every field of
``targets_dict``, rcnn_cls / rcnn_reg, the three losses and their sum, and the gradients of the sum."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd"), HERE, os.path.join(REPO, "tests")]

SEED, B, M, G, R = 61, 2, 160, 12, 128


def golden_batch():
    """Runs BEFORE make_golden is imported (it installs the reference's namespace modules): the builder imports this
    repository's ``pcdet``."""
    import roi_targets_reference as rt
    rng = np.random.RandomState(SEED)
    P = rt.sampler_params(R=R)
    g0 = rt.grid_gt(rng, [1, 2, 3, 1, 2, 3, 1, 1, 2, 3])
    nb = g0[0].copy()
    nb[0] -= 1.0 * np.sin(g0[0, 6])
    nb[1] += 1.0 * np.cos(g0[0, 6])
    g0 = np.concatenate([g0, nb[None]])
    pick = lambda n, hi: [int(k) for k in rng.randint(0, hi, n)]      # noqa: E731
    plan0 = [(k, rt.FG) for k in pick(70, 11)] + [(k, rt.HARD) for k in pick(40, 11)] + [(k, rt.EASY) for k in pick(25, 11)]
    r0, l0 = rt.rois_for(rng, g0, plan0, far=15)
    g1 = rt.grid_gt(rng, [2, 1, 3, 1, 2, 3, 1, 2, 1])
    plan1 = [(k, rt.FG) for k in pick(30, 9)] + [(k, rt.HARD) for k in pick(50, 9)] + [(k, rt.EASY) for k in pick(40, 9)]
    r1, l1 = rt.rois_for(rng, g1, plan1, far=20)
    S = rt.assemble(rng, [(g0, r0, l0), (g1, r1, l1)], G=G, M=M, R=R)
    rt.check_margins(S, P)
    cnt = rt.counts(S, P)
    assert cnt[0]['n_fg'] > P['fg_per_image'] > cnt[1]['n_fg'] > 0 and all(c['n_hard'] and c['n_easy'] for c in cnt), cnt
    iou = lambda a, b: rt.pt.iou3d_fp64(a, b, rt.bev_overlap)      # noqa: E731
    return S, iou


def main():
    S, iou = golden_batch()
    for k in [k for k in sys.modules if k == "pcdet" or k.startswith("pcdet.")]:
        del sys.modules[k]
    import make_golden as mg
    import make_golden_roi_head as mgr
    rh, configs = mg.rh, mg.configs
    mgr.install_roi_head_stubs()
    ycfg = rh.load_yaml_cfg("cfgs/waymo_models/gd_mae_ts.yaml")
    mc = ycfg.MODEL
    assert mg.to_plain(mc.ROI_HEAD) == mg.to_plain(configs.graphrcnn_head_cfg())
    iu = sys.modules["pcdet.ops.iou3d_nms.iou3d_nms_utils"]
    iu.boxes_iou3d_gpu = lambda a, b: torch.tensor([[iou(x, y) for y in b.numpy()] for x in a.numpy()], dtype=torch.float32).reshape(a.shape[0], b.shape[0])
    gh = rh.ref("pcdet.models.roi_heads.graphrcnn_head")
    ds = configs.waymo_two_stage_cfg()[1]
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        head = gh.GraphRCNNHead(input_channels=128, model_cfg=mc.ROI_HEAD, point_cloud_range=ds.point_cloud_range,
                                voxel_size=ds.voxel_size, backbone_channels=None, num_class=1)
    finally:
        torch.Tensor.cuda = real_cuda
    head.train()
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    bd = {'batch_size': B, 'rois': torch.from_numpy(S['rois'].copy()), 'roi_scores': torch.from_numpy(S['roi_scores'].copy()),
          'roi_labels': torch.from_numpy(S['roi_labels'].copy()), 'gt_boxes': torch.from_numpy(S['gt_boxes'].copy())}
    td = head.assign_targets(bd)
    g = torch.Generator().manual_seed(SEED + 1)
    rcnn_cls = (torch.randn(B * R, 1, generator=g) * 1.5).requires_grad_()
    rcnn_reg = (torch.randn(B * R, 7, generator=g) * 0.2).requires_grad_()
    head.forward_ret_dict = dict(td, rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg, batch_size=B)
    loss, tb = head.get_loss()
    loss.backward()
    z = {"seed": np.int64(SEED), "rois_in": S['rois'], "roi_scores_in": S['roi_scores'], "roi_labels_in": S['roi_labels'],
         "gt_boxes": S['gt_boxes'], "rcnn_cls": rcnn_cls.detach().numpy(), "rcnn_reg": rcnn_reg.detach().numpy(),
         "losses": np.array([tb['rcnn_loss_cls'], tb['rcnn_loss_reg'], tb['rcnn_loss_corner'], tb['rcnn_loss']], np.float64),
         "grad_cls": rcnn_cls.grad.numpy(), "grad_reg": rcnn_reg.grad.numpy()}
    for k, v in td.items():
        z["t_" + k] = v.detach().numpy()
    assert set(td) == {'rois', 'gt_of_rois', 'gt_iou_of_rois', 'roi_scores', 'roi_labels', 'roi_indices', 'reg_valid_mask', 'rcnn_cls_labels',
                       'gt_of_rois_src'}, sorted(td)
    assert abs(float(loss.detach()) - tb['rcnn_loss']) < 1e-6 and int(z["t_reg_valid_mask"].sum()) > 40
    path = os.path.join(HERE, "roi_targets_b2.npz")
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB", "losses", z["losses"].tolist(), "fg rows", int(z["t_reg_valid_mask"].sum()))


if __name__ == "__main__":
    main()
