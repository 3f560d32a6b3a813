"""GPU: ``gdmae_roi_targets`` (csrc/roi_targets.hip) against the numpy statement of the proposal-target contract (fp64
geometry from oracle/iou3d_oracle.py) on the crafted scenes of tests/roi_targets_reference.py: R = 16, M <= 40, G <= 12, one scene
with M = 130 and G = 70.  The scenes keep every decision (thresholds, best GT, heading wraps) away from its boundary, so indices,
labels, masks and the integer ``cls`` labels must be equal and copied rows bit-identical.

Measured on an MI355X against the fp64 statement, the largest over all scenes (the tests print the figures per scene):
``gt_iou_of_rois`` 1.290e-4 (scene strides: the fp32 polygon of ``bev_overlap`` against exact clipping), the ``roi_iou`` labels
1.202e-4 (scene one_bg_list: the overlap's deviation times 1 / (0.75 - 0.25)), ``gt_of_rois`` 1.526e-5 (scene strides: one fp32 ulp
of a 130 m offset to GT row 0).  The bounds are 4 x these (tests/test_iou3d_nms.py bounds ``gdmae_boxes_bev_pairs`` against the same
oracle the same way)."""
import numpy as np
import pytest
import torch

import roi_targets_reference as rt
from gdmae_hip import lib as L
from pcdet.models.roi_heads import proposal_targets as pt

pytestmark = pytest.mark.gpu

MEASURED_IOU = 1.290e-4
MEASURED_LABEL = 1.202e-4
MEASURED_CT = 1.526e-5


def run_hip(S, P):
    t = lambda a: torch.from_numpy(a.copy()).cuda()      # noqa: E731
    out = pt.roi_targets(t(S['rois']), t(S['roi_scores']), t(S['roi_labels']), t(S['gt_boxes']), t(S['u_fg']), t(S['u_bg']), P)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", sorted(rt.SCENES))
def test_kernel_matches_the_statement(name):
    S, P, ref = rt.scene(name)
    out = run_hip(S, P)
    assert set(out) == set(pt.FIELDS)
    for k in pt.FIELDS:
        assert out[k].shape == ref[k].shape and out[k].dtype == ref[k].dtype, k
    assert np.array_equal(out['roi_indices'], ref['roi_indices']), np.nonzero(out['roi_indices'] != ref['roi_indices'])
    for k in ('roi_labels', 'reg_valid_mask'):
        assert np.array_equal(out[k], ref[k]), k
    for k in ('rois', 'roi_scores', 'gt_of_rois_src'):
        assert out[k].tobytes() == ref[k].tobytes(), k
    d = lambda k: float(np.abs(out[k].astype(np.float64) - ref[k].astype(np.float64)).max())      # noqa: E731
    print(f"{name}: deviation from the fp64 statement: gt_iou_of_rois {d('gt_iou_of_rois'):.3e} rcnn_cls_labels {d('rcnn_cls_labels'):.3e} "
          f"gt_of_rois {d('gt_of_rois'):.3e}; counts {rt.counts(S, P)}")
    if P['cls_type'] == 'cls':
        assert np.array_equal(out['rcnn_cls_labels'], ref['rcnn_cls_labels'])
    else:
        assert d('rcnn_cls_labels') <= 4 * MEASURED_LABEL
    assert d('gt_iou_of_rois') <= 4 * MEASURED_IOU and d('gt_of_rois') <= 4 * MEASURED_CT


def test_refusals():
    S, P, _ = rt.scene('duplicate_gt')
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device='cuda')      # noqa: E731
    with pytest.raises(NotImplementedError, match="RoIs per sample"):
        pt.roi_targets(z(1, 1025, 7), z(1, 1025), z(1, 1025, dt=torch.int64), z(1, 4, 8), z(1, 1025), z(1, 16), P)
    with pytest.raises(NotImplementedError, match="GT rows"):
        pt.roi_targets(z(1, 8, 7), z(1, 8), z(1, 8, dt=torch.int64), z(1, 1025, 8), z(1, 8), z(1, 16), P)
    with pytest.raises(NotImplementedError, match="ROI_PER_IMAGE"):
        pt.roi_targets(z(1, 8, 7), z(1, 8), z(1, 8, dt=torch.int64), z(1, 4, 8), z(1, 8), z(1, 1025), rt.sampler_params(R=1025))
    with pytest.raises(NotImplementedError, match="columns"):
        pt.roi_targets(z(1, 8, 9), z(1, 8), z(1, 8, dt=torch.int64), z(1, 4, 8), z(1, 8), z(1, 16), P)
    # the entry point itself returns non-zero before it touches a pointer
    lib = L.load()
    for M, G, R, cols in ((1025, 4, 16, 7), (8, 1025, 16, 7), (8, 4, 1025, 7), (8, 4, 16, 8)):
        rc = lib.gdmae_roi_targets(None, None, None, 1, M, cols, None, G, None, None, None, R, 8, 0.55, 0.75, 0.25, 0.1, 1, 0,
                                   None, None, None, None, None, None, None, None, None, None, 0, None)
        assert rc != 0 and b"roi_targets" in lib.gdmae_last_error()
    # at the limits it runs: M = G = 1024 rows (all padded but a few), R = 1024
    P2 = rt.sampler_params(R=1024)
    rois, labels, gt = np.zeros((1, 1024, 7), np.float32), np.zeros((1, 1024), np.int64), np.zeros((1, 1024, 8), np.float32)
    rois[0, :9], labels[0, :9], gt[0, :6] = S['rois'][0], S['roi_labels'][0], S['gt_boxes'][0]
    gt[0, 1023] = gt[0, 0]                                             # the last row is valid: all 1024 rows are compared
    gt[0, 1023, :2] += 200.0
    gt[0, 6:1023, 7] = 2                                               # label-only rows in between: only the class-2 RoIs visit them
    rng = np.random.RandomState(9)
    S2 = dict(rois=rois, roi_scores=rng.random_sample((1, 1024)).astype(np.float32), roi_labels=labels, gt_boxes=gt,
              u_fg=rng.random_sample((1, 1024)).astype(np.float32), u_bg=rng.random_sample((1, 1024)).astype(np.float32))
    out = run_hip(S2, P2)
    ref = rt.reference(rois, S2['roi_scores'], labels, gt, S2['u_fg'], S2['u_bg'], P2)
    assert np.array_equal(out['roi_indices'], ref['roi_indices']) and np.array_equal(out['reg_valid_mask'], ref['reg_valid_mask'])
    assert out['gt_of_rois_src'].tobytes() == ref['gt_of_rois_src'].tobytes()
