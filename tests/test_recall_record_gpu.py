"""GPU: ``gdmae_recall_record`` (csrc/recall_record.hip) through ``gdmae_hip.evaluation.RecallRecord`` against the numpy statement of
the recall-record contract (fp64 geometry from oracle/iou3d_oracle.py) on the crafted scenes of
tests/recall_record_reference.py: at most 130 predicted rows, 40 RoIs and 65 GT rows per sample.  The scenes keep every GT row's
largest IoU 1e-3 away from the thresholds and every compared pair away from the margin cases of the reference's corner test, so
the counters must be equal; ``best_iou`` is compared numerically.

Measured on an MI355X against the fp64 statement, the largest deviation of ``best_iou`` over all scenes (the test prints the figure
per scene): 1.789e-4 (scene zero_rows: the fp32 polygon of ``bev_overlap`` against exact clipping;
tests/test_roi_targets_gpu.py measured 1.290e-4 for the same arithmetic on its scenes).  The bound is 4 x that."""
import numpy as np
import pytest
import torch

import recall_record_reference as rr
from gdmae_hip import evaluation
from gdmae_hip import lib as L
from pcdet.models.detectors.detector3d_template import Detector3DTemplate

pytestmark = pytest.mark.gpu

MEASURED_BEST_IOU = 1.789e-4


def dev_inputs(S, samples=None):
    t = lambda a: None if a is None else torch.from_numpy(a[samples].copy() if samples is not None else a.copy()).cuda()      # noqa: E731
    return dict(pred_boxes=t(S['pred']), pred_num=t(S['pred_num']), gt_boxes=t(S['gt']), rois=t(S['rois']), roi_num=t(S['roi_num']))


def run_hip(S, rec=None, samples=None):
    rec = rec or evaluation.RecallRecord(S['thresh'], "cuda")
    best = rec.update(**dev_inputs(S, samples))
    torch.cuda.synchronize()
    return rec, best.cpu().numpy()


@pytest.mark.parametrize("name", sorted(rr.SCENES))
def test_kernel_matches_the_statement(name):
    S, counters, ref = rr.scene(name)
    rec, best = run_hip(S)
    assert best.shape == ref.shape and best.dtype == np.float32
    d = float(np.abs(best.astype(np.float64) - ref).max())
    print(f"{name}: best_iou deviation from the fp64 statement {d:.3e}; counters {rec.counters.tolist()}")
    assert rec.counters.tolist() == counters.tolist()
    assert rec.result() == dict(zip(evaluation.counter_names(S['thresh']), counters.tolist()))
    assert d <= 4 * MEASURED_BEST_IOU
    for b in range(S['gt'].shape[0]):                                  # rows at or beyond the valid count: exactly 0
        assert not best[b, evaluation.valid_gt_rows(S['gt'][b]):].any()
    if S['rois'] is None:
        assert not best[..., 0].any()


def test_identical_box_is_recalled_at_every_threshold():
    S, counters, _ = rr.scene('identical')
    rec, best = run_hip(S)
    assert abs(float(best[0, 0, 1]) - 1.0) <= 4 * MEASURED_BEST_IOU and abs(float(best[0, 3, 1]) - 1.0) <= 4 * MEASURED_BEST_IOU
    r = rec.result()
    assert r['recall_rcnn_0.3'] == r['recall_rcnn_0.5'] == r['recall_rcnn_0.7'] == 2


def test_updates_accumulate_and_reset():
    S, c1, _ = rr.scene('counts')
    rec, _ = run_hip(S)
    run_hip(S, rec)
    assert rec.counters.tolist() == (2 * c1).tolist()
    rec.reset()
    assert rec.counters.tolist() == [0] * 7
    S2, c2, _ = rr.scene('zero_rows')
    run_hip(S2, rec)
    run_hip(S, rec)
    assert rec.counters.tolist() == (c1 + c2).tolist()
    assert rec.ret_dict()['recall/rcnn_0.3'] == int(c1[4] + c2[4]) / int(c1[0] + c2[0])


@pytest.mark.parametrize("name", ["counts", "zero_rows", "seams"])
def test_a_sample_alone_and_inside_the_batch(name):
    S, counters, _ = rr.scene(name)
    _, whole = run_hip(S)
    rec = evaluation.RecallRecord(S['thresh'], "cuda")
    for b in range(S['gt'].shape[0]):
        _, one = run_hip(S, rec, samples=slice(b, b + 1))
        assert one.tobytes() == whole[b:b + 1].tobytes(), b
    assert rec.counters.tolist() == counters.tolist()


@pytest.mark.parametrize("name", sorted(rr.SCENES))
def test_counters_equal_generate_recall_record(name):
    """the per-sample function on the same device tensors (rows behind a count trimmed for the predictions, zeroed for the RoIs: the
    function takes all RoI rows, and a zero box has IoU 0 with everything)"""
    S, _, _ = rr.scene(name)
    t = dev_inputs(S)
    rec = evaluation.RecallRecord(S['thresh'], "cuda")
    rec.update(**t)
    B = S['gt'].shape[0]
    dd = {'gt_boxes': t['gt_boxes']}
    if t['rois'] is not None:
        dd['rois'] = t['rois'].clone()
        if t['roi_num'] is not None:
            for b in range(B):
                dd['rois'][b, int(S['roi_num'][b]):] = 0
    want = {}
    for b in range(B):
        n = S['pred'].shape[1] if S['pred_num'] is None else int(S['pred_num'][b])
        want = Detector3DTemplate.generate_recall_record(t['pred_boxes'][b, :n], want, b, data_dict=dd, thresh_list=S['thresh'])
    assert rec.result() == want


def test_no_host_read():
    S, counters, _ = rr.scene('counts')
    t = dev_inputs(S)
    rec = evaluation.RecallRecord(S['thresh'], "cuda")
    rec.update(**t)                                                    # loads the library, outside the checked region
    torch.cuda.synchronize()
    rec.reset()
    mode = torch.cuda.get_sync_debug_mode()
    control = False
    try:
        torch.cuda.set_sync_debug_mode("error")
        rec.update(**t)
        try:
            Detector3DTemplate.generate_recall_record(t['pred_boxes'][0], {}, 0, data_dict={'gt_boxes': t['gt_boxes']}, thresh_list=S['thresh'])
        except RuntimeError:
            control = True
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    if not control:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on the per-sample function's host reads in this torch build")
    assert rec.counters.tolist() == counters.tolist()


def test_refusals():
    """T outside 1 .. 8, any *_cols < 7 and negative sizes are error returns before a pointer is touched; n, M, G of 0 are legal"""
    lib = L.load()
    th = L.host_f32([0.5] * 9)

    def rc(B=1, n=4, pc=7, M=0, rcols=7, G=4, gc=8, T=3):
        return lib.gdmae_recall_record(None, None, B, n, pc, None, None, M, rcols, None, G, gc, th, T, None, None, None)
    for kw in (dict(T=0), dict(T=9), dict(pc=6), dict(rcols=6), dict(gc=6), dict(B=-1), dict(n=-1), dict(M=-1), dict(G=-1)):
        assert rc(**kw) != 0 and b"recall_record" in lib.gdmae_last_error(), kw
    with pytest.raises(L.GdmaeHipError, match="7 columns"):
        evaluation.RecallRecord([0.5], "cuda").update(torch.zeros(1, 4, 6, device="cuda"), None, torch.zeros(1, 4, 8, device="cuda"))
    # zero sizes run: gt_num still grows without predictions, and nothing happens without GT rows
    S, counters, _ = rr.scene('identical')
    gt = torch.from_numpy(S['gt'].copy()).cuda()
    rec = evaluation.RecallRecord(S['thresh'], "cuda")
    best = rec.update(torch.zeros(1, 0, 7, device="cuda"), None, gt, rois=torch.zeros(1, 0, 7, device="cuda"))
    assert rec.counters.tolist() == [4, 0, 0, 0, 0, 0, 0] and not best.any()
    best = rec.update(torch.from_numpy(S['pred'].copy()).cuda(), None, gt[:, :0])
    assert rec.counters.tolist() == [4, 0, 0, 0, 0, 0, 0] and tuple(best.shape) == (1, 0, 2)
    # T = 8: the scene's largest IoUs over the predicted rows are 1, 1, one below 0.28 and 0
    rec8 = evaluation.RecallRecord([0.29, 0.3, 0.31, 0.5, 0.69, 0.7, 0.71, 0.99], "cuda")
    rec8.update(torch.from_numpy(S['pred'].copy()).cuda(), torch.from_numpy(S['pred_num'].copy()).cuda(), gt)
    assert rec8.counters.tolist() == [4] + [0] * 8 + [2] * 8
