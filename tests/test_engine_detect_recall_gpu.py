"""GPU: ``engine.detect(batch_dict, recall=record)`` of the three engines and ``gdmae_hip.evaluation.evaluate`` on the small models and
scenes of the existing engine tests (tests/test_inference_engine.py, ``two_stage_scene`` of tests/test_center_head_detect_gpu.py, the
tie-free anchor scene of tests/test_anchor_detect_gpu.py: the scenes on which ``detect`` and ``engine(batch_dict)`` are asserted equal).

``gt_boxes`` are built from the engine's own output: jittered copies of some of ``detect``'s boxes (and, for the two-stage engine, of
its RoIs), two boxes far from everything and zero padding.  A candidate whose largest IoU (``boxes_iou3d_gpu``) on either side lies
within 1e-3 of a threshold is rejected, so the device record, the per-sample function and the op-by-op tail must agree exactly."""
import math

import numpy as np
import pytest
import torch

from gdmae_hip import evaluation
from pcdet.models.detectors.detector3d_template import Detector3DTemplate
from pcdet.ops.iou3d_nms.iou3d_nms_utils import boxes_iou3d_gpu

pytestmark = pytest.mark.gpu

G_ROWS = 12


def make_gt(sides, thresh, seed, pc_range, take=6):
    """sides: list over the samples of lists of (k, 7) box tensors -> gt_boxes (B, G_ROWS, 8): ``take`` jittered copies, two far boxes,
    zeros.  Every row's largest IoU with every side is >= 1e-3 away from every threshold (the far boxes': 0)."""
    rng = np.random.RandomState(seed)
    dev = sides[0][0].device
    gt = torch.zeros(len(sides), G_ROWS, 8, device=dev)

    def best(box):
        g = torch.tensor(box[None, :7], dtype=torch.float32, device=dev)
        return [float(boxes_iou3d_gpu(s.contiguous(), g).max()) if s.shape[0] else 0.0 for s in side]
    for b, side in enumerate(sides):
        cand = torch.cat(side).cpu().numpy().astype(np.float64)
        assert cand.shape[0] > 0, "the scene has no box to copy"
        rows = []
        for _ in range(200):
            if len(rows) == take:
                break
            j = cand[rng.randint(cand.shape[0])].copy()
            s = j[3] * rng.uniform(0.0, 0.45) * rng.choice([-1.0, 1.0])
            j[0] += s * math.cos(j[6])
            j[1] += s * math.sin(j[6])
            j[2] += rng.uniform(-0.1, 0.1)
            j[3:6] *= rng.uniform(0.92, 1.08, 3)
            j[6] += rng.uniform(-0.08, 0.08)
            if all(abs(v - t) >= 1e-3 for v in best(j) for t in thresh):
                rows.append(np.append(j, 1.0 + len(rows) % 3))
        assert len(rows) == take
        for i in range(2):
            far = np.array([pc_range[0] + 2.0 + 5.0 * i, pc_range[4] - 2.0, 0.0, 2.0, 1.0, 1.5, 0.3, 1.0])
            assert max(best(far)) == 0.0, "the far box meets a predicted box"
            rows.append(far)
        gt[b, :len(rows)] = torch.tensor(np.stack(rows), dtype=torch.float32, device=dev)
    return gt


def per_sample_record(out, gt, thresh, rois=None, roi_num=None):
    """``generate_recall_record`` sample by sample on ``detect``'s own boxes (RoI rows behind the count zeroed: IoU 0)"""
    dd = {'gt_boxes': gt}
    if rois is not None:
        dd['rois'] = rois[..., :7].clone()
        for b, n in enumerate(roi_num.tolist()):
            dd['rois'][b, n:] = 0
    want = {}
    for b, n in enumerate(out['num'].tolist()):
        want = Detector3DTemplate.generate_recall_record(out['pred_boxes'][b, :n], want, b, data_dict=dd, thresh_list=thresh)
    return want


def check_engine(eng, net, bd, pc_range, rois=None, roi_num=None):
    post = net.model_cfg.POST_PROCESSING
    thresh = list(post.RECALL_THRESH_LIST)
    dev = bd['points'].device
    B = int(bd['batch_size'])
    out0 = eng.detect(dict(bd))
    nums = out0['num'].tolist()
    assert sum(nums) > 0
    sides = [[out0['pred_boxes'][b, :nums[b], :7]] + ([rois[b, :int(roi_num[b]), :7]] if rois is not None else []) for b in range(B)]
    gt_a, gt_b = make_gt(sides, thresh, 11, pc_range), make_gt(sides, thresh, 12, pc_range)
    bd_a, bd_b = dict(bd, gt_boxes=gt_a), dict(bd, gt_boxes=gt_b)

    # the same tensors with and without the record
    rec = evaluation.RecallRecord(thresh, dev)
    out1 = eng.detect(dict(bd_a), recall=rec)
    assert set(out1) == set(out0)
    for k in out0:
        assert torch.equal(out1[k], out0[k]), k
    got = rec.result()
    print(f"{type(eng).__name__}: boxes {nums}, record {got}")
    # the op-by-op tail of engine(batch_dict) and the per-sample function on detect's own boxes
    assert got == eng(dict(bd_a))[1]
    assert got == per_sample_record(out0, gt_a, thresh, rois, roi_num)
    T0 = 'recall_rcnn_%s' % str(thresh[0])
    assert got['gt_num'] == B * 8 and 0 < got[T0] <= B * 6                 # the far boxes are never recalled
    if rois is None:
        assert all(got['recall_roi_%s' % str(t)] == 0 for t in thresh)
    else:
        assert got['recall_roi_%s' % str(thresh[0])] > 0

    # no gt_boxes, or RECALL_MODE other than normal: the record stays untouched and the output is the same
    idle = evaluation.RecallRecord(thresh, dev)
    eng.detect(dict(bd), recall=idle)
    post.RECALL_MODE = 'speed'
    try:
        out2 = eng.detect(dict(bd_a), recall=idle)
    finally:
        post.pop('RECALL_MODE')
    assert idle.counters.tolist() == [0] * (1 + 2 * len(thresh)) and torch.equal(out2['pred_boxes'], out0['pred_boxes'])

    # evaluate: two batches, the summed record and the per-sample lists
    preds, ret = evaluation.evaluate(eng, [dict(bd_a), dict(bd_b)])
    eng.detect(dict(bd_b), recall=rec)                                   # rec now holds batch a + batch b
    both = per_sample_record(out0, gt_b, thresh, rois, roi_num)
    assert rec.result() == {k: got[k] + both[k] for k in got}
    assert ret == rec.ret_dict() and ret['recall/rcnn_%s' % str(thresh[0])] == (got[T0] + both[T0]) / (2 * B * 8)
    want = net.padded_to_pred_dicts(out0)
    assert len(preds) == 2 * B
    for a, w in zip(preds, want + want):
        assert set(a) == set(w) == {'pred_boxes', 'pred_scores', 'pred_labels'}
        for k in w:
            assert torch.equal(a[k], w[k]), k
    none, ret2 = evaluation.evaluate(eng, [dict(bd_a), dict(bd_b)], keep_predictions=False)
    assert none is None and ret2 == ret

    # the record's thresholds must be the config's
    with pytest.raises(ValueError, match="RECALL_THRESH_LIST"):
        eng.detect(dict(bd_a), recall=evaluation.RecallRecord(thresh[:-1] + [0.9], dev))
    with pytest.raises(ValueError, match="RECALL_THRESH_LIST"):
        eng.detect(dict(bd_a), recall=evaluation.RecallRecord(thresh[:1], dev))


def test_centerpoint_engine():
    from gdmae_hip import inference
    from test_inference_engine import _batch, _model
    net, ds, skw = _model()
    check_engine(inference.compile_detector(net), net, _batch(ds, skw), ds.point_cloud_range)


def test_graphrcnn_engine():
    from gdmae_hip import configs, inference
    from test_center_head_detect_gpu import two_stage_scene
    scene = two_stage_scene()
    eng, net = scene["engine"], scene["net"]
    bd = {"points": scene["points"], "batch_size": 2}
    # the call order of test_graphrcnn_engine_detect_equals_the_engine_call, which asserts the two tails equal on this scene: the
    # engine call comes first.  (Measured on an MI355X on this scene, eight ``detect`` calls in a fresh process, no record anywhere:
    # the first call's boxes are up to 0.82 m away from those of the other seven, which are bit-equal; with
    # ``CenterPointEngine.detect`` in front of each, the first call of each kind differs - the first stage's boxes by up to 0.75 m,
    # scores, labels and counts equal - and the rest are bit-equal.  The second stage alone on fixed RoIs repeats bit for bit.  So
    # the first stage's first call or two in a process differ from its later ones; that code is not touched here.)
    eng(dict(bd))
    first = inference.CenterPointEngine.detect(eng, dict(bd))
    M = max(1, int(first['num'].max()))
    check_engine(eng, net, bd, configs.waymo_two_stage_cfg()[1].point_cloud_range, rois=first['pred_boxes'][:, :M].contiguous(), roi_num=first['num'])


def test_anchor_engine():
    from gdmae_hip import inference
    from test_anchor_detect_gpu import TIE_FREE_SEED, TIE_FREE_THRESH
    from test_inference_engine_kitti import _batch, _model

    def edit(cfg):
        cfg.POST_PROCESSING.SCORE_THRESH = TIE_FREE_THRESH
    net, ds = _model(cfg_edit=edit)
    check_engine(inference.compile_detector(net), net, _batch(ds, seed=TIE_FREE_SEED), ds.point_cloud_range)
