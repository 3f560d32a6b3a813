"""CPU: the bookkeeping of ``gdmae_hip.evaluation.RecallRecord`` (key names and ``ret_dict`` arithmetic in the reference's format),
the numpy statement of the recall-record contract against the fp64 oracle on two scenes, the builder's own assertions on
every scene of tests/recall_record_reference.py, and the CPU-tensor refusal."""
import numpy as np
import pytest
import torch

import recall_record_reference as rr
from gdmae_hip import evaluation
from oracle import iou3d_oracle
from pcdet.models.roi_heads import proposal_targets as pt


def test_key_names_and_ret_dict_in_the_reference_format():
    rec = evaluation.RecallRecord([0.3, 0.5, 0.7], "cpu")
    keys = ['gt_num', 'recall_roi_0.3', 'recall_roi_0.5', 'recall_roi_0.7', 'recall_rcnn_0.3', 'recall_rcnn_0.5', 'recall_rcnn_0.7']
    assert rec.counters.dtype == torch.int64 and tuple(rec.counters.shape) == (7,)
    assert rec.result() == dict.fromkeys(keys, 0) and list(rec.result()) == keys
    # gt_num == 0: the reference divides by max(gt_num, 1)
    assert rec.ret_dict() == {f'recall/{s}_{t}': 0.0 for t in ('0.3', '0.5', '0.7') for s in ('roi', 'rcnn')}
    rec.counters += torch.tensor([40, 30, 20, 10, 36, 28, 12])
    r = rec.result()
    assert r == dict(zip(keys, [40, 30, 20, 10, 36, 28, 12])) and all(type(v) is int for v in r.values())
    want = {}
    for t in [0.3, 0.5, 0.7]:                                # eval_utils.py:104-110, with the metric dict of statistics_info
        want['recall/roi_%s' % str(t)] = r['recall_roi_%s' % str(t)] / max(r['gt_num'], 1)
        want['recall/rcnn_%s' % str(t)] = r['recall_rcnn_%s' % str(t)] / max(r['gt_num'], 1)
    assert rec.ret_dict() == want and list(rec.ret_dict()) == list(want) and rec.ret_dict()['recall/rcnn_0.5'] == 0.7
    rec.reset()
    assert rec.result() == dict.fromkeys(keys, 0)
    # keys are str(t) of what the config holds, as the reference formats them
    assert list(evaluation.RecallRecord([0.25, 1], "cpu").result()) == ['gt_num', 'recall_roi_0.25', 'recall_roi_1', 'recall_rcnn_0.25', 'recall_rcnn_1']
    for bad in ([], [0.1] * 9):
        with pytest.raises(ValueError, match="thresholds"):
            evaluation.RecallRecord(bad, "cpu")


@pytest.mark.parametrize("name", sorted(rr.SCENES))
def test_every_scene_passes_its_own_assertions(name):
    S, counters, best = rr.scene(name)
    T = len(S['thresh'])
    assert counters.shape == (1 + 2 * T,) and counters[0] == sum(evaluation.valid_gt_rows(g) for g in S['gt'])
    assert (counters[1:1 + T] == 0).all() == (S['rois'] is None)              # without RoIs the roi counters stay 0
    assert best.shape == (*S['gt'].shape[:2], 2) and best.min() >= 0 and best.max() <= 1 + 1e-12
    assert (np.diff(counters[1:1 + T]) <= 0).all() and (np.diff(counters[1 + T:]) <= 0).all() and counters[1:].max() <= counters[0]


def test_known_answers():
    S, counters, best = rr.scene('identical')
    assert counters.tolist() == [4, 2, 1, 1, 2, 2, 2] and best[0, 0, 1] == pytest.approx(1.0, abs=1e-12) and best[0, 2].tolist() == [0, 0]
    S, counters, best = rr.scene('zero_rows')
    assert counters[0] == 0 + 6 + 9 and (best[0] == 0).all() and (best[1, 2] == 0).all() and (best[1, [0, 1, 3, 4, 5], 1] > 0.7).all()
    S, counters, best = rr.scene('seams')
    assert counters[0] == 12 * 6 and (best[1:, 0, 1] > 0.7).all() and best[0].max() == 0
    S, counters, best = rr.scene('prefilter')
    assert 0 < best[0, 0, 1] < 0.01 and best[0, 1, 1] == 0 and best[0, 2, 1] == 0 and counters.tolist() == [4, 0, 0, 0, 1, 0, 0]
    S, counters, best = rr.scene('counts')
    assert (best[1, :, 1] == 0).all() and (best[2, :, 0] == 0).all() and best[1, :, 0].max() > 0.3


@pytest.mark.parametrize("name", ["counts", "zero_rows"])
def test_statement_against_the_fp64_oracle(name):
    """the package's statement with its own fp64 clipping and no shortcut == the same rules written out on the oracle's geometry"""
    S, counters, best = rr.scene(name)
    got_c, got_b = evaluation.recall_record_numpy(S['pred'], S['pred_num'], S['gt'], S['thresh'], rois=S['rois'], roi_num=S['roi_num'])
    B, G = S['gt'].shape[:2]
    T = len(S['thresh'])
    want_b, want_c = np.zeros((B, G, 2)), np.zeros(1 + 2 * T, np.int64)
    for b in range(B):
        live = np.nonzero(np.abs(S['gt'][b]).sum(axis=1) != 0)[0]
        nv = int(live.max()) + 1 if live.size else 0
        want_c[0] += nv
        for col, side in ((0, 'rois'), (1, 'pred')):
            rows = rr.rows_of(S, side, b)
            for g in range(nv):
                a = S['gt'][b, g].astype(np.float64)
                for p in rows.astype(np.float64):
                    oh = max(min(p[2] + p[5] / 2, a[2] + a[5] / 2) - max(p[2] - p[5] / 2, a[2] - a[5] / 2), 0.0)
                    o3 = iou3d_oracle.exact_overlap(p[:7], a[:7]) * oh if p[3] * p[4] * a[3] * a[4] != 0 else 0.0
                    want_b[b, g, col] = max(want_b[b, g, col], o3 / max(p[3] * p[4] * p[5] + a[3] * a[4] * a[5] - o3, 1e-6))
            for i, t in enumerate(S['thresh']):
                want_c[1 + col * T + i] += int((want_b[b, :nv, col] > t).sum())
    assert np.array_equal(got_c, want_c) and np.array_equal(got_c, counters)
    assert np.abs(got_b - want_b).max() < 1e-9 and np.abs(best - want_b).max() < 1e-9
    assert pt.exact_bev_overlap is not rr.bev_overlap


def test_cpu_tensors_are_refused_by_name():
    S, _, _ = rr.scene('one_gt')
    rec = evaluation.RecallRecord(S['thresh'], "cpu")
    with pytest.raises(NotImplementedError, match="CPU tensors"):
        rec.update(torch.from_numpy(S['pred'].copy()), torch.from_numpy(S['pred_num'].copy()), torch.from_numpy(S['gt'].copy()))
    assert rec.result()['gt_num'] == 0
