"""CPU: the numpy statement of the KITTI evaluator (``gdmae_hip.evaluation.kitti_eval_numpy``) against the reference's
``get_official_eval_result`` / ``eval_class`` recorded in tests/golden/kitti_eval.npz (tests/golden/make_golden_kitti_eval.py: the
unmodified reference under a numba stand-in), plus the host-side pieces of ``kitti_eval``: the alpha == -10 decision, the shim module
and the refusal of a CPU device.

The golden scene keeps the margins of tests/kitti_eval_reference.py (asserted again here), so tp / fp / fn are the same integers in
the statement's fp64 geometry and in the reference's fp32 polygon arithmetic: precision and recall must be EQUAL, bit for bit.

The orientation curve is a quotient of a sum of cosines; statement and reference add the same fp64 terms in the same order (the
true positives of a frame in GT order, then the frames in order).  Measured here (the test prints the figures): orientation 0.0,
AP values 0.0.  Four times nothing is nothing, and an exact zero is not what the arithmetic promises: numpy may evaluate ``cos`` on
an array (the statement) by another code path than on a scalar (the reference), 1 ulp = 1.1e-16 per term, with up to about 400 terms
and as many additions behind a quotient <= 1.  Asserted: 400 x 2 x 1.1e-16 = 8.8e-14 on the orientation curve and, AP being a mean
of such values in percent, 8.8e-12 on the AP values."""
import os

import numpy as np
import pytest

import kitti_eval_reference as kr
from gdmae_hip import evaluation

BOUND_ORIENTATION, BOUND_AP = 8.8e-14, 8.8e-12
CLASSES = ['Car', 'Pedestrian', 'Cyclist']


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "kitti_eval.npz"))
    gt_annos, dt_annos = kr.unpack_annos(z)
    return z, gt_annos, dt_annos, kr.statement(gt_annos, dt_annos, CLASSES)


def test_golden_scene_keeps_the_margins_and_holds_every_case(golden):
    _, gt_annos, dt_annos, (_, _, st) = golden
    for g, d in zip(gt_annos, dt_annos):
        why = []
        assert kr.margins_hold(g, d, why), why
    assert {'Car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting', 'DontCare', 'Truck', 'Tram'} <= set(n for a in gt_annos for n in a['name'])
    for flags in (st['clean']['ignored_gt'], st['clean']['ignored_dt']):
        assert all(set(np.unique(flags[c, l]).tolist()) == {-1, 0, 1} for c in range(3) for l in range(3))
    matched = (st['matched'] > -np.inf).sum(axis=1)
    assert matched.max() > 41 and (st['n_thresholds'] < matched).any()          # get_thresholds skips


def test_precision_and_recall_equal_the_reference(golden):
    z, _, _, (_, _, st) = golden
    assert st['precision'].shape == z['ref_precision'].shape == (3, 3, 3, 2, 41)
    assert np.array_equal(st['precision'], z['ref_precision'], equal_nan=True)
    assert np.array_equal(st['recall'], z['ref_recall'], equal_nan=True)
    assert (z['ref_precision'] > 0).any(axis=-1).all(axis=(2, 3)).any()


def test_orientation_and_ap_values_within_the_measured_bound(golden):
    z, _, _, (result, ret, st) = golden
    d = float(np.abs(st['aos'][0] - z['ref_orientation'][0]).max())
    assert not st['aos'][1:].any() and not z['ref_orientation'][1:].any()
    keys = [str(k) for k in z['ret_keys']]
    assert list(ret.keys()) == keys and len(keys) == 36
    d_ap = float(np.abs(np.array([ret[k] for k in keys]) - z['ret_values']).max())
    print(f"orientation deviation from the reference {d:.3e}; AP deviation {d_ap:.3e}")
    assert d <= BOUND_ORIENTATION and d_ap <= BOUND_AP


def test_result_text_has_the_reference_line_structure(golden):
    z, _, _, (result, _, _) = golden
    ours, theirs = result.split("\n"), str(z['result']).split("\n")
    assert len(ours) == len(theirs) == 3 * 2 * 10 + 1
    for a, b in zip(ours, theirs):
        assert a.split(":")[0] == b.split(":")[0]
        va, vb = ([float(v) for v in s.split(":")[1].split(",")] if s.count(":") == 1 and s.split(":")[1] else [] for s in (a, b))
        assert len(va) == len(vb) and all(abs(x - y) <= 1.01e-4 for x, y in zip(va, vb)), (a, b)
    assert result == str(z['result'])          # on this scene no value sits at a rounding point of the text: character for character


def minus_ten(dt_annos):
    return [dict(a, alpha=np.full_like(a['alpha'], -10)) for a in dt_annos]


def test_alpha_minus_ten_produces_no_aos(golden):
    _, gt_annos, dt_annos, (result, ret, _) = golden
    assert evaluation.kitti_compute_aos(dt_annos) and "aos  AP:" in result
    r2, ret2, st2 = kr.statement(gt_annos[:3], minus_ten(dt_annos[:3]), CLASSES)
    assert not st2['compute_aos'] and "aos" not in r2 and not any("aos" in k for k in ret2) and len(ret2) == 27
    assert not st2['aos'].any() and len(r2.split("\n")) == 3 * 2 * 8 + 1
    # the first detection anno WITH rows decides; an empty one in front of it does not
    empty = {k: v[:0] for k, v in dt_annos[0].items()}
    assert evaluation.kitti_compute_aos([empty] + dt_annos) and not evaluation.kitti_compute_aos([empty] + minus_ten(dt_annos))
    assert not evaluation.kitti_compute_aos([empty])
    detail = {}
    kr.statement(gt_annos[:2], dt_annos[:2], 'Car', PR_detail_dict=detail)
    assert sorted(detail) == ['3d', 'aos', 'bbox', 'bev'] and all(v.shape == (1, 3, 2, 41) for v in detail.values())


def test_class_names_as_ints_and_single_names(golden):
    _, gt_annos, dt_annos, _ = golden
    a = kr.statement(gt_annos[:2], dt_annos[:2], ['Car', 'Cyclist'])
    b = kr.statement(gt_annos[:2], dt_annos[:2], [0, 2])
    assert a[0] == b[0] and a[1] == b[1]
    assert kr.statement(gt_annos[:2], dt_annos[:2], 'Car')[0] == kr.statement(gt_annos[:2], dt_annos[:2], [0])[0]


def deciding_pair(gt_annos, dt_annos):
    """frame 0: the last detection and GT row 0 (a true positive by construction) as the BEV boxes the statement hands to bev_overlap"""
    g, d = gt_annos[0], dt_annos[0]
    rect = lambda a, i: tuple(float(v) for v in (a['location'][i, 0], a['location'][i, 2], 0.0, a['dimensions'][i, 0], a['dimensions'][i, 2], 0.0, -a['rotation_y'][i]))      # noqa: E731
    return rect(d, len(d['name']) - 1), rect(g, 0)


@pytest.mark.parametrize("change", ["pushed across 0.7", "pair dropped"])
def test_the_statement_can_fail(golden, change):
    """one overlap pushed across 0.7, or one (detection, GT) pair dropped, changes asserted integers"""
    _, gt_annos, dt_annos, _ = golden
    pair = deciding_pair(gt_annos, dt_annos)
    seen = []

    def tampered(a, b):
        v = kr.bev_overlap(a, b)
        if (tuple(float(x) for x in a), tuple(float(x) for x in b)) == pair:
            seen.append(v)
            return 0.7 * v if change == "pushed across 0.7" else 0.0
        return v
    _, _, st = kr.statement(gt_annos[:2], dt_annos[:2], CLASSES)
    _, _, st2 = evaluation.kitti_eval_numpy(gt_annos[:2], dt_annos[:2], CLASSES, bev_overlap=tampered, stages=True)
    assert len(seen) == 1 and seen[0] > 0
    before, after = st['overlaps'][0][1, -1, 0], st2['overlaps'][0][1, -1, 0]
    assert before > 0.7 + kr.MARGIN and after < 0.7 - kr.MARGIN
    assert not np.array_equal(st['pr_counts'], st2['pr_counts'])
    assert np.array_equal(st['pr_counts'][:18], st2['pr_counts'][:18])          # the image metric does not see the BEV boxes
    assert not np.array_equal(st['precision'], st2['precision'], equal_nan=True)


def test_shim_forwards(golden, monkeypatch):
    import torch
    from pcdet.datasets.kitti.kitti_object_eval_python import eval as shim
    _, gt_annos, dt_annos, _ = golden
    calls = []
    monkeypatch.setattr(evaluation, "kitti_eval", lambda *a, **k: calls.append(("hip", a, k)) or ("hip", {}))
    monkeypatch.setattr(evaluation, "kitti_eval_numpy", lambda *a, **k: calls.append(("numpy", a, k)) or ("numpy", {}))
    detail = {}
    for available, want in ((False, "numpy"), (True, "hip")):
        monkeypatch.setattr(torch.cuda, "is_available", lambda available=available: available)
        assert shim.get_official_eval_result(gt_annos, dt_annos, CLASSES, PR_detail_dict=detail)[0] == want
        kind, a, k = calls[-1]
        assert kind == want and a[0] is gt_annos and a[1] is dt_annos and a[2] is CLASSES and k['PR_detail_dict'] is detail


def test_cpu_device_is_refused_by_name(golden):
    _, gt_annos, dt_annos, _ = golden
    for call in (lambda: evaluation.kitti_eval(gt_annos, dt_annos, CLASSES, device="cpu"),
                 lambda: evaluation.KittiEval(gt_annos, dt_annos, CLASSES, "cpu")):
        with pytest.raises(NotImplementedError, match="kitti_eval"):
            call()


def test_clean_data_equals_a_row_by_row_restatement(golden):
    """the vectorised flags against the per-row rules, spelled out the slow way"""
    _, gt_annos, dt_annos, (_, _, st) = golden
    cd = st['clean']
    for c, name in enumerate(n.lower() for n in CLASSES):
        for l in range(3):
            want_gt, want_dt = [], []
            for g, d in zip(gt_annos, dt_annos):
                for i in range(len(g['name'])):
                    n = g['name'][i].lower()
                    valid = 1 if n == name else (0 if (name, n) in (('pedestrian', 'person_sitting'), ('car', 'van')) else -1)
                    ignore = (g['occluded'][i] > evaluation.KITTI_MAX_OCCLUSION[l] or g['truncated'][i] > evaluation.KITTI_MAX_TRUNCATION[l]
                              or g['bbox'][i, 3] - g['bbox'][i, 1] <= evaluation.KITTI_MIN_HEIGHT[l])
                    want_gt.append(0 if valid == 1 and not ignore else (1 if valid == 0 or (ignore and valid == 1) else -1))
                for i in range(len(d['name'])):
                    small = abs(d['bbox'][i, 3] - d['bbox'][i, 1]) < evaluation.KITTI_MIN_HEIGHT[l]
                    want_dt.append(1 if small else (0 if d['name'][i].lower() == name else -1))
            assert cd['ignored_gt'][c, l].tolist() == want_gt and cd['ignored_dt'][c, l].tolist() == want_dt
            assert cd['num_valid'][c, l] == want_gt.count(0)
    assert cd['dc_rows'].sum() == sum(int((g['name'] == 'DontCare').sum()) for g in gt_annos) == cd['dc_off'][-1] > 0
