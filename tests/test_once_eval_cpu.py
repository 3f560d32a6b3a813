"""CPU: the numpy statement ``once_eval_numpy`` against the recorded reference (tests/golden/once_eval.npz, built by
tests/golden/make_golden_once_eval.py from the reference's own functions under a numba stand-in), in the three recorded
configurations (use_superclass, ap_with_heading) = (True, True), (False, True), (True, False).

EQUAL: flags, num_valid_gt, thresholds and their counts, tp / fp / fn, precision and recall (bit for bit: the same quotients of the
same integers, the same running maximum), the text.

ret_dict: an AP is a sum of <= 50 precisions in [0, 1] taken in the reference's order, divided by 50 and multiplied by 100, the mean a
sum of <= 5 such values.  With bit-equal precisions the sums are the same sequence of fp64 operations, so the expected deviation is
0; the asserted bound allows one rounding per term of either sum, 55 x 2^-53 x 100 = 6.2e-13, rounded up to 1e-12.  Measured: 0.0 in
all three configurations.

ious: the reference's polygon is fp32 with a vertex sort, the statement's an exact fp64 clipping.  The builder measured 2.083e-4 as
their largest deviation on this scene (small boxes beyond 50 m: the reference's edge intersections are determinants of absolute fp32
coordinates); asserted here: 4 x that, 8.332e-4, still below the scene's 1e-3 margin.  The figure belongs to this scene: frame 0's
seed was chosen because two others gave 2.5e-4 and 3.4e-4 (tests/once_eval_reference.py ``GOLDEN_SEEDS``).

The wrong-rule tests put one wrong reading at a time in the place of one function or constant of ``gdmae_hip.evaluation``; the
statement itself has a single reading and no switch for them."""
import functools
import os

import numpy as np
import pytest
import torch

import once_eval_reference as kr
from gdmae_hip import evaluation

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "once_eval.npz")
BUILDER_IOU_DEVIATION = 2.083e-4
CONFIGS = {'sh': dict(use_superclass=True, ap_with_heading=True), 'nh': dict(use_superclass=False, ap_with_heading=True),
           's_': dict(use_superclass=True, ap_with_heading=False)}


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    return (z,) + kr.unpack_annos(z)


@functools.lru_cache(maxsize=None)
def stated(tag):
    _, g, p = golden()
    return kr.statement(g, p, kr.FIVE, **CONFIGS[tag])


def reference_curves(n_thr, table, pts=51):
    """the reference's own loops on its recorded tp / fp / fn table"""
    K = table.shape[0]
    precision, recall = np.zeros((K, pts)), np.zeros((K, pts))
    with np.errstate(all='ignore'):
        for k in range(K):
            cm = table[k].astype(np.float64)
            for t in range(n_thr[k]):
                recall[k, t] = cm[t, 0] / (cm[t, 0] + cm[t, 2])
                precision[k, t] = cm[t, 0] / (cm[t, 0] + cm[t, 1])
            for t in range(n_thr[k]):
                precision[k, t] = np.max(precision[k, t:], axis=-1)
                recall[k, t] = np.max(recall[k, t:], axis=-1)
    return precision, recall


@pytest.mark.parametrize("tag", list(CONFIGS))
def test_the_statement_equals_the_recorded_reference(tag):
    z, g, p = golden()
    ret_str, ret, st = stated(tag)
    assert np.array_equal(st['flag_gt'], z[tag + '_flag_gt']) and np.array_equal(st['flag_pred'], z[tag + '_flag_pred'])
    assert np.array_equal(st['num_valid'], z[tag + '_num_valid']) and np.array_equal(st['n_thresholds'], z[tag + '_n_thresholds'])
    assert np.array_equal(st['thresholds'].astype(np.float64), z[tag + '_thresholds'])
    assert np.array_equal(st['counts'], z[tag + '_table'])
    precision, recall = reference_curves(z[tag + '_n_thresholds'], z[tag + '_table'])
    K = precision.shape[0]
    assert st['precision'].reshape(K, -1).tobytes() == precision.tobytes() and st['recall'].reshape(K, -1).tobytes() == recall.tobytes()
    assert list(ret) == z[tag + '_ret_keys'].tolist()
    worst = max(abs(float(v) - w) for v, w in zip(ret.values(), z[tag + '_ret_values']))
    print(f"{tag}: largest ret_dict deviation from the reference {worst:.3e}")
    assert worst <= 1e-12
    assert ret_str == str(z[tag + '_text'])
    ious = np.concatenate([o.reshape(-1) for o in st['overlaps']])
    worst = float(np.abs(ious - z[tag + '_ious']).max())
    print(f"{tag}: largest deviation of the statement's overlaps from the reference's fp32 polygon {worst:.3e}")
    assert ious.shape == z[tag + '_ious'].shape and worst <= 4 * BUILDER_IOU_DEVIATION


def test_the_golden_scene_reaches_its_edges():
    _, g, p = golden()
    _, _, st = stated('sh')
    for a, b, (a2, b2) in zip(g, p, zip(*kr.golden_scene())):                             # the fixture holds the seeded scene
        why = []
        assert kr.margins_hold(a, b, why), why
        assert a['name'].tolist() == a2['name'].tolist() and np.array_equal(a['boxes_3d'], a2['boxes_3d'])
        assert b['name'].tolist() == b2['name'].tolist() and np.array_equal(b['boxes_3d'], b2['boxes_3d']) and np.array_equal(b['score'], b2['score'])
    matched = (st['matched'] > -np.inf).sum(axis=1)
    assert matched[0] > 51 > st['n_thresholds'][0]                                       # the rule skips Vehicle scores
    lone = int(np.nonzero(st['num_valid'] == 1)[0][0])
    assert matched[lone] == 1 and st['n_thresholds'][lone] == 51 and len(set(st['thresholds'][lone, :51].tolist())) == 1
    assert (st['thresholds'][lone, 51:] == 0).all()


def _vehicle_by_name(classes, use_superclass, _stated=evaluation.once_name_codes):
    return _stated(classes, False)


def _fp_counts_flag_1_too(kept, flag_pred, assigned):
    return (kept & (flag_pred != -1)[None, :] & ~assigned).sum(axis=1).astype(np.int64)


# each entry states ONE rule of the statement wrongly: (the name in gdmae_hip.evaluation, what stands in its place)
WRONG_RULES = {'vehicle_by_name': ('once_name_codes', _vehicle_by_name),
               'no_heading_fold': ('once_heading_rejected', lambda a, b: abs(float(a) - float(b)) > np.pi / 2),
               'iou_ge': ('once_overlaps_enough', lambda iou, threshold: iou >= threshold),
               'no_eps': ('ONCE_THRESHOLD_EPS', 0.0),
               'fp_counts_ignored': ('once_false_positives', _fp_counts_flag_1_too)}


@pytest.mark.parametrize("mutation", list(WRONG_RULES))
def test_a_wrong_rule_moves_the_golden_table(mutation, monkeypatch):
    """Under the scene's margins no IoU lies at a threshold, so ``>=`` for ``>`` is made visible with a Cyclist threshold of 0: every
    disjoint pair is then a candidate under ``>=`` and none under ``>``."""
    _, g, p = golden()
    options = dict(iou_thresholds={'Vehicle': 0.7, 'Pedestrian': 0.3, 'Cyclist': 0.0}) if mutation == 'iou_ge' else {}
    ret_str, ret = evaluation.once_eval_numpy(g, p, kr.FIVE, bev_overlap=kr.bev_overlap, **options)
    monkeypatch.setattr(evaluation, *WRONG_RULES[mutation])
    bad_str, bad = evaluation.once_eval_numpy(g, p, kr.FIVE, bev_overlap=kr.bev_overlap, **options)
    moved = max(abs(float(ret[k]) - float(bad[k])) for k in ret)
    print(f"{mutation}: the table moves by up to {moved:.2f} AP")
    assert moved >= 0.5 and bad_str != ret_str


def test_both_evaluators_match_by_one_rule():
    """There is one matching rule: on a frame of each golden scene, with the same flags on both sides and no DontCare box, the second
    pass gives the same tp / fp / fn through the KITTI wrapper ((D, G) overlaps, the bound inside) and through the ONCE one."""
    import kitti_eval_reference as kk
    kg, kd = kk.unpack_annos(np.load(os.path.join(os.path.dirname(GOLDEN), "kitti_eval.npz")))
    _, og, op = golden()
    frames = [(kk.frame_overlaps(kg[0], kd[0])[0][2].T, kd[0]['score']),
              (evaluation.once_statement_overlaps(og[0]['boxes_3d'], op[0]['boxes_3d'], True, kr.bev_overlap), op[0]['score'])]
    for ov, score in frames:
        G, P = ov.shape
        score = np.asarray(score, np.float32)
        flag_gt, flag_pred = (np.where(i % 4 == 3, 1, np.where(i % 5 == 4, -1, 0)).astype(np.int8) for i in (np.arange(G), np.arange(P)))
        thresholds = np.sort(score)[::-1][::max(P // 6, 1)]
        for min_ov in (0.25, 0.5):
            tp, fp, fn, _ = evaluation._kitti_second_pass(ov.T, score, None, None, flag_gt, flag_pred, None, min_ov, thresholds, False)
            once = evaluation._once_second_pass(ov, evaluation.once_overlaps_enough(ov, min_ov), score, flag_gt, flag_pred, thresholds)
            assert all(np.array_equal(a, b) for a, b in zip((tp, fp, fn), once))
            assert tp.sum() > 0 and fp.sum() > 0 and fn.sum() > 0 and len(thresholds) > 3


def test_options_and_refusals():
    _, g, p = golden()
    with pytest.raises(AssertionError, match="Car/Bus/Truck must all exist"):
        evaluation.once_eval_numpy(g, p, ['Car', 'Pedestrian'])
    with pytest.raises(AssertionError, match="the number of GT must match predictions"):
        evaluation.once_eval_numpy(g[:2], p[:3], kr.FIVE)
    with pytest.raises(AssertionError, match="difficulty mode is not supported"):
        evaluation.once_eval_numpy(g[:2], p[:2], kr.FIVE, difficulty_mode='Easy')
    for mode, n in (('Overall', 1), ('Distance', 3), ('Overall&Distance', 4)):
        ret_str, ret = evaluation.once_eval_numpy(g[:2], p[:2], kr.FIVE, difficulty_mode=mode, num_pr_points=10, bev_overlap=kr.bev_overlap)
        assert len(ret) == 4 * n and ret_str.startswith("\n|AP@10       |")
    # zero-row annos whatever the dtype of ``name`` (the reference's empty template has a float name); no frames at all
    empty = evaluation.once_annos_template(0)
    ret_str, ret = evaluation.once_eval_numpy([g[0], {'name': np.zeros(0), 'boxes_3d': np.zeros((0, 7))}], [empty, p[1]], kr.FIVE,
                                              bev_overlap=kr.bev_overlap)
    assert all(float(v) == 0 for v in ret.values())
    # 51 copies of the one score; an empty list without a valid GT row and without a true positive
    assert evaluation.once_get_thresholds(np.array([0.5], np.float32), 1, 50) == [np.float32(0.5)] * 51
    assert evaluation.once_get_thresholds(np.zeros(0, np.float32), 0, 50) == [] and evaluation.once_get_thresholds(np.zeros(0, np.float32), 7, 50) == []
    names, accept = evaluation.once_name_codes(['Vehicle', 'Pedestrian', 'Cyclist'], True)
    assert names == ['Pedestrian', 'Cyclist', 'Vehicle'] and accept.tolist() == [0b1100, 0b0001, 0b0010]      # "other" (bit 3) is a Vehicle


def test_the_forwarder_returns_the_statement():
    from pcdet.datasets.once.once_eval import evaluation as shim
    _, g, p = golden()
    ret_str, ret, _ = stated('sh')
    got_str, got = shim.get_evaluation_results(g, p, list(kr.FIVE))
    assert got_str == ret_str and list(got) == list(ret) and max(abs(float(got[k]) - float(ret[k])) for k in ret) <= 1e-12
    assert shim.iou_threshold_dict == {'Car': 0.7, 'Bus': 0.7, 'Truck': 0.7, 'Pedestrian': 0.3, 'Cyclist': 0.5}
    assert shim.superclass_iou_threshold_dict == {'Vehicle': 0.7, 'Pedestrian': 0.3, 'Cyclist': 0.5}


def test_prediction_dicts_equal_the_hand_built_annos():
    rng = np.random.RandomState(5)
    names = ['Car', 'Pedestrian', 'Cyclist']
    samples = [dict(pred_boxes=torch.from_numpy(rng.randn(n, 9).astype(np.float32)), pred_scores=torch.from_numpy(rng.rand(n).astype(np.float32)),
                    pred_labels=torch.from_numpy(rng.randint(1, 4, n))) for n in (4, 0, 2)]
    annos = evaluation.once_prediction_dicts({'frame_id': ['a', 'b', 'c']}, samples, names)
    assert [a['frame_id'] for a in annos] == ['a', 'b', 'c']
    for a, s in zip(annos, samples):
        n = s['pred_scores'].shape[0]
        if n == 0:                                                                       # the reference's empty template
            assert a['name'].shape == (0,) and a['score'].shape == (0,) and a['boxes_3d'].shape == (0, 7)
            continue
        assert a['name'].tolist() == [names[k - 1] for k in s['pred_labels'].tolist()]
        assert a['score'].dtype == np.float32 and np.array_equal(a['score'], s['pred_scores'].numpy())
        assert a['boxes_3d'].dtype == np.float32 and np.array_equal(a['boxes_3d'], s['pred_boxes'].numpy()[:, :7])
    with pytest.raises(NotImplementedError, match="output_path"):
        evaluation.once_prediction_dicts({'frame_id': ['a', 'b', 'c']}, samples, names, output_path="/tmp/x")
