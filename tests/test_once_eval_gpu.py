"""GPU: ``gdmae_once_eval`` (csrc/once_eval.hip) through ``gdmae_hip.evaluation.OnceEval`` / ``once_eval``, stage by stage against the
numpy statement ``once_eval_numpy`` (fp64 convex clipping) on the scenes of tests/once_eval_reference.py.

The crafted scene has 11 frames with 0, 1, 63, 64, 65 and 129 predictions (the deciding prediction last in its frame) and 0, 1, 2 and
33 GT rows: a frame with GT rows and no predictions, one with predictions and no GT rows, an empty one; no Cyclist GT row and no
Truck prediction anywhere; an unknown GT name; equal scores on competing predictions, an exact copy of a GT box (and a copy of the
copy), a flag-1 prediction that is the only candidate of a flag-0 GT row, rows at 29.99 / 30.01 / 49.99 / 50.01 m, boxes just inside
and just outside the circle prefilter, a zero-volume pair; heading differences just under and just over pi / 2, just over pi, above
2.5 pi, and 1e-3 rad.  It is evaluated whole, as its first 1, 7, 8 and 9 frames (the second pass takes 8 frames per wavefront), with
and without the superclass rule, with and without the heading rule, in all three difficulty modes, with 50 and 10 PR points and with
a single class; the golden scene (14 frames, more than 51 matched Vehicle scores) is evaluated too, in the three recorded
configurations, and compared with the reference's recorded tables.  Every frame keeps the margins asserted in the scene builder, so
flags, matched scores, thresholds, their counts and tp / fp / fn must be EQUAL; the overlaps are compared numerically.

Measured on an MI355X against the fp64 statement, the largest figure over all scenes (every test prints its own):
  overlaps                          2.972e-8 (crafted and golden; first_1 2.715e-8, first_7 / first_8 2.935e-8): the fp32 rounding
                                    of the result (half an ulp below 1 is 2.98e-8); boxes are fp32 on both sides and the
                                    arithmetic between is fp64
  ret_dict                          0.0 in every run
The test asserts 4 x the overlap figure."""
import functools
import os

import numpy as np
import pytest
import torch

import once_eval_reference as kr
from gdmae_hip import evaluation
from gdmae_hip import lib as L

pytestmark = pytest.mark.gpu

MEASURED_OVERLAP = 2.972e-8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "once_eval.npz")
RUNS = {'crafted': (11, {}), 'first_1': (1, {}), 'first_7': (7, {}), 'first_8': (8, {}), 'first_9': (9, {}),
        'no_superclass': (11, dict(use_superclass=False)), 'no_heading': (11, dict(ap_with_heading=False)),
        'overall': (11, dict(difficulty_mode='Overall')), 'distance': (11, dict(difficulty_mode='Distance')),
        'pr10': (11, dict(num_pr_points=10)), 'one_class': (11, dict(use_superclass=False, classes=['Pedestrian']))}
GOLDEN_RUNS = {'golden': ('sh', dict(use_superclass=True, ap_with_heading=True)), 'golden_nh': ('nh', dict(use_superclass=False, ap_with_heading=True)),
               'golden_s_': ('s_', dict(use_superclass=True, ap_with_heading=False))}
SCENES = list(RUNS) + list(GOLDEN_RUNS)


@functools.lru_cache(maxsize=None)
def annos(name):
    """-> (gt_annos, pred_annos, classes, options)"""
    if name in GOLDEN_RUNS:
        return kr.unpack_annos(np.load(GOLDEN)) + (kr.FIVE, GOLDEN_RUNS[name][1])
    g, p = kr.crafted_scene()
    n, options = RUNS[name]
    options = dict(options)
    return g[:n], p[:n], options.pop('classes', kr.FIVE), options


@functools.lru_cache(maxsize=None)
def solved(name):
    """-> (the statement's (ret_str, ret_dict, stages), the device evaluator): computed once per scene and left unchanged"""
    g, p, classes, options = annos(name)
    ev = evaluation.OnceEval(g, p, classes, "cuda", **options)
    torch.cuda.synchronize()
    return kr.statement(g, p, classes, **options), ev


def test_the_scene_reaches_its_edges():
    g, p, _, _ = annos('crafted')
    assert len(g) == 11 and L.load().gdmae_once_eval_frames_per_chunk() == 8                 # the subsets above are c - 1, c, c + 1
    assert {0, 1, 63, 64, 65, 129} <= set(len(a['name']) for a in p) and {0, 1, 2, 33} <= set(len(a['name']) for a in g)
    sizes = [(len(a['name']), len(b['name'])) for a, b in zip(g, p)]
    assert (0, 0) in sizes and any(a and not b for a, b in sizes) and any(b and not a for a, b in sizes)
    names_g, names_p = set(n for a in g for n in a['name']), set(n for a in p for n in a['name'])
    assert 'Cyclist' in names_p and 'Cyclist' not in names_g and 'Truck' in names_g and 'Truck' not in names_p and 'Tricycle' in names_g
    for a, b in zip(g, p):
        why = []
        assert kr.margins_hold(a, b, why), why
    (_, _, st), _ = solved('crafted')
    go, po = st['gt_off'], st['pred_off']
    # the deciding (last) prediction of the frames with 63, 64, 65 and 129 predictions is a true positive of the first pass (overall)
    for f in range(11):
        if len(p[f]['name']) in (63, 64, 65, 129):
            c = 0 if p[f]['name'][-1] != 'Pedestrian' else 1
            assert float(st['matched'][c * 4, go[f + 1] - 1]) == float(p[f]['score'][-1]), f
    # frame 8: the distances, the flag-1 only candidate, equal scores, the copies, the prefilter, the zero-volume pair
    b8 = kr.evaluation.once_boxes([g[8]]).astype(np.float64)
    dist = np.sqrt((b8[:4, :3] ** 2).sum(axis=1))
    assert np.abs(dist - [29.99, 30.01, 49.99, 50.01]).max() < 1e-4 and st['flag_gt'][0, 1:, go[8]:go[8] + 4].tolist() == [
        [0, 1, 1, 1], [1, 0, 0, 1], [1, 1, 1, 0]]
    assert st['flag_gt'][0, 1, go[8] + 4] == 0 and st['flag_pred'][0, 1, po[8] + 4] == 1 and st['overlaps'][8][4, 4] > 0.7
    assert st['matched'][0, go[8] + 4] > 0 and st['matched'][1, go[8] + 4] == -np.inf          # a true positive overall, "assigned only" below 30 m
    sc8 = p[8]['score']
    assert sc8[5] == sc8[6] and min(st['overlaps'][8][5, 5:7]) > 0.3 and st['matched'][4, go[8] + 5] == sc8[5]
    assert np.array_equal(p[8]['boxes_3d'][7], p[8]['boxes_3d'][8]) and np.array_equal(p[8]['boxes_3d'][7], g[8]['boxes_3d'][6].astype(np.float32))
    inside, outside = st['overlaps'][8][7, 9], st['overlaps'][8][7, 10]
    d = [np.hypot(*(b8[7, :2] - p[8]['boxes_3d'][j, :2])) - np.hypot(b8[7, 3], b8[7, 4]) - 1e-3 for j in (9, 10)]
    assert -2e-2 < d[0] < 0 < d[1] < 2e-2 and outside == 0 and 0 < inside < 1e-4              # the corners overlap by millimetres
    # the statement proper, without the helper's circle shortcut: the exact clipping says 0 outside the prefilter and > 0 inside
    from pcdet.models.roi_heads import proposal_targets as pt
    turned = lambda b: [float(v) for v in b[:6]] + [-float(b[6])]      # noqa: E731
    exact = [pt.exact_bev_overlap(turned(b8[7]), turned(np.asarray(p[8]['boxes_3d'][j], np.float64))) for j in (9, 10)]
    assert exact[1] == 0.0 and 0 < exact[0] < 1e-3
    assert g[8]['boxes_3d'][8, 5] == 0 and p[8]['boxes_3d'][11, 5] == 0 and st['overlaps'][8][8, 11] == 0
    # frame 9: the heading rule decides (the statement without it has all five pairs far above 0.7)
    (_, _, plain), _ = solved('no_heading')
    own = np.diag(st['overlaps'][9])
    assert (np.diag(plain['overlaps'][9]) > 0.8).all() and (own > 0.8).tolist() == [True, False, False, True, True]
    rot = g[9]['boxes_3d'][:, 6] - p[9]['boxes_3d'][:, 6].astype(np.float64)
    assert abs(rot[3]) > 2.5 * np.pi and abs(abs(rot[4]) - 1e-3) < 1e-6 and 0 < abs(rot[2]) - np.pi < 3e-3
    assert (st['n_thresholds'].reshape(3, 4)[2] == 0).all() and (st['matched'] > -np.inf).sum(axis=1).max() > 8
    (_, _, st5), _ = solved('no_superclass')
    assert not st5['n_thresholds'].reshape(5, 4)[2].any() and st5['num_valid'].reshape(5, 4)[2, 0] > 0      # Truck: GT rows, no prediction


@pytest.mark.parametrize("name", SCENES)
def test_overlaps(name):
    (_, _, st), ev = solved(name)
    worst = 0.0
    assert ev.overlaps().shape == (ev.NP,) and ev.overlaps().dtype == torch.float32
    for f in range(ev.F):
        got = ev.frame_overlaps(f)
        assert got.shape == st['overlaps'][f].shape and got.dtype == np.float32
        if got.size:
            worst = max(worst, float(np.abs(got.astype(np.float64) - st['overlaps'][f]).max()))
            assert ((got == 0) == (st['overlaps'][f] == 0)).all()            # disjoint and heading-rejected pairs: exactly 0 on both sides
    print(f"{name}: largest overlap deviation from the fp64 statement {worst:.3e}")
    assert worst <= 4 * MEASURED_OVERLAP


@pytest.mark.parametrize("name", SCENES)
def test_flags_matched_scores_thresholds_and_counts_are_equal(name):
    (_, _, st), ev = solved(name)
    fg, fp = (t.cpu().numpy() for t in ev.flags())
    assert fg.dtype == np.int8 and np.array_equal(fg, st['flag_gt']) and np.array_equal(fp, st['flag_pred'])
    matched = ev.matched_scores().cpu().numpy()
    assert matched.shape == st['matched'].shape == (ev.K, ev.NG) and matched.dtype == np.float32
    for k in range(ev.K):
        assert np.array_equal(np.sort(matched[k]), np.sort(st['matched'][k])), k          # the multiset per combo
    assert np.array_equal(matched, st['matched'])                                         # and slot by slot
    thr, cnt, nv = (t.cpu().numpy() for t in ev.thresholds())
    assert cnt.tolist() == st['n_thresholds'].tolist() and nv.tolist() == st['num_valid'].tolist()
    assert thr.dtype == np.float32 and thr.tobytes() == st['thresholds'].tobytes()
    counts = ev.counts().cpu().numpy()
    assert counts.dtype == np.int64 and np.array_equal(counts, st['counts'])
    precision, recall = ev.curves()
    assert np.array_equal(precision, st['precision'], equal_nan=True) and np.array_equal(recall, st['recall'], equal_nan=True)
    assert precision.shape == (ev.C, ev.B, ev.num_pr_points + 1)
    print(f"{name}: matched scores per combo {(matched > -np.inf).sum(axis=1).tolist()}, thresholds {cnt.tolist()}; "
          f"tp {int(counts[..., 0].sum())} fp {int(counts[..., 1].sum())} fn {int(counts[..., 2].sum())}")


@pytest.mark.parametrize("name", SCENES)
def test_result_text_and_ret_dict(name):
    g, p, classes, options = annos(name)
    (ret_str, ret, _), _ = solved(name)
    got_str, got = evaluation.once_eval(g, p, classes, **options)
    assert list(got) == list(ret)
    worst = max(abs(float(got[k]) - float(ret[k])) for k in ret)
    print(f"{name}: largest ret_dict deviation {worst:.3e}")
    assert worst <= 1e-12                      # the curves are equal bit for bit and summed in one order: fp64 round-off of <= 63 terms
    assert got_str == ret_str


@pytest.mark.parametrize("name", list(GOLDEN_RUNS))
def test_golden_table_equals_the_reference(name):
    z, tag = np.load(GOLDEN), GOLDEN_RUNS[name][0]
    _, ev = solved(name)
    fg, fp = (t.cpu().numpy() for t in ev.flags())
    assert np.array_equal(fg, z[tag + '_flag_gt']) and np.array_equal(fp, z[tag + '_flag_pred'])
    thr, cnt, nv = (t.cpu().numpy() for t in ev.thresholds())
    assert np.array_equal(nv, z[tag + '_num_valid']) and np.array_equal(cnt, z[tag + '_n_thresholds'])
    assert np.array_equal(thr.astype(np.float64), z[tag + '_thresholds']) and np.array_equal(ev.counts().cpu().numpy(), z[tag + '_table'])
    ret_str, ret = ev.result()
    assert ret_str == str(z[tag + '_text']) and list(ret) == z[tag + '_ret_keys'].tolist()
    assert max(abs(float(v) - w) for v, w in zip(ret.values(), z[tag + '_ret_values'])) <= 1e-12
    if tag == 'sh':
        assert (ev.matched_scores()[0] > -np.inf).sum().item() > 51 > cnt[0]             # get_thresholds skipped Vehicle scores


@pytest.mark.parametrize("name", ['crafted', 'first_9', 'golden'])
def test_two_runs_are_bit_identical(name):
    g, p, classes, options = annos(name)
    _, ev = solved(name)
    again = evaluation.OnceEval(g, p, classes, "cuda", **options)
    stages = lambda e: (e.overlaps(),) + e.flags() + (e.matched_scores(),) + e.thresholds() + (e.counts(),)      # noqa: E731
    for a, b in zip(stages(ev), stages(again)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("f", [0, 1, 8, 9])
def test_a_frame_alone_and_inside_the_set(f):
    """overlaps, flags and first-pass matches of a frame do not depend on its neighbours"""
    g, p, classes, _ = annos('crafted')
    _, whole = solved('crafted')
    alone = evaluation.OnceEval(g[f:f + 1], p[f:f + 1], classes, "cuda")
    assert alone.frame_overlaps(0).tobytes() == whole.frame_overlaps(f).tobytes()
    go, po = whole.gt_off, whole.pred_off
    for a, w, off in zip(alone.flags(), whole.flags(), (go, po)):
        assert a.cpu().numpy().tobytes() == w[:, :, int(off[f]):int(off[f + 1])].contiguous().cpu().numpy().tobytes()
    assert alone.matched_scores().cpu().numpy().tobytes() == whole.matched_scores()[:, int(go[f]):int(go[f + 1])].contiguous().cpu().numpy().tobytes()


def test_bad_sizes_are_refused_before_anything_is_launched():
    lib = L.load()
    off = lambda *v: np.array(v, np.int32)      # noqa: E731

    def refused(stage, n_frames, n_classes, mode, npp, gt_off, pred_off, ws_bytes=0):
        h = [None if o is None else o.ctypes.data for o in (gt_off, pred_off)]
        rc = lib.gdmae_once_eval(stage, n_frames, n_classes, mode, npp, 1, *h, *([None] * 20), ws_bytes, None)
        return rc != 0 and b"once_eval" in lib.gdmae_last_error()
    ok = off(0, 3)
    assert refused(1, -1, 3, 2, 50, ok, ok) and refused(1, 0, 3, 2, 50, ok, ok) and refused(3, 1, 3, 2, 50, ok, ok)
    assert refused(1, 1, 0, 2, 50, ok, ok) and refused(1, 1, 33, 2, 50, ok, ok) and refused(1, 1, 3, 3, 50, ok, ok)
    assert refused(1, 1, 3, 2, 64, ok, ok) and refused(1, 1, 3, 2, 0, ok, ok)
    assert refused(1, 1, 3, 2, 50, off(0, 1025), ok) and refused(1, 1, 3, 2, 50, ok, off(0, 1025))
    assert refused(1, 2, 3, 2, 50, off(0, 3, 2), off(0, 3, 6)) and refused(1, 1, 3, 2, 50, None, ok)
    assert refused(2, 1, 3, 2, 50, ok, ok, ws_bytes=0)                                              # no workspace for the second stage
    g, p, classes, _ = annos('first_1')
    big = {k: np.concatenate([v] * 1025) for k, v in p[0].items()}
    assert len(big['name']) == 1025
    with pytest.raises(ValueError, match="once_eval: a frame with 1025 predictions"):
        evaluation.OnceEval(g, [big], classes, "cuda")
    with pytest.raises(ValueError, match="once_eval: num_pr_points 64"):
        evaluation.once_eval(g, p, classes, num_pr_points=64)
    for call in (lambda: evaluation.once_eval(g, p, classes, device="cpu"), lambda: evaluation.OnceEval(g, p, classes, torch.device("cpu"))):
        with pytest.raises(NotImplementedError, match="once_eval"):
            call()


def test_the_shim_runs_on_the_device():
    from pcdet.datasets.once.once_eval import evaluation as shim
    g, p, classes, _ = annos('first_7')
    (ret_str, ret, _), _ = solved('first_7')
    got_str, got = shim.get_evaluation_results(g, p, list(classes))
    assert got_str == ret_str and list(got) == list(ret)
    assert shim.iou_threshold_dict['Pedestrian'] == 0.3 and shim.superclass_iou_threshold_dict['Vehicle'] == 0.7
