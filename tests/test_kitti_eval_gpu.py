"""GPU: ``gdmae_kitti_eval`` (csrc/kitti_eval.hip) through ``gdmae_hip.evaluation.KittiEval`` / ``kitti_eval``, stage by stage against
the numpy statement ``kitti_eval_numpy`` (fp64 convex clipping) on the scenes of tests/kitti_eval_reference.py.

The crafted scene has 11 frames with 0, 1, 63, 64, 65 and 129 detections (the deciding detection last in its frame) and 0, 1, 2 and 33
GT rows: a frame with GT rows and no detections, one with detections and no GT rows, an empty one; no Cyclist GT row and no Truck
detection anywhere; equal scores on competing detections, an exact copy of a GT box (and a copy of the copy), a pair that differs
by 1e-3 rad of heading, boxes just inside and just outside the centre-distance prefilter, detections over DontCare boxes, a Car
detection on a Van, detections under the height limits.  It is evaluated whole, as its first 1, 7, 8 and 9 frames (the second pass
takes 8 frames per wavefront), with one class and with all six; the golden scene (14 frames, more than 41 matched Car scores) is
evaluated too and compared with the reference's recorded curves.  Every frame keeps the margins asserted in the scene builder, so
matched scores, thresholds, their counts and tp / fp / fn must be EQUAL; overlaps and the similarity sum are compared numerically.

Measured on an MI355X against the fp64 statement, the largest figure over all scenes (every test prints its own):
  overlaps                          7.969e-6 (scene golden)    the fp32 rounding of the annos on upload (a GT location of 90 m is
                                                               4e-6 m off) and of the result; the arithmetic between is fp64
  similarity sum, per (combo, t)    3.454e-8 (scene crafted)   alpha as fp32: 1.2e-7 rad per true positive
  aos AP values (percent)           4.086e-8 (scene golden)
The tests assert 4 x these figures."""
import functools

import numpy as np
import pytest
import torch

import kitti_eval_reference as kr
from gdmae_hip import evaluation
from gdmae_hip import lib as L
from oracle import iou3d_oracle

pytestmark = pytest.mark.gpu

MEASURED_OVERLAP = 7.969e-6
MEASURED_SIM = 3.454e-8
MEASURED_AOS_AP = 4.086e-8
THREE = ['Car', 'Pedestrian', 'Cyclist']


@functools.lru_cache(maxsize=None)
def annos(name):
    if name == 'golden':
        import os
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_eval.npz"))
        return kr.unpack_annos(z) + (THREE,)
    g, d = kr.crafted_scene()
    if name == 'minus_ten':
        return g[:3], [dict(a, alpha=np.full_like(a['alpha'], -10)) for a in d[:3]], THREE
    n, classes = {'crafted': (11, THREE), 'first_1': (1, THREE), 'first_7': (7, THREE), 'first_8': (8, THREE), 'first_9': (9, THREE),
                  'one_class': (11, 'Car'), 'six_classes': (11, list(evaluation.KITTI_CLASS_NAMES))}[name]
    return g[:n], d[:n], classes


SCENES = ['crafted', 'first_1', 'first_7', 'first_8', 'first_9', 'one_class', 'six_classes', 'minus_ten', 'golden']


@functools.lru_cache(maxsize=None)
def solved(name):
    """-> (the statement's (result, ret_dict, stages), the device evaluator): computed once per scene and left unchanged"""
    g, d, classes = annos(name)
    ev = evaluation.KittiEval(g, d, classes, "cuda")
    torch.cuda.synchronize()
    return kr.statement(g, d, classes), ev


def test_the_scene_reaches_its_edges():
    g, d, _ = annos('crafted')
    assert sorted(len(a['name']) for a in d)[:2] == [0, 0] and {1, 63, 64, 65, 129} <= set(len(a['name']) for a in d)
    assert {0, 1, 2, 33} <= set(len(a['name']) for a in g)
    assert any(len(a['name']) and not len(b['name']) for a, b in zip(g, d)) and any(len(b['name']) and not len(a['name']) for a, b in zip(g, d))
    names_g, names_d = set(n for a in g for n in a['name']), set(n for a in d for n in a['name'])
    assert 'Cyclist' in names_d and 'Cyclist' not in names_g and 'Truck' in names_g and 'Truck' not in names_d
    for a, b in zip(g, d):
        why = []
        assert kr.margins_hold(a, b, why), why
    # the nearly aligned pair: the margin variant of the BEV overlap (oracle/iou3d_oracle.py ``overlap``) misses its true IoU by far
    # more than the bound asserted on the overlaps below
    a, b = kr.nearly_aligned_pair(g[0], d[0])
    area = a[3] * a[4] + b[3] * b[4]
    iou = lambda ov: ov / (area - ov)      # noqa: E731
    assert abs(iou(iou3d_oracle.overlap(a, b)) - iou(kr.bev_overlap(a, b))) > 1e-3 > 10 * 4 * MEASURED_OVERLAP
    (_, _, st), _ = solved('crafted')
    cyclist, matched = st['n_thresholds'].reshape(3, 3, 3, 2)[:, 2], (st['matched'] > -np.inf).sum(axis=1)
    assert not cyclist.any() and matched.max() > 8                             # a class without GT rows: no thresholds at all
    (_, _, st6), _ = solved('six_classes')
    truck = st6['n_thresholds'].reshape(3, 6, 3, 2)[:, 5]
    assert not truck.any() and st6['clean']['num_valid'][5].min() > 0         # GT rows, no detection: no thresholds either
    # the deciding (last) detection of the frames with 63, 64, 65 and 129 detections is a true positive of the first pass
    go, do = st['clean']['gt_off'], st['clean']['dt_off']
    last_scores = {f: float(d[f]['score'][-1]) for f in range(len(d)) if len(d[f]['name']) in (63, 64, 65, 129)}
    assert len(last_scores) == 4 and all(float(st['matched'][1, go[f]]) == s for f, s in last_scores.items())


@pytest.mark.parametrize("name", SCENES)
def test_overlaps(name):
    (_, _, st), ev = solved(name)
    worst, do = 0.0, st['clean']['dt_off']
    dc = ev.overlaps()[1].cpu().numpy()
    assert ev.overlaps()[0].shape == (3, ev.NP) and dc.shape == (ev.ND,)
    for f in range(ev.F):
        got = ev.frame_overlaps(f)
        assert got.shape == st['overlaps'][f].shape and got.dtype == np.float32
        if got.size:
            worst = max(worst, float(np.abs(got.astype(np.float64) - st['overlaps'][f]).max()))
            assert ((got == 0) == (st['overlaps'][f] == 0)).all()                # disjoint pairs are exactly 0 on both sides
        if do[f + 1] > do[f]:
            worst = max(worst, float(np.abs(dc[do[f]:do[f + 1]].astype(np.float64) - st['dc_max'][f]).max()))
    print(f"{name}: largest overlap deviation from the fp64 statement {worst:.3e}")
    assert worst <= 4 * MEASURED_OVERLAP


@pytest.mark.parametrize("name", SCENES)
def test_matched_scores_thresholds_and_counts_are_equal(name):
    (_, _, st), ev = solved(name)
    matched = ev.matched_scores().cpu().numpy()
    assert matched.shape == st['matched'].shape == (ev.K, ev.NG) and matched.dtype == np.float32
    for k in range(ev.K):
        assert np.array_equal(np.sort(matched[k]), np.sort(st['matched'][k])), k          # the multiset per combo
    assert np.array_equal(matched, st['matched'])                                         # and slot by slot
    thr, cnt = (t.cpu().numpy() for t in ev.thresholds())
    assert cnt.tolist() == st['n_thresholds'].tolist()
    assert thr.dtype == np.float32 and thr.tobytes() == st['thresholds'].tobytes()
    print(f"{name}: matched scores per combo {(matched > -np.inf).sum(axis=1).tolist()}, thresholds {cnt.tolist()}")


@pytest.mark.parametrize("name", SCENES)
def test_pr_counts_are_equal_and_similarity_within_the_bound(name):
    (_, _, st), ev = solved(name)
    counts, sim = (t.cpu().numpy() for t in ev.pr())
    assert counts.dtype == np.int64 and sim.dtype == np.float64
    assert np.array_equal(counts, st['pr_counts'])
    d = float(np.abs(sim - st['pr_sim']).max())
    print(f"{name}: tp {int(counts[..., 0].sum())} fp {int(counts[..., 1].sum())} fn {int(counts[..., 2].sum())}; similarity deviation {d:.3e}")
    assert d <= 4 * MEASURED_SIM
    assert ev.compute_aos == st['compute_aos'] and (ev.compute_aos or not sim.any())
    assert not sim.reshape(3, -1)[1:].any()                                              # the orientation belongs to the bbox metric
    precision, recall, aos = ev.curves()
    assert np.array_equal(precision, st['precision'], equal_nan=True) and np.array_equal(recall, st['recall'], equal_nan=True)
    assert precision.shape == (3, ev.C, 3, 2, 41) and float(np.nanmax(np.abs(aos - st['aos']))) <= 4 * MEASURED_SIM


@pytest.mark.parametrize("name", SCENES)
def test_result_text_and_ret_dict(name):
    g, d, classes = annos(name)
    (result, ret, st), _ = solved(name)
    detail = {}
    got, got_ret = evaluation.kitti_eval(g, d, classes, PR_detail_dict=detail)
    assert list(got_ret) == list(ret) and len(ret) == (12 if st['compute_aos'] else 9) * (1 if isinstance(classes, str) else len(classes))
    worst = 0.0
    for k in ret:
        if '_aos/' in k:
            worst = max(worst, abs(float(got_ret[k]) - float(ret[k])))
        else:
            assert got_ret[k] == ret[k], k
    print(f"{name}: aos AP deviation {worst:.3e}")
    assert worst <= 4 * MEASURED_AOS_AP
    ours, theirs = got.split("\n"), result.split("\n")
    assert len(ours) == len(theirs)
    for a, b in zip(ours, theirs):
        if a.startswith("aos"):
            assert all(abs(float(x) - float(y)) <= 0.0101 for x, y in zip(a.split(":")[1].split(","), b.split(":")[1].split(","))), (a, b)
        else:
            assert a == b
    assert sorted(detail) == (['3d', 'aos', 'bbox', 'bev'] if st['compute_aos'] else ['3d', 'bbox', 'bev'])
    assert np.array_equal(detail['3d'], st['precision'][2], equal_nan=True)


def test_golden_curves_equal_the_reference():
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_eval.npz"))
    _, ev = solved('golden')
    precision, recall, _ = ev.curves()
    assert np.array_equal(precision, z['ref_precision'], equal_nan=True) and np.array_equal(recall, z['ref_recall'], equal_nan=True)
    cnt = ev.thresholds()[1].cpu().numpy()
    assert ((ev.matched_scores() > -np.inf).sum(dim=1).cpu().numpy() > np.maximum(cnt, 41)).any()          # get_thresholds skipped scores


@pytest.mark.parametrize("name", ['crafted', 'first_9', 'golden'])
def test_two_runs_are_bit_identical(name):
    g, d, classes = annos(name)
    _, ev = solved(name)
    again = evaluation.KittiEval(g, d, classes, "cuda")
    for a, b in zip(ev.overlaps() + (ev.matched_scores(),) + ev.thresholds() + ev.pr(), again.overlaps() + (again.matched_scores(),) + again.thresholds() + again.pr()):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("f", [0, 5, 7, 9])
def test_a_frame_alone_and_inside_the_set(f):
    """overlaps and first-pass matches of a frame do not depend on its neighbours; its tp / fp / fn do not depend on where it sits in
    its chunk of 8 frames (empty frames around it change neither the thresholds nor the counts)"""
    g, d, classes = annos('crafted')
    _, whole = solved('crafted')
    alone = evaluation.KittiEval(g[f:f + 1], d[f:f + 1], classes, "cuda")
    assert alone.frame_overlaps(0).tobytes() == whole.frame_overlaps(f).tobytes()
    go = whole.clean['gt_off']
    assert alone.matched_scores().cpu().numpy().tobytes() == whole.matched_scores()[:, int(go[f]):int(go[f + 1])].contiguous().cpu().numpy().tobytes()
    empty_g, empty_d = {k: v[:0] for k, v in g[f].items()}, {k: v[:0] for k, v in d[f].items()}
    chunk = L.load().gdmae_kitti_eval_frames_per_chunk()
    assert chunk == 8
    for before, after in ((chunk - 1, 0), (chunk, 1), (3, chunk + 2)):
        padded = evaluation.KittiEval([empty_g] * before + [g[f]] + [empty_g] * after, [empty_d] * before + [d[f]] + [empty_d] * after, classes, "cuda")
        for a, b in zip(alone.thresholds() + alone.pr(), padded.thresholds() + padded.pr()):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), (before, after)


def test_bad_sizes_are_refused_before_anything_is_launched():
    lib = L.load()
    off = lambda *v: np.array(v, np.int32)      # noqa: E731

    def refused(stage, n_frames, n_combos, gt_off, dt_off, dc_off, ws_bytes=0):
        h = [None if o is None else o.ctypes.data for o in (gt_off, dt_off, dc_off)]
        rc = lib.gdmae_kitti_eval(stage, n_frames, n_combos, *h, *([None] * 18), 0, *([None] * 9), ws_bytes, None)
        return rc != 0 and b"kitti_eval" in lib.gdmae_last_error()
    ok = off(0, 3)
    assert refused(1, -1, 54, ok, ok, ok) and refused(1, 0, 54, ok, ok, ok)                       # negative / zero frame count
    assert refused(1, 1, 0, ok, ok, ok) and refused(1, 1, 109, ok, ok, ok) and refused(3, 1, 54, ok, ok, ok)
    assert refused(1, 1, 54, off(0, 1025), ok, ok) and refused(1, 1, 54, ok, off(0, 1025), ok)    # beyond the per-frame caps
    assert refused(1, 2, 54, off(0, 3, 2), off(0, 3, 6), off(0, 0, 0))                            # a negative count in a frame
    assert refused(1, 1, 54, ok, off(0, -1), ok) and refused(1, 1, 54, None, ok, ok)
    assert refused(2, 1, 54, ok, ok, ok, ws_bytes=0)                                              # no workspace for the second stage
    g, d, classes = annos('first_1')
    big = {k: np.concatenate([v] * 42) for k, v in d[0].items()}
    assert len(big['name']) > evaluation.KITTI_MAX_ROWS
    with pytest.raises(ValueError, match="kitti_eval"):
        evaluation.KittiEval(g, [big], classes, "cuda")
    for call in (lambda: evaluation.kitti_eval(g, d, classes, device="cpu"), lambda: evaluation.KittiEval(g, d, classes, torch.device("cpu"))):
        with pytest.raises(NotImplementedError, match="kitti_eval"):
            call()


def test_the_shim_runs_on_the_device():
    from pcdet.datasets.kitti.kitti_object_eval_python import eval as shim
    g, d, classes = annos('first_7')
    (result, ret, _), _ = solved('first_7')
    got, got_ret = shim.get_official_eval_result(g, d, classes)
    assert list(got_ret) == list(ret) and got.split("\n")[:4] == result.split("\n")[:4]
