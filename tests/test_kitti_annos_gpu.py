"""GPU: ``gdmae_kitti_annos`` (csrc/kitti_annos.hip) against the numpy statement ``kitti_annos_numpy``, the record
``KittiDetections``, ``KittiEval`` from the record and ``evaluate_kitti`` end to end, on the scenes of tests/kitti_annos_reference.py.

Kernel and statement evaluate the same fp64 expressions in the same order on the same fp32 inputs and round once; only cos, sin and
atan2 come from two libraries (an fp64 ulp apart at most), so an fp32 result can differ by a flipped rounding: every output must be
within 1 fp32 ulp of the statement's, or within 1e-12 where a sum cancels to nearly zero (the fp64 error of operands of 1e2 is
1e-14, far above an fp32 ulp of a result near 0).  Clipped entries, flags, labels, ``score`` and ``boxes_lidar`` must be EQUAL.
Every kernel test prints how many entries differ at all; measured on an MI355X: 0 of the 30,700 fp32 entries of the seven cases."""
import functools
import os

import numpy as np
import pytest
import torch

import kitti_annos_reference as ka
import kitti_eval_reference as kr
from gdmae_hip import evaluation
from gdmae_hip import lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -777.25
FLOAT_KEYS = ('bbox', 'geo', 'alpha', 'score', 'boxes_lidar')
PAD = 5                                                            # rows behind ND in every output buffer


def padded(frames, rows, cols=7, n=None):
    """the layout of ``detect``: rows at or beyond num are NaN / a label that is no class"""
    F, n = len(frames), rows if n is None else n
    boxes = np.full((F, n, cols), np.nan, np.float32)
    scores, labels = np.full((F, n), np.nan, np.float32), np.full((F, n), -12345, np.int64)
    for f, fr in enumerate(frames):
        k = len(fr['scores'])
        boxes[f, :k, :7], scores[f, :k], labels[f, :k] = fr['boxes'], fr['scores'], fr['labels']
        if cols > 7:
            boxes[f, :k, 7:] = 3.5                                 # CenterHead's velocity columns
    up = lambda a: torch.from_numpy(a).to(DEV)      # noqa: E731
    return {'pred_boxes': up(boxes), 'pred_scores': up(scores), 'pred_labels': up(labels),
            'num': up(np.array([len(fr['scores']) for fr in frames], np.int32))}


def calib_rows(frames):
    return torch.from_numpy(np.stack([evaluation.kitti_pack_calib(ka.CALIBS[f['calib']], ka.SHAPES[f['calib']]) for f in frames])).to(DEV)


def sentinel_outputs(nd, C):
    """flat buffers with PAD rows behind ND, filled with a sentinel; the views the entry writes into"""
    flat = {'bbox': torch.full(((nd + PAD) * 4,), SENTINEL, device=DEV), 'geo': torch.full(((nd + PAD) * 7,), SENTINEL, device=DEV),
            'alpha': torch.full((nd + PAD,), SENTINEL, device=DEV), 'score': torch.full((nd + PAD,), SENTINEL, device=DEV),
            'boxes_lidar': torch.full(((nd + PAD) * 7,), SENTINEL, device=DEV), 'label': torch.full((nd + PAD,), -99, dtype=torch.int32, device=DEV),
            'ignored_dt': torch.full((C * 3 * nd + PAD,), 77, dtype=torch.int8, device=DEV)}
    view = {'bbox': flat['bbox'][:nd * 4].view(nd, 4), 'geo': flat['geo'][:nd * 7].view(nd, 7), 'alpha': flat['alpha'][:nd], 'score': flat['score'][:nd],
            'boxes_lidar': flat['boxes_lidar'][:nd * 7].view(nd, 7), 'label': flat['label'][:nd], 'ignored_dt': flat['ignored_dt'][:C * 3 * nd].view(C, 3, nd)}
    return flat, view


def run_kernel(frames, rows, cols, class_names, classes):
    t = padded(frames, rows, cols)
    off = np.concatenate([[0], np.cumsum([len(f['scores']) for f in frames])])
    nd = int(off[-1])
    flat, view = sentinel_outputs(nd, len(classes))
    evaluation.kitti_annos_launch(t['pred_boxes'], t['pred_scores'], t['pred_labels'], t['num'], calib_rows(frames),
                                  torch.from_numpy(off.astype(np.int32)).to(DEV), nd, evaluation.kitti_class_map(class_names), classes, out=view)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in flat.items()}, {k: v.cpu().numpy() for k, v in view.items()}, nd


def expected(frames, class_names, classes):
    annos = [ka.statement(f, class_names) for f in frames]
    full = [a for a in annos if len(a['score'])]
    cat = lambda k, w: np.concatenate([a[k].reshape(-1, w) for a in full] + [np.zeros((0, w), np.float32)], axis=0)      # noqa: E731
    want = {'bbox': cat('bbox', 4), 'geo': np.concatenate([cat('location', 3), cat('dimensions', 3), cat('rotation_y', 1)], axis=1),
            'alpha': cat('alpha', 1)[:, 0], 'score': cat('score', 1)[:, 0], 'boxes_lidar': cat('boxes_lidar', 7),
            'label': np.concatenate([f['labels'] for f in frames] + [np.zeros(0, np.int64)]).astype(np.int32),
            'ignored_dt': evaluation.kitti_clean_dt(annos, classes)['ignored_dt']}
    return want, annos


def within_an_ulp(got, want):
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    return (d <= np.spacing(np.abs(want)).astype(np.float64)) | (d <= 1e-12)


def compare(name, frames, rows, cols, class_names=ka.THREE, classes=None):
    classes = evaluation.kitti_class_ints(class_names) if classes is None else classes
    flat, got, nd = run_kernel(frames, rows, cols, class_names, classes)
    want, _ = expected(frames, class_names, classes)
    differ = total = 0
    for k in FLOAT_KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == np.float32, k
        assert not (got[k] == np.float32(SENTINEL)).any() and np.isfinite(got[k]).all(), k          # every row below ND is written
        ok = within_an_ulp(got[k], want[k])
        assert ok.all(), (name, k, got[k][~ok][:4], want[k][~ok][:4])
        differ, total = differ + int((got[k] != want[k]).sum()), total + got[k].size
    for k in ('score', 'boxes_lidar'):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert np.array_equal(got['geo'][:, 3:6], want['geo'][:, 3:6])
    hi = np.concatenate([np.tile(np.array([[ka.SHAPES[f['calib']][1] - 1, ka.SHAPES[f['calib']][0] - 1] * 2], np.float32), (len(f['scores']), 1))
                         for f in frames] + [np.zeros((0, 4), np.float32)])
    clipped = (want['bbox'] == 0) | (want['bbox'] == hi)
    assert np.array_equal((got['bbox'] == 0) | (got['bbox'] == hi), clipped) and np.array_equal(got['bbox'][clipped], want['bbox'][clipped])
    assert np.array_equal(got['label'], want['label']) and np.array_equal(got['ignored_dt'], want['ignored_dt'])
    # nothing beyond ND
    for k, per_row in (('bbox', 4), ('geo', 7), ('alpha', 1), ('score', 1), ('boxes_lidar', 7)):
        assert (flat[k][nd * per_row:] == np.float32(SENTINEL)).all(), k
    assert (flat['label'][nd:] == -99).all() and (flat['ignored_dt'][len(classes) * 3 * nd:] == 77).all()
    print(f"{name}: ND {nd}, {differ} of {total} fp32 entries differ from the statement's (each by one ulp), {int(clipped.sum())} clipped entries")
    again = run_kernel(frames, rows, cols, class_names, classes)[0]
    for k in flat:
        assert flat[k].tobytes() == again[k].tobytes(), k                                           # two runs are bit-identical
    return got


@functools.lru_cache(maxsize=None)
def frames_of(counts, seed=40):
    """one frame per count with the calibrations in turn; a count of -1 is the crafted frame"""
    return tuple(ka.special_frame() if n < 0 else ka.random_frame(seed + i, n, i % 3) for i, n in enumerate(counts))


CASES = {
    'rows 1, F 3': ((1, 0, 1), 1, 7),
    'rows 65, F 9': ((0, 1, 63, 64, 65, 0, -1, 65, 2), 65, 7),
    'rows 65, F 1': ((64,), 65, 7),
    'rows 65, F 3, 9 columns': ((65, 0, 63), 65, 9),
    'rows 500, F 3': ((500, 0, 65), 500, 7),
    'rows 500, F 1, 9 columns': ((500,), 500, 9),
    'rows 500, F 1, empty': ((0,), 500, 7),
}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_the_statement(name):
    counts, rows, cols = CASES[name]
    compare(name, list(frames_of(counts)), rows, cols)


def test_kernel_reaches_the_edges_and_every_flag():
    frames = list(frames_of((0, 1, 63, 64, 65, 0, -1, 65, 2)))
    assert set().union(*[ka.reached(f) for f in frames]) == ka.EDGES
    assert {f['calib'] for f in frames} == {0, 1, 2}
    got = compare('edges', frames, 65, 7)
    for c in range(3):
        for l in range(3):
            assert set(np.unique(got['ignored_dt'][c, l]).tolist()) == {-1, 0, 1}, (c, l)


def test_another_class_order_and_other_evaluated_classes():
    """labels that mean ['Pedestrian', 'Car'], evaluated as Car alone, as all six KITTI classes and as a class no label means"""
    frames = [ka.random_frame(60, 33, 1, n_classes=2), ka.random_frame(61, 0, 2, n_classes=2), ka.random_frame(62, 20, 0, n_classes=2)]
    for classes in ([0], [0, 1, 2, 3, 4, 5], [2], [1, 0]):
        got = compare(f'swapped names, classes {classes}', frames, 65, 7, class_names=ka.SWAPPED, classes=classes)
    own = got['ignored_dt'][:, 2] == 0                                         # classes [1, 0]: row 0 Pedestrian = label 1
    assert (own[0] <= (got['label'] == 1)).all() and (own[1] <= (got['label'] == 2)).all() and own[0].any() and own[1].any()


def test_a_nan_row_is_nan_on_both_sides():
    """numpy's min, max and clip hand a NaN on, and so does the kernel (fmin / fmax would give a finite clipped box)"""
    frames = [dict(ka.random_frame(63, 5, 0)), ka.random_frame(64, 3, 1)]
    frames[0]['boxes'] = frames[0]['boxes'].copy()
    frames[0]['boxes'][2, 0] = np.nan
    classes = evaluation.kitti_class_ints(ka.THREE)
    _, got, nd = run_kernel(frames, 65, 7, ka.THREE, classes)
    want, _ = expected(frames, ka.THREE, classes)
    assert nd == 8 and np.isnan(want['bbox'][2]).all() and np.isnan(want['geo'][2, :3]).all() and np.isnan(want['alpha'][2])
    for k in ('bbox', 'geo', 'alpha'):
        nan = np.isnan(want[k])
        assert np.array_equal(np.isnan(got[k]), nan) and within_an_ulp(got[k][~nan], want[k][~nan]).all(), k
    assert np.array_equal(got['ignored_dt'], want['ignored_dt']) and nan.sum() == 1


def test_launch_refuses_tensors_that_are_not_contiguous():
    frames = [ka.random_frame(65, 4, 0), ka.random_frame(66, 4, 1)]
    t = padded(frames, 8, cols=9)
    off = torch.tensor([0, 4, 8], dtype=torch.int32, device=DEV)
    args = lambda boxes, scores: (boxes, scores, t['pred_labels'], t['num'], calib_rows(frames), off, 8, [0, 1, 2], [0])      # noqa: E731
    for bad in (args(t['pred_boxes'][..., :7], t['pred_scores']), args(t['pred_boxes'], t['pred_scores'].t().contiguous().t())):
        with pytest.raises(ValueError, match="kitti_annos: a tensor that is not contiguous"):
            evaluation.kitti_annos_launch(*bad)
    assert evaluation.kitti_annos_launch(*args(t['pred_boxes'], t['pred_scores']))['bbox'].shape == (8, 4)


# ------------------------------------------------------------------------------------------------------------------------------
# the record
# ------------------------------------------------------------------------------------------------------------------------------
def host_reads(fn):
    """-> (the result of fn, the synchronising operations torch reports while it runs)"""
    import warnings
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    return out, [str(w.message) for w in seen if "synchroniz" in str(w.message).lower() and "prototype" not in str(w.message).lower()]


def test_finish_makes_exactly_one_host_read():
    gts, frames, _ = ka.eval_scene()
    gts, frames = [gts[1], gts[0], gts[2]], [frames[1], frames[0], frames[2]]      # 0, 13 and 17 detections: the first frame is empty
    out, bd = padded(frames, 30), ka.batch_dict(frames)
    _, control = host_reads(lambda: (out['num'].tolist(), out['num'].tolist()))
    assert len(control) == 2, f"the sync debug mode does not count host reads one by one: {control}"

    def record():
        det = evaluation.KittiDetections(ka.THREE, DEV, rows=30, frames=4)
        det.update(out, bd)
        return det
    record().finish()                                                        # every launch and allocation below has run once
    det = record()
    done, seen = host_reads(det.finish)
    assert len(seen) == 1, seen
    assert done['dt_off'].tolist() == [0, 0, 13, 30]
    (aos, again), seen = host_reads(lambda: (det.compute_aos(), det.finish()))      # decided from what that read brought; cached
    assert aos is True and again is done and seen == []
    _, seen = host_reads(det.to_annos)
    assert len(seen) == 1, seen                                              # "one more read"
    det = record()
    ev, seen = host_reads(lambda: evaluation.KittiEval(gts, det, ka.THREE))
    print(f"KittiEval from a fresh record: {len(seen)} synchronising operations before curves(): the record's one read and the synchronous "
          f"uploads of the GT side and of the combos (DESIGN 7p)")
    assert ev.compute_aos is True and det.finish(ev.classes)['dt_off'].tolist() == [0, 0, 13, 30]


class StubEngine:
    """``detect`` alone, as every engine has it: no model, no anchor plan"""

    def __init__(self, outs):
        self.outs = list(outs)

    def detect(self, batch_dict):
        return self.outs.pop(0)


def test_evaluate_kitti_runs_any_engine_and_widens_for_a_wider_batch():
    gts, frames, _ = ka.eval_scene()
    wide = [dict(f) for f in frames[3:]] + [ka.random_frame(88, 520, 1)]
    gts = gts + [{k: v[:0] for k, v in gts[0].items()}]
    lists, ns = [frames[:3], wide], (17, 520)                                # the second batch is wider than the store's 500 rows
    batches = batches_of(lists, ns, cols=9)
    result, ret, annos = evaluation.evaluate_kitti(StubEngine([b[0] for b in batches]), [b[1] for b in batches], gts, ka.THREE, keep_annos=True)
    det = evaluation.KittiDetections(ka.THREE, DEV, rows=520)
    for out, bd, _ in batches:
        det.update(out, bd)
    want_result, want_ret = evaluation.kitti_eval(gts, det, ka.THREE)
    assert result == want_result and "aos  AP:" in result and list(ret) == list(want_ret)
    assert [len(a['score']) for a in annos] == [len(f['scores']) for f in frames[:3] + wide]
    for a, b in zip(annos, det.to_annos()):
        assert a['frame_id'] == b['frame_id'] and all(np.array_equal(a[k], b[k]) for k in ka.ANNO_KEYS)
    # widen on its own: rows and frames kept, refused by name outside its range
    small = evaluation.KittiDetections(ka.THREE, DEV, rows=17, frames=1)
    small.update(*batches[0][:2])
    small.widen(40)
    assert small.rows == 40 and small.F == 3
    for a, b in zip(small.to_annos(), annos[:3]):
        assert all(np.array_equal(a[k], b[k]) for k in ka.ANNO_KEYS)
    for rows in (40, 1025):
        with pytest.raises(ValueError, match="KittiDetections.widen: rows"):
            small.widen(rows)
    with pytest.raises(ValueError, match="KittiDetections: rows 1025"):
        evaluation.evaluate_kitti(StubEngine([padded([frames[0]], 1025)]), [ka.batch_dict([frames[0]])], gts[:1], ka.THREE)
def batches_of(frame_lists, ns, cols=7):
    out, first = [], 0
    for frames, n in zip(frame_lists, ns):
        out.append((padded(frames, None, cols, n=n), ka.batch_dict(frames, first_id=100 + first), frames))
        first += len(frames)
    return out


def test_record_across_a_store_doubling_equals_the_kernel_per_batch(tmp_path):
    fr = [ka.random_frame(70 + i, n, i % 3) for i, n in enumerate((20, 0, 7, 33, 1, 12, 5))]
    batches = batches_of([fr[:3], fr[3:6], fr[6:]], ns=(20, 33, 7), cols=9)
    det = evaluation.KittiDetections(ka.THREE, DEV, rows=40, frames=2)
    assert det._cap == 2
    caps = []
    for out, bd, _ in batches:
        det.update(out, bd)
        caps.append(det._cap)
    assert caps == [4, 8, 8] and det.F == 7
    done = det.finish()
    assert det.finish() is done                                                 # cached
    assert done['dt_off'].tolist() == np.concatenate([[0], np.cumsum([len(f['scores']) for f in fr])]).tolist()
    annos = det.to_annos()
    assert [a['frame_id'] for a in annos] == ['%06d' % (100 + i) for i in range(7)]
    classes = evaluation.kitti_class_ints(ka.THREE)
    at = 0
    for out, bd, frames in batches:
        _, got, nd = run_kernel(frames, out['pred_scores'].shape[1], 9, ka.THREE, classes)
        off = np.concatenate([[0], np.cumsum([len(f['scores']) for f in frames])])
        for i, f in enumerate(frames):
            a, rows = annos[at + i], slice(int(off[i]), int(off[i + 1]))
            if len(f['scores']) == 0:
                assert all(a[k].shape[0] == 0 and a[k].dtype == np.float64 for k in ka.ANNO_KEYS)
                continue
            for k, want in (('bbox', got['bbox'][rows]), ('location', got['geo'][rows, 0:3]), ('dimensions', got['geo'][rows, 3:6]),
                            ('rotation_y', got['geo'][rows, 6]), ('alpha', got['alpha'][rows]), ('score', got['score'][rows]),
                            ('boxes_lidar', got['boxes_lidar'][rows])):
                assert a[k].dtype == np.float32 and a[k].tobytes() == np.ascontiguousarray(want).tobytes(), k
            assert a['name'].tolist() == [ka.THREE[k - 1] for k in f['labels']]
            assert not a['truncated'].any() and not a['occluded'].any()
        at += len(frames)
    # an update invalidates what finish cached
    det.update(*batches[0][:2])
    assert det.F == 10 and det.finish() is not done and len(det.to_annos()) == 10
    # the label files: the reference's format on the record's own values
    det.write_label_files(tmp_path)
    for a in det.to_annos():
        lines = open(os.path.join(tmp_path, a['frame_id'] + '.txt')).read().split('\n')
        want = [' '.join([str(a['name'][i]), '-1', '-1'] + ['%.4f' % v for v in (
            a['alpha'][i], *a['bbox'][i], a['dimensions'][i][1], a['dimensions'][i][2], a['dimensions'][i][0], *a['location'][i], a['rotation_y'][i],
            a['score'][i])]) for i in range(len(a['score']))]
        assert lines == want + ['']


def test_record_refuses_by_name_before_any_copy():
    frames = [ka.random_frame(80, 9, 0)]
    det = evaluation.KittiDetections(ka.THREE, DEV, rows=8, frames=1)
    det._store['num'].fill_(-5)
    with pytest.raises(ValueError, match="KittiDetections.update: n 9 rows"):
        det.update(padded(frames, 9), ka.batch_dict(frames))
    assert det.F == 0 and det.frame_ids == [] and det._store['num'].tolist() == [-5]
    with pytest.raises(ValueError, match="KittiDetections: rows 1025"):
        evaluation.KittiDetections(ka.THREE, DEV, rows=1025)
    ok = evaluation.KittiDetections(ka.THREE, DEV, rows=9)                    # n <= rows is accepted
    ok.update(padded(frames, 9), ka.batch_dict(frames))
    assert ok.finish()['dt_off'].tolist() == [0, 9]
    with pytest.raises(ValueError, match="GT annos"):
        evaluation.KittiEval([], ok, ka.THREE)


def test_update_makes_no_host_read():
    frames = [ka.random_frame(81 + i, n, i % 3) for i, n in enumerate((12, 0, 30))]
    out, bd = padded(frames, 30), ka.batch_dict(frames)
    det = evaluation.KittiDetections(ka.THREE, DEV, rows=30, frames=8)
    det.update(out, bd)
    uploaded = dict(bd, image_shape=torch.from_numpy(bd['image_shape']).to(DEV))               # an image_shape already on the device
    torch.cuda.synchronize()
    mode, control = torch.cuda.get_sync_debug_mode(), False
    try:
        torch.cuda.set_sync_debug_mode("error")
        det.update(out, bd)
        det.update(out, uploaded)
        try:
            out['num'].tolist()
        except RuntimeError:
            control = True
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert control, "torch.cuda.set_sync_debug_mode('error') did not raise on a host read: the check above proves nothing"
    annos = det.to_annos()
    assert len(annos) == 9
    for i in range(3):
        for k in ka.ANNO_KEYS:
            assert np.array_equal(annos[i][k], annos[3 + i][k]) and np.array_equal(annos[i][k], annos[6 + i][k]), k


def test_prediction_dicts_on_device_tensors():
    frames = [ka.random_frame(90 + i, n, i % 3) for i, n in enumerate((14, 0, 3))]
    bd = ka.batch_dict(frames)
    pred = [{'pred_boxes': torch.from_numpy(f['boxes']).to(DEV), 'pred_scores': torch.from_numpy(f['scores']).to(DEV),
             'pred_labels': torch.from_numpy(f['labels']).to(DEV)} for f in frames]
    got = evaluation.kitti_prediction_dicts(bd, pred, ka.THREE)
    cpu = evaluation.kitti_prediction_dicts(bd, [{k: v.cpu() for k, v in d.items()} for d in pred], ka.THREE)
    assert [a['frame_id'] for a in got] == [a['frame_id'] for a in cpu] == bd['frame_id']
    for a, b in zip(got, cpu):
        assert sorted(a) == sorted(b)
        for k in ka.ANNO_KEYS:
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
            if k == 'name':
                assert a[k].tolist() == b[k].tolist()
            elif len(a['score']):
                assert within_an_ulp(a[k], b[k]).all(), k


# ------------------------------------------------------------------------------------------------------------------------------
# the evaluator from the record
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def evaluated():
    gts, frames, annos = ka.eval_scene()
    det = evaluation.KittiDetections(ka.THREE, DEV, rows=32)
    det.update(padded(frames, 32), ka.batch_dict(frames))
    from_record = evaluation.KittiEval(gts, det, ka.THREE)
    from_annos = evaluation.KittiEval(gts, det.to_annos(), ka.THREE)
    torch.cuda.synchronize()
    return gts, annos, det, from_record, from_annos


def test_evaluator_scene_keeps_the_margins():
    gts, annos, det, _, _ = evaluated()
    assert any(len(g['name']) and not len(a['score']) for g, a in zip(gts, annos)) and any(len(a['score']) and not len(g['name']) for g, a in zip(gts, annos))
    for g, a, d in zip(gts, annos, det.to_annos()):
        for dt in (a, d):                                                     # the statement's annos and the device's
            why = []
            assert kr.margins_hold(g, dict(dt, name=np.asarray(dt['name'], dtype='<U10')), why), why


def test_evaluator_from_the_record_is_bit_identical_to_the_one_from_its_annos():
    gts, _, det, a, b = evaluated()
    assert a.compute_aos is True and b.compute_aos is True and a.ND == b.ND > 0 and a.NP == b.NP > 0
    assert np.array_equal(a.clean['dt_off'], b.clean['dt_off'])
    assert np.array_equal(det.finish(a.classes)['ignored_dt'].cpu().numpy(), b.clean['ignored_dt'])
    for what, x, y in zip(('overlaps', 'dc_max', 'matched scores', 'thresholds', 'threshold counts', 'tp / fp / fn', 'similarity sums'),
                          a.overlaps() + (a.matched_scores(),) + a.thresholds() + a.pr(), b.overlaps() + (b.matched_scores(),) + b.thresholds() + b.pr()):
        assert x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), what
    ra, rb = evaluation.kitti_eval(gts, det, ka.THREE), evaluation.kitti_eval(gts, det.to_annos(), ka.THREE)
    assert ra[0] == rb[0] and "aos  AP:" in ra[0] and list(ra[1]) == list(rb[1]) and all(ra[1][k] == rb[1][k] for k in ra[1])


def test_evaluator_counts_equal_the_numpy_evaluator_on_the_statements_annos():
    gts, annos, _, a, _ = evaluated()
    _, _, st = kr.statement(gts, annos, ka.THREE)
    counts = a.pr()[0].cpu().numpy()
    assert np.array_equal(counts, st['pr_counts']) and counts[..., 0].sum() > 20
    assert a.thresholds()[1].cpu().numpy().tolist() == st['n_thresholds'].tolist()
    assert a.thresholds()[0].cpu().numpy().tobytes() == st['thresholds'].tobytes()          # the thresholds are copied scores
    print(f"evaluator from the record: tp {int(counts[..., 0].sum())} fp {int(counts[..., 1].sum())} fn {int(counts[..., 2].sum())}")


def test_one_class_evaluated_from_a_record_of_three():
    gts, annos, det, _, _ = evaluated()
    a, b = evaluation.kitti_eval(gts, det, 'Pedestrian'), evaluation.kitti_eval(gts, det.to_annos(), 'Pedestrian')
    assert a[0] == b[0] and a[0].startswith("Pedestrian AP@0.50")


# ------------------------------------------------------------------------------------------------------------------------------
# end to end (the model and the batch of tests/test_inference_engine_kitti.py, as tests/test_anchor_detect_gpu.py uses them)
# ------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_kitti_equals_kitti_eval_on_the_prediction_dicts():
    from gdmae_hip import inference
    from test_inference_engine_kitti import _batch, _model
    net, ds = _model()
    eng = inference.compile_detector(net)
    names = list(ds.class_names)
    batches = []
    for i, seed in enumerate((77, 78)):
        bd = _batch(ds, seed=seed)
        bd.update(calib=[ka.CALIBS[(2 * i + b) % 3] for b in range(2)], frame_id=['%06d' % (2 * i + b) for b in range(2)],
                  image_shape=np.array([ka.SHAPES[(2 * i + b) % 3] for b in range(2)], np.int32))
        batches.append(bd)
    # the reference's route, batch by batch; GT annos: every frame's twelve best detections over 45 px, so that the table is not empty
    want_annos = []
    for bd in batches:
        want_annos += evaluation.kitti_prediction_dicts(bd, net.padded_to_pred_dicts(eng.detect(dict(bd))), names)
    gts = []
    for a in want_annos:
        tall = np.nonzero(a['bbox'][:, 3] - a['bbox'][:, 1] > 45)[0]            # valid at every difficulty
        top = tall[np.argsort(-a['score'][tall], kind='stable')[:12]]
        g = {k: a[k][top] for k in ('name', 'alpha', 'bbox', 'dimensions', 'location', 'rotation_y')}
        gts.append(dict(g, truncated=np.zeros(len(top)), occluded=np.zeros(len(top), np.int64)))
    # detect's outputs are untouched by update
    out = eng.detect(dict(batches[0]))
    before = {k: v.clone() for k, v in out.items()}
    det = evaluation.KittiDetections(names, out['pred_scores'].device, rows=net.batched_rows())
    det.update(out, batches[0])
    det.finish()
    assert all(torch.equal(out[k], before[k]) for k in before) and sorted(out) == sorted(before)
    # the loop with the record against that route
    result, ret, annos = evaluation.evaluate_kitti(eng, [dict(bd) for bd in batches], gts, names, keep_annos=True)
    want_result, want_ret = evaluation.kitti_eval(gts, want_annos, names)
    assert np.nanmax(np.array([float(v) for v in want_ret.values()])) > 0
    assert sum(len(a['score']) for a in annos) > 0 and len(annos) == len(want_annos) == 4
    for a, b in zip(annos, want_annos):
        assert a['frame_id'] == b['frame_id']
        for k in ka.ANNO_KEYS:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert result == want_result and list(ret) == list(want_ret) and all(ret[k] == want_ret[k] or (ret[k] != ret[k] and want_ret[k] != want_ret[k]) for k in ret)
    assert evaluation.evaluate_kitti(eng, [dict(bd) for bd in batches], gts, names)[2] is None
    best = max((k for k in ret if ret[k] == ret[k]), key=lambda k: ret[k])
    print(f"end to end: {[len(a['score']) for a in annos]} detections per frame, {sorted(set(n for a in annos for n in a['name']))}; {best} = {ret[best]:.4f}")
