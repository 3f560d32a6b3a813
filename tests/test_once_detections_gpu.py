"""GPU: ``OnceDetections`` / ``once_prediction_dicts`` / ``evaluate_once`` (gdmae_hip/evaluation.py): the padded output of
``detect`` as a device record, its annos, and the AP table computed from the record without a host copy of the predictions.

Host reads: ``update`` none; ``counts`` one; ``OnceEval`` from a record whose counts are known none until ``curves``;
``curves`` one; ``to_annos`` one more."""
import warnings

import numpy as np
import pytest
import torch

import once_eval_reference as kr
from gdmae_hip import evaluation

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = ['Car', 'Bus', 'Truck', 'Pedestrian', 'Cyclist']


def padded(p_annos, n, cols=7):
    """the hand-made ``detect`` output of a list of prediction annos: zero rows beyond ``num[b]``"""
    B = len(p_annos)
    boxes, scores, labels = np.zeros((B, n, cols), np.float32), np.zeros((B, n), np.float32), np.zeros((B, n), np.int64)
    for b, a in enumerate(p_annos):
        k = len(a['name'])
        boxes[b, :k, :7], scores[b, :k] = a['boxes_3d'], a['score']
        boxes[b, :k, 7:] = 5.0
        labels[b, :k] = [NAMES.index(x) + 1 for x in a['name']]
    up = lambda a: torch.from_numpy(a).to(DEV)      # noqa: E731
    return {'pred_boxes': up(boxes), 'pred_scores': up(scores), 'pred_labels': up(labels),
            'num': up(np.array([len(a['name']) for a in p_annos], np.int32))}


def scene():
    """the golden scene with every prediction named by one of the five classes (a label has no unknown name)"""
    g, p = kr.unpack_annos(np.load(kr.__file__.replace("once_eval_reference.py", "golden/once_eval.npz")))
    order = [3, 4, 0, 1, 2, 5, 6]                           # 21 and 25 predictions first: the second batch (up to 31) needs ``widen``
    return [g[f] for f in order], [p[f] for f in order]


def batches():
    g, p = scene()
    parts = [p[0:2], p[2:5], p[5:7]]
    return g, p, [(padded(q, max(len(a['name']) for a in q), cols=9 if i == 1 else 7), {'frame_id': ['f%d' % (len(sum(parts[:i], [])) + j) for j in range(len(q))]})
                  for i, q in enumerate(parts)]


def record(bs=None):
    bs = batches()[2] if bs is None else bs
    det = None
    for i, (out, bd) in enumerate(bs):
        n = out['pred_scores'].shape[1]
        if det is None:
            det = evaluation.OnceDetections(NAMES, DEV, rows=n, frames=2)
        elif n > det.rows:
            det.widen(n)
        det.update(out, bd)
    return det


def host_reads(fn):
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


def test_the_record_needs_a_widen_and_its_annos_equal_the_prediction_dicts():
    g, p, bs = batches()
    widths = [out['pred_scores'].shape[1] for out, _ in bs]
    assert max(widths[1:]) > widths[0], widths                                            # one of the three updates needs ``widen``
    det = record()
    assert det.F == 7 and det.rows == max(widths) and det.counts().tolist() == [len(a['name']) for a in p]
    annos = det.to_annos()
    per_sample = [dict(pred_boxes=out['pred_boxes'][b, :int(out['num'][b])], pred_scores=out['pred_scores'][b, :int(out['num'][b])],
                       pred_labels=out['pred_labels'][b, :int(out['num'][b])]) for out, _ in bs for b in range(out['num'].shape[0])]
    want = evaluation.once_prediction_dicts({'frame_id': ['f%d' % i for i in range(7)]}, per_sample, NAMES)
    for a, b, src in zip(annos, want, p):
        assert a['frame_id'] == b['frame_id'] and a['name'].tolist() == b['name'].tolist() == src['name'].tolist()
        for k in ('score', 'boxes_3d'):
            assert a[k].dtype == b[k].dtype == np.float32 and np.array_equal(a[k], b[k]) and np.array_equal(a[k], src[k]), k
    empty = evaluation.OnceDetections(NAMES, DEV, rows=4)
    empty.update(padded([{'name': [], 'boxes_3d': np.zeros((0, 7)), 'score': np.zeros(0)}], 4), {'frame_id': ['e']})
    (a,) = empty.to_annos()
    assert a['name'].shape == (0,) and a['boxes_3d'].shape == (0, 7) and a['frame_id'] == 'e'
    for rows in (det.rows, 1025):
        with pytest.raises(ValueError, match="OnceDetections.widen: rows"):
            det.widen(rows)
    with pytest.raises(ValueError, match="OnceDetections.update: n"):
        empty.update(padded([p[0]], 40), {'frame_id': ['x']})


@pytest.mark.parametrize("options", [{}, dict(use_superclass=False), dict(difficulty_mode='Distance', num_pr_points=10)])
def test_the_table_from_the_record_equals_the_table_from_its_annos(options):
    g, _, _ = batches()
    det = record()
    a, b = evaluation.OnceEval(g, det, NAMES, **options), evaluation.OnceEval(g, det.to_annos(), NAMES, **options)
    stages = lambda e: (e.overlaps(),) + e.flags() + (e.matched_scores(),) + e.thresholds() + (e.counts(),)      # noqa: E731
    for x, y in zip(stages(a), stages(b)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    ra, rb = evaluation.once_eval(g, det, NAMES, **options), evaluation.once_eval(g, det.to_annos(), NAMES, **options)
    assert ra[0] == rb[0] and list(ra[1]) == list(rb[1]) and all(float(ra[1][k]) == float(rb[1][k]) for k in ra[1])
    assert max(float(v) for v in ra[1].values()) > 10
    with pytest.raises(AssertionError, match="the number of GT must match predictions"):
        evaluation.once_eval(g[:3], det, NAMES)


def test_host_reads():
    g, _, bs = batches()
    record().counts()                                                                     # every allocation below has run once
    evaluation.once_eval(g, record(), NAMES)
    _, control = host_reads(lambda: (bs[0][0]['num'].tolist(), bs[0][0]['num'].tolist()))
    assert len(control) == 2, f"the sync debug mode does not count host reads one by one: {control}"
    torch.cuda.synchronize()
    mode, raised = torch.cuda.get_sync_debug_mode(), False
    try:
        torch.cuda.set_sync_debug_mode("error")
        det = record(bs)                                                                  # three updates and a widen: no host read
        try:
            bs[0][0]['num'].tolist()
        except RuntimeError:
            raised = True
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert raised, "torch.cuda.set_sync_debug_mode('error') did not raise on a host read: the check above proves nothing"
    _, seen = host_reads(det.counts)
    assert len(seen) == 1, seen
    _, seen = host_reads(det.counts)
    assert seen == []                                                                     # cached
    ev = evaluation.OnceEval(g, det, NAMES)
    _, seen = host_reads(ev.curves)
    assert len(seen) == 1, seen
    _, seen = host_reads(lambda: (ev.curves(), ev.result()))
    assert seen == []
    _, seen = host_reads(det.to_annos)
    assert len(seen) == 1, seen                                                           # "one more read"


class StubEngine:
    def __init__(self, outs):
        self.outs = list(outs)

    def detect(self, batch_dict):
        return self.outs.pop(0)


def test_evaluate_once_runs_any_engine():
    g, p, bs = batches()
    ret_str, ret, annos = evaluation.evaluate_once(StubEngine([b[0] for b in bs]), [b[1] for b in bs], g, NAMES, keep_annos=True)
    want_str, want, _ = kr.statement(g, p, NAMES)
    assert ret_str == want_str and max(abs(float(ret[k]) - float(want[k])) for k in want) <= 1e-12
    assert [len(a['name']) for a in annos] == [len(a['name']) for a in p]
    assert evaluation.evaluate_once(StubEngine([b[0] for b in bs]), [b[1] for b in bs], g, NAMES)[2] is None
    with pytest.raises(ValueError, match="evaluate_once: no batches"):
        evaluation.evaluate_once(StubEngine([]), [], g, NAMES)
    with pytest.raises(NotImplementedError, match="OnceDetections"):
        evaluation.OnceDetections(NAMES, "cpu")


def test_evaluate_once_end_to_end_on_the_centerpoint_engine():
    from gdmae_hip import inference
    from test_inference_engine import _batch, _model
    net, ds, skw = _model()
    eng = inference.compile_detector(net)
    names = list(ds.class_names)
    batches_ = []
    for i, seed in enumerate((21, 22)):
        bd = _batch(ds, skw, seed=seed)
        bd['frame_id'] = ['%06d' % (2 * i + b) for b in range(2)]
        batches_.append(bd)
    want_annos = []
    for bd in batches_:
        want_annos += evaluation.once_prediction_dicts(bd, net.padded_to_pred_dicts(eng.detect(dict(bd))), names)
    # GT annos: every frame's twelve best boxes, moved by a few centimetres
    rng, gts = np.random.RandomState(9), []
    for a in want_annos:
        top = np.argsort(-a['score'], kind='stable')[:12]
        boxes = a['boxes_3d'][top].astype(np.float64)
        boxes[:, :2] += rng.uniform(-0.05, 0.05, (len(top), 2))
        gts.append(dict(name=a['name'][top], boxes_3d=boxes))
    options = dict(use_superclass=False, iou_thresholds={n: 0.5 for n in names})
    ret_str, ret, annos = evaluation.evaluate_once(eng, [dict(bd) for bd in batches_], gts, names, keep_annos=True, **options)
    assert len(annos) == len(want_annos) == 4 and sum(len(a['score']) for a in annos) > 0
    for a, b in zip(annos, want_annos):
        assert a['frame_id'] == b['frame_id'] and a['name'].tolist() == b['name'].tolist()
        assert np.array_equal(a['score'], b['score']) and np.array_equal(a['boxes_3d'], b['boxes_3d'])
    want_str, want = evaluation.once_eval_numpy(gts, annos, names, bev_overlap=kr.bev_overlap, **options)
    assert ret_str == want_str and list(ret) == list(want)
    assert all(abs(float(ret[k]) - float(want[k])) <= 1e-12 or (ret[k] != ret[k] and want[k] != want[k]) for k in ret)
    assert np.nanmax(np.array([float(v) for v in want.values()])) > 0
    print(f"end to end: {[len(a['score']) for a in annos]} detections per frame, classes {names}\n{ret_str}")
