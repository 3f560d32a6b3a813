"""The numpy statement of the recall-record contract (``gdmae_hip.evaluation.recall_record_numpy``) with its geometry from
``oracle/iou3d_oracle.py``, and a builder of scenes on which the contract has one answer.

Not a test.  Boxes come from the helpers of tests/roi_targets_reference.py: GT boxes on a 16 m grid, predicted boxes and RoIs = GT
boxes shifted along their length to a chosen IoU band (the bands below stay 0.02 away from the recall thresholds 0.3 / 0.5 / 0.7 and
from the thresholds that file's ``roi_near`` avoids by itself).  ``check_margins`` asserts on everything generated:
  * every valid GT row's largest fp64 IoU, over the predicted rows and over the RoI rows, is >= 1e-3 away from every threshold;
  * no compared pair is a margin case of the reference's BEV overlap (``roi_targets_reference.margin_case``).  "Compared" means every
    pair whose centres are within the two half-diagonals + 0.2 m: beyond the half-diagonals the circumscribed circles are disjoint
    and the overlap is 0 in any arithmetic, which is also why the fp64 statement skips the clipping there."""
import functools
import math

import numpy as np

import roi_targets_reference as rt
from gdmae_hip import evaluation
from roi_targets_reference import MARGIN, gt_box, margin_case, roi_near

T3 = [0.3, 0.5, 0.7]
LOW, MID, HIGH, TOP = (0.02, 0.28), (0.32, 0.48), (0.52, 0.68), (0.77, 0.98)      # IoU bands between the thresholds


def centre_gap(a, b):
    """distance of the centres minus the two half-diagonals (> 0: the footprints cannot meet)"""
    a, b = [float(v) for v in a[:7]], [float(v) for v in b[:7]]
    return math.hypot(a[0] - b[0], a[1] - b[1]) - 0.5 * math.hypot(a[3], a[4]) - 0.5 * math.hypot(b[3], b[4])


def bev_overlap(a, b):
    """the oracle's exact fp64 clipping; 0 without it where the circumscribed circles are disjoint"""
    return 0.0 if centre_gap(a, b) > 1e-6 else rt.bev_overlap(a, b)


statement = functools.partial(evaluation.recall_record_numpy, bev_overlap=bev_overlap)


def solve(S):
    return statement(S['pred'], S['pred_num'], S['gt'], S['thresh'], rois=S['rois'], roi_num=S['roi_num'])


def rows_of(S, side, b):
    rows, num = (S['pred'], S['pred_num']) if side == 'pred' else (S['rois'], S['roi_num'])
    return rows[b] if num is None else rows[b, :max(int(num[b]), 0)]


def check_margins(S, best):
    for b in range(S['gt'].shape[0]):
        nv = evaluation.valid_gt_rows(S['gt'][b])
        for col, side in ((1, 'pred'), (0, 'rois')):
            if side == 'rois' and S['rois'] is None:
                continue
            for t in S['thresh']:
                assert nv == 0 or np.abs(best[b, :nv, col] - t).min() >= MARGIN, (b, side, t)
            for p in rows_of(S, side, b):
                for g in range(nv):
                    if centre_gap(p, S['gt'][b, g]) <= 0.2:
                        assert not margin_case(p, S['gt'][b, g]), (b, side, g)


# ---------------------------------------------------------------------------------------------------------------------------------
# scene builder
# ---------------------------------------------------------------------------------------------------------------------------------
def grid_gt(rng, n, per_row=9, pitch=15.0, origin=(-60.0, -60.0)):
    return np.stack([gt_box(rng, origin[0] + pitch * (i % per_row), origin[1] + pitch * (i // per_row), 1 + i % 3) for i in range(n)])


def far_boxes(rng, k, row=0):
    """k boxes away from the grid and from each other"""
    return [gt_box(rng, 90.0 + 8.0 * i, -90.0 - 8.0 * row, 1 + i % 3)[:7] for i in range(k)]


def near(rng, gt, plan):
    """plan: list of (GT row, band) -> list of 7-column boxes"""
    return [roi_near(rng, gt[g], *band) for g, band in plan]


def random_plan(rng, n_gt, k, bands=(LOW, MID, HIGH, TOP)):
    return [(int(g), bands[int(c)]) for g, c in zip(rng.randint(0, n_gt, k), rng.randint(0, len(bands), k))]


def assemble(rng, samples, G, n, M=None, pred_cols=7, gt_cols=8, thresh=T3, null_pred_num=False, null_roi_num=False):
    """samples: list of (gt (g, 8), predicted boxes [7-column], RoIs [7-column] or None) -> the padded batch.  Rows behind a sample's
    count hold copies of its GT boxes (IoU 1 if they were read) unless the count argument is null, where they are its own last row
    repeated (or zero rows when it has none)."""
    B = len(samples)
    with_rois = samples[0][2] is not None
    S = dict(gt=np.zeros((B, G, gt_cols), np.float32), pred=np.zeros((B, n, pred_cols), np.float32), thresh=list(thresh),
             pred_num=None if null_pred_num else np.zeros(B, np.int32), rois=np.zeros((B, M, 7), np.float32) if with_rois else None,
             roi_num=None if (null_roi_num or not with_rois) else np.zeros(B, np.int32))
    for b, (gt, pred, rois) in enumerate(samples):
        S['gt'][b, :gt.shape[0]] = gt[:, :gt_cols]
        for rows, key, num in ((pred, 'pred', S['pred_num']), (rois, 'rois', S['roi_num'])):
            if rows is None:
                continue
            k, cap = len(rows), S[key].shape[1]
            assert k <= cap
            order = rng.permutation(k)
            for i, j in enumerate(order):
                S[key][b, i, :7] = rows[j]
            S[key][b, :k, 7:] = rng.uniform(-3, 3, (k, S[key].shape[2] - 7))            # velocities: never read
            if num is not None:
                num[b] = k
                live = gt[(gt != 0).any(axis=1)]
                for i in range(k, cap):
                    S[key][b, i, :7] = live[(i - k) % len(live), :7] if len(live) else rng.uniform(1, 2, 7)
            elif k:
                S[key][b, k:] = S[key][b, k - 1]
    return S


def _scene_seams():
    """predicted-row counts 0, 1, 63, 64, 65 and 129 (n = 130, 9 columns); in every sample the LAST predicted row is the only one above
    0.3 for GT row 0; no RoIs: the roi counters stay 0"""
    rng = np.random.RandomState(201)
    samples = []
    for k in (0, 1, 63, 64, 65, 129):
        gt = grid_gt(rng, 12)
        pred = []
        if k:
            others = [(g + 1, band) for g, band in random_plan(rng, 11, max(k - 4, 0))]              # GT rows 1 .. 11, any band
            pred = near(rng, gt, [(0, LOW)] * min(k - 1, 3) + others + [(0, TOP)])
        samples.append((gt, pred, None))
    S = assemble(rng, samples, G=14, n=130, pred_cols=9)
    for b, (_, pred, _) in enumerate(samples):                         # the decisive row goes last
        if len(pred) > 1:
            rows = S['pred'][b, :len(pred), :7]
            i = int(np.nonzero((rows == pred[-1]).all(axis=1))[0][0])
            S['pred'][b, [i, len(pred) - 1]] = S['pred'][b, [len(pred) - 1, i]]
    return S


def _scene_counts():
    """B = 3 with RoIs: pred_num[1] = 0 and roi_num[2] = 0 (the rows behind the counts are copies of the GT boxes)"""
    rng = np.random.RandomState(202)
    samples = []
    for b in range(3):
        gt = grid_gt(rng, 9 - b)
        pred = [] if b == 1 else near(rng, gt, random_plan(rng, gt.shape[0], 20)) + far_boxes(rng, 3)
        rois = [] if b == 2 else near(rng, gt, random_plan(rng, gt.shape[0], 14)) + far_boxes(rng, 2, row=1)
        samples.append((gt, pred, rois))
    return assemble(rng, samples, G=10, n=30, M=20)


def _scene_null_counts():
    """null pred_num and roi_num: all n and all M rows count"""
    rng = np.random.RandomState(203)
    samples = []
    for b in range(2):
        gt = grid_gt(rng, 7)
        samples.append((gt, near(rng, gt, random_plan(rng, 7, 70 - 5 * b)), near(rng, gt, random_plan(rng, 7, 10 - b))))
    return assemble(rng, samples, G=7, n=70, M=10, null_pred_num=True, null_roi_num=True)


def _scene_one_gt():
    """G = 1, T = 1, 7-column GT"""
    rng = np.random.RandomState(204)
    samples = []
    for band in (HIGH, MID):
        gt = grid_gt(rng, 1)
        samples.append((gt, near(rng, gt, [(0, band), (0, LOW)]) + far_boxes(rng, 2), None))
    return assemble(rng, samples, G=1, n=5, gt_cols=7, thresh=[0.5])


def _scene_many_gt():
    """G = 65: more than one wavefront of GT rows in the valid-row count; sample 0 fills all 65 rows, sample 1 has 64 and a trailing
    zero row"""
    rng = np.random.RandomState(205)
    samples = []
    for b in range(2):
        gt = grid_gt(rng, 65 - b)
        samples.append((gt, near(rng, gt, random_plan(rng, 65 - b, 80)), near(rng, gt, random_plan(rng, 65 - b, 40))))
    return assemble(rng, samples, G=65, n=90, M=40)


def _scene_zero_rows():
    """sample 0: an all-zero GT table; sample 1: an all-zero row in the middle (it counts in gt_num and is never recalled) and three
    trailing zero rows; sample 2: a full table"""
    rng = np.random.RandomState(206)
    gt1 = grid_gt(rng, 6)
    ref1 = gt1.copy()
    gt1[2] = 0
    gt2 = grid_gt(rng, 9)
    samples = [(np.zeros((0, 8), np.float32), far_boxes(rng, 4), far_boxes(rng, 2, row=1)),
               (gt1, near(rng, ref1, [(g, TOP) for g in range(6)]), near(rng, ref1, [(g, MID) for g in range(6)])),
               (gt2, near(rng, gt2, random_plan(rng, 9, 12)), near(rng, gt2, random_plan(rng, 9, 8)))]
    return assemble(rng, samples, G=9, n=14, M=9)


def _scene_identical():
    """GT rows 0 and 3 are predicted exactly (IoU 1: recalled at every threshold), row 1 has a TOP RoI only, row 2 nothing"""
    rng = np.random.RandomState(207)
    gt = grid_gt(rng, 4)
    pred = [gt[0, :7].copy(), gt[3, :7].copy()] + near(rng, gt, [(1, LOW)]) + far_boxes(rng, 2)
    rois = near(rng, gt, [(1, TOP), (0, MID)])
    return assemble(rng, [(gt, pred, rois)], G=6, n=8, M=4)


def _scene_prefilter():
    """one predicted box per GT row, of the GT's size and heading, along the GT's diagonal: row 0 at (the two half-diagonals - 0.3 m),
    the corners overlap a little; row 1 at (+ 0.08 m), inside the 0.1 m slack of the prefilter: clipped, overlap 0; row 2 at (+ 0.12 m),
    outside: not clipped, overlap 0; row 3 a MID box for contrast"""
    rng = np.random.RandomState(208)
    gt = grid_gt(rng, 4)
    pred = []
    for g, extra in ((0, -0.3), (1, 0.08), (2, 0.12)):
        p = gt[g, :7].astype(np.float64).copy()
        d = math.hypot(p[3], p[4]) + extra
        phi = p[6] + math.atan2(p[4], p[3])
        p[0] += d * math.cos(phi)
        p[1] += d * math.sin(phi)
        pred.append(p.astype(np.float32))
        gap = centre_gap(pred[-1], gt[g])
        assert abs(gap - extra) < 1e-3 and (gap < 0.1) == (g < 2), (g, gap)
    pred += near(rng, gt, [(3, MID)])
    return assemble(rng, [(gt, pred, None)], G=4, n=4)


SCENES = {'seams': _scene_seams, 'counts': _scene_counts, 'null_counts': _scene_null_counts, 'one_gt': _scene_one_gt,
          'many_gt': _scene_many_gt, 'zero_rows': _scene_zero_rows, 'identical': _scene_identical, 'prefilter': _scene_prefilter}
_SOLVED = {}


def scene(name):
    """(inputs, counters (1 + 2 T) int64, best_iou (B, G, 2) fp64) - built, margin-checked and solved once per process, never modified"""
    if name not in _SOLVED:
        S = SCENES[name]()
        counters, best = solve(S)
        check_margins(S, best)
        for a in (*S.values(), counters, best):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _SOLVED[name] = (S, counters, best)
    return _SOLVED[name]
