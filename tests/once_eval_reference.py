"""Scene builders for the ONCE evaluator (``gdmae_hip.evaluation.once_eval`` / ``once_eval_numpy``) on which the
statistics have ONE answer in any arithmetic.  Not a test.

A frame lives on 120 slots: a 12 x 10 ground grid with 12 m pitch around the sensor (lidar x, y), so that its rows fall into all three
distance bands.  A GT row takes a slot; a prediction "of" a GT row is that row shifted along its length to an overlap drawn from bands
between the thresholds; fillers take slots of their own.  GT annos are fp64 with two decimals, prediction annos fp32 (network outputs).
GT headings are multiples of 0.01 rad and prediction headings odd multiples of 0.005 rad, so that every heading difference of an
ordinary pair is an odd multiple of 0.005: at least 2.6e-3 away from pi / 2, pi and 3 pi / 2.  The crafted heading cases break that
pattern on purpose and sit in a small frame of their own.

``margins_hold`` is asserted on every frame that leaves this file; a frame is regenerated from the next seed until it holds:
  * every pair IoU is >= 1e-3 away from 0.7, 0.5 and 0.3;
  * two predictions with a positive IoU with the same GT row differ in it by >= 1e-3, or are exact copies of each other;
  * every distance is >= 1e-2 m away from 30 and 50;
  * every folded heading difference is >= 1e-3 rad away from pi / 2, and unfolded >= 1e-3 away from pi.
Under these margins flags, matched scores, thresholds and tp / fp / fn are integers / fp32 values that must be equal."""
import functools
import math

import numpy as np

from gdmae_hip import evaluation
from pcdet.models.roi_heads import proposal_targets as pt

MARGIN = 1e-3
DIST_MARGIN = 1e-2
IOU_THRESHOLDS = (0.7, 0.5, 0.3)
FIVE = ['Car', 'Bus', 'Truck', 'Pedestrian', 'Cyclist']
NX, NY, PITCH = 12, 10, 12.0
DIMS = {'Car': (4.4, 1.9, 1.6), 'Bus': (9.0, 2.8, 3.2), 'Truck': (7.0, 2.5, 3.0), 'Pedestrian': (0.8, 0.7, 1.7), 'Cyclist': (1.8, 0.7, 1.6),
        'Tricycle': (2.6, 1.4, 1.7)}      # (l, w, h); Tricycle is a name the evaluator does not know
BANDS = ((0.05, 0.2), (0.36, 0.44), (0.56, 0.64), (0.78, 0.95))
# one seed per frame of the golden scene.  Frame 0 is not 100: with that seed the reference's fp32 polygon is 2.5e-4 off on a
# Pedestrian pair at 59 m, more than the quarter of the margin tests/golden/make_golden_once_eval.py allows
GOLDEN_SEEDS = [200, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 112, 113]


@functools.lru_cache(maxsize=None)
def _bev(a, b):
    # The circle test is a shortcut of THIS helper, not part of the contract: the statement is the exact clipping, which returns 0
    # for two rectangles whose circumscribed circles do not meet.  tests/test_once_eval_gpu.py asserts once, on the pair just
    # outside the kernel's prefilter, that the unfiltered clipping agrees.
    ra, rb = 0.5 * math.hypot(a[3], a[4]), 0.5 * math.hypot(b[3], b[4])
    if math.hypot(a[0] - b[0], a[1] - b[1]) > ra + rb + 1e-3:
        return 0.0                                            # the circumscribed circles do not meet: the clipping would return 0
    return pt.exact_bev_overlap(a, b)


def bev_overlap(a, b):
    """the package's exact fp64 clipping, remembered per pair (the subsets of a scene repeat its frames)"""
    return _bev(tuple(float(v) for v in a), tuple(float(v) for v in b))


statement = functools.partial(evaluation.once_eval_numpy, bev_overlap=bev_overlap, stages=True)


def slot_ground(s):
    return -66.0 + PITCH * (s % NX), -54.0 + PITCH * (s // NX)


def slot_band(s):
    d = math.hypot(*slot_ground(s))
    return 0 if d < 28 else 1 if 32 < d < 48 else 2 if d > 52 else -1


def gt_row(rng, name, slot, rot=None):
    l, w, h = (np.array(DIMS[name]) * (1 + 0.1 * rng.uniform(-1, 1, 3))).round(2)
    x, y = (np.array(slot_ground(slot)) + rng.uniform(-0.5, 0.5, 2)).round(2)
    rot = round(float(rng.uniform(-math.pi, math.pi)), 2) if rot is None else rot
    return dict(name=name, box=[x, y, round(float(-0.8 + rng.uniform(-0.1, 0.1)), 2), l, w, h, rot])


def shift_for(u):
    """relative shift of one of two equal intervals that leaves an IoU of u"""
    return (1.0 - u) / (1.0 + u)


def det_of(rng, g, score, u=None, name=None, drot=None, exact=False, jitter=0.05):
    """a prediction of GT row g: shifted along its length to a BEV IoU of about u, turned by an odd multiple of 0.005 rad"""
    x, y, z, l, w, h, rot = g['box']
    if exact:
        return dict(name=name or g['name'], box=[x, y, z, l, w, h, rot], score=score)
    u = rng.uniform(*BANDS[rng.randint(len(BANDS))]) if u is None else u
    s = shift_for(u) * l * (1 if rng.rand() < 0.5 else -1)
    drot = (2 * rng.randint(-10, 10) + 1) * 0.005 if drot is None else drot
    dims = np.array([l, w, h]) * (1 + jitter * rng.uniform(-1, 1, 3))
    return dict(name=name or g['name'], score=score,
                box=[x + s * math.cos(rot), y - s * math.sin(rot), z + rng.uniform(-0.05, 0.05), *dims, rot + drot])      # rot turns clockwise in (x, y), as in the reference


def filler(rng, name, slot, score):
    g = gt_row(rng, name if name in DIMS else 'Car', slot)
    g['box'][6] += 0.005
    return dict(g, name=name, score=score)


def to_annos(gts, preds):
    g = dict(name=np.array([r['name'] for r in gts], dtype='<U16'), boxes_3d=np.array([r['box'] for r in gts], np.float64).reshape(-1, 7))
    p = dict(name=np.array([r['name'] for r in preds], dtype='<U16'), boxes_3d=np.array([r['box'] for r in preds], np.float32).reshape(-1, 7),
             score=np.array([r['score'] for r in preds], np.float32))
    return g, p


def margins_hold(gt, pred, why=None):
    """the conditions of the module docstring on one frame (annos); ``why`` collects the first violation"""
    why = [] if why is None else why
    g32, p32 = (np.asarray(a['boxes_3d'], np.float32).astype(np.float64) for a in (gt, pred))
    for side, b in (('gt', g32), ('pred', p32)):
        dist = np.sqrt((b[:, :3] ** 2).sum(axis=1))
        for edge in (30.0, 50.0):
            if b.shape[0] and np.abs(dist - edge).min() < DIST_MARGIN:
                why.append(f"{side} distance {dist[np.abs(dist - edge).argmin()]:.5f}")
                return False
    if g32.shape[0] and p32.shape[0]:
        d = np.abs(g32[:, 6][:, None] - p32[:, 6][None, :])
        f = np.where(d >= math.pi, 2 * math.pi - d, d)
        if np.abs(f - math.pi / 2).min() < MARGIN or np.abs(d - math.pi).min() < MARGIN:
            why.append("a heading difference at pi / 2 or pi")
            return False
    ov = evaluation.once_statement_overlaps(g32, p32, False, bev_overlap)
    for t in IOU_THRESHOLDS:
        if ov.size and np.abs(ov - t).min() < MARGIN:
            why.append(f"an IoU {ov.flat[np.abs(ov - t).argmin()]:.5f} at {t}")
            return False
    for i in range(ov.shape[0]):
        js = np.nonzero(ov[i] > 0)[0]
        for a in range(len(js)):
            for b in range(a + 1, len(js)):
                ja, jb = js[a], js[b]
                if abs(ov[i, ja] - ov[i, jb]) < MARGIN and not np.array_equal(pred['boxes_3d'][ja], pred['boxes_3d'][jb]):
                    why.append(f"GT row {i}: predictions {ja} and {jb} with IoU {ov[i, ja]:.5f} and {ov[i, jb]:.5f}")
                    return False
    return True


def until_margins(build, seed):
    """build(rng) -> (gts, preds) rows; the first seed from ``seed`` in steps of 1000 whose frame keeps the margins"""
    for attempt in range(200):
        g, p = to_annos(*build(np.random.RandomState(seed + 1000 * attempt)))
        if margins_hold(g, p):
            return g, p
    raise AssertionError(f"no frame with margins from seed {seed}")


def random_frame(rng, names, n_gt, per_gt, n_fill, slots=None, deciding_last=False, fill_names=None):
    """n_gt GT rows with names drawn from ``names``, up to ``per_gt`` predictions each, ``n_fill`` fillers on slots of their own"""
    slots = list(rng.permutation(NX * NY)) if slots is None else list(slots)
    gts = [gt_row(rng, names[rng.randint(len(names))], slots.pop()) for _ in range(n_gt)]
    preds = []
    for i, g in enumerate(gts[:-1] if deciding_last else gts):
        for _ in range(rng.randint(0, per_gt + 1) if per_gt else 0):
            other = FIVE[rng.randint(5)] if rng.rand() < 0.15 else None
            preds.append(det_of(rng, g, round(float(rng.uniform(0.05, 0.95)), 3), name=other or (g['name'] if g['name'] in FIVE else 'Car')))
    fill_names = fill_names or FIVE
    for _ in range(n_fill):
        preds.append(filler(rng, fill_names[rng.randint(len(fill_names))], slots.pop(), round(float(rng.uniform(0.05, 0.6)), 3)))
    order = rng.permutation(len(preds))
    preds = [preds[i] for i in order]
    if deciding_last:
        preds.append(det_of(rng, gts[-1], 0.99, u=0.9, name=gts[-1]['name']))
    return gts, preds


def sized_frame(seed, names, n_gt, n_pred, fill_names=None):
    """exactly n_gt GT rows and n_pred predictions, the last prediction the only candidate (and a true positive) of the last GT row"""
    def build(rng):
        per = max(1, min(4, (n_pred - 1) // max(n_gt - 1, 1)))
        gts, preds = random_frame(rng, names, n_gt, per if n_gt > 1 else 0, 0, deciding_last=True, fill_names=fill_names)
        last = preds.pop()
        slots = [s for s in rng.permutation(NX * NY)]
        used = {(round((g['box'][0] + 66.0) / PITCH), round((g['box'][1] + 54.0) / PITCH)) for g in gts}
        free = [s for s in slots if (s % NX, s // NX) not in used]
        preds = preds[:n_pred - 1]
        names_f = fill_names or ['Car', 'Bus', 'Pedestrian', 'Cyclist']
        while len(preds) < n_pred - 1:
            preds.append(filler(rng, names_f[rng.randint(len(names_f))], free[len(preds) % len(free)], round(float(rng.uniform(0.05, 0.6)), 3)))
            if len(preds) > len(free):                        # more fillers than free slots: stack them high above each other
                preds[-1]['box'][2] += 10.0 * (len(preds) // len(free))
        return gts, preds + [last]
    return until_margins(build, seed)


def at_distance(row, dist, theta=0.3):
    row = dict(row, box=list(row['box']))
    row['box'][0], row['box'][1], row['box'][2] = dist * math.cos(theta), dist * math.sin(theta), 0.0
    return row


def band_edges_frame(rng):
    """rows at 29.99 / 30.01 / 49.99 / 50.01 m (2e-5 further from the edge, so that the 1e-2 margin holds after fp32 rounding); equal
    scores on competing predictions; an exact copy of a GT box and a copy of the copy; a flag-1 prediction that is the only candidate
    of a flag-0 GT row; boxes just inside and just outside the circle prefilter; a zero-volume pair"""
    gts, preds = [], []
    for k, d in enumerate((29.98998, 30.01002, 49.98998, 50.01002)):
        g = at_distance(gt_row(rng, 'Car', 0, rot=0.0), d, theta=0.2 + 0.6 * k)
        gts.append(g)
        x, y, z, l, w, h, rot = g['box']
        preds.append(dict(name='Car', score=0.9 - 0.01 * k, box=[x, y, z, l * 0.95, w * 0.95, h, rot + 0.005]))      # the same centre
    # a flag-0 GT row (below 30 m) whose only candidate lies beyond 30 m: length along the ray, the prediction shifted outwards
    g = at_distance(gt_row(rng, 'Car', 0, rot=0.0), 29.8, theta=2.9)
    g['box'][6] = -2.9                                       # clockwise: the length lies along the ray
    gts.append(g)
    preds.append(dict(name='Car', score=0.8, box=[30.3 * math.cos(2.9), 30.3 * math.sin(2.9)] + g['box'][2:6] + [-2.895]))
    # equal scores on two competing predictions, an exact copy and a copy of the copy
    g = gt_row(rng, 'Pedestrian', 3 * NX + 5)
    gts.append(g)
    preds += [det_of(rng, g, 0.7, u=0.6), det_of(rng, g, 0.7, u=0.8)]
    g = gt_row(rng, 'Car', 6 * NX + 6)
    gts.append(g)
    preds += [det_of(rng, g, 0.6, exact=True), det_of(rng, g, 0.6, exact=True)]
    # the circle prefilter: same heading, centres on the diagonal, 1e-2 inside and 1e-2 outside the reach of the two circles
    g = gt_row(rng, 'Car', 8 * NX + 2, rot=0.3)
    gts.append(g)
    x, y, z, l, w, h, rot = g['box']
    diag, phi = math.hypot(l, w), -rot + math.atan2(w, l)
    for sign, gap in ((1, -1e-2), (-1, 1e-2)):
        r = sign * (diag + 1e-3 + gap)
        preds.append(dict(name='Car', score=0.5, box=[x + r * math.cos(phi), y + r * math.sin(phi), z, l, w, h, rot]))      # corners overlap by millimetres
    # a zero-volume pair: union 0, 0 / 0 in the reference
    g = gt_row(rng, 'Pedestrian', 1 * NX + 9)
    g['box'][5] = 0.0
    gts.append(g)
    preds.append(dict(det_of(rng, g, 0.4, exact=True)))
    return gts, preds


def headings_frame(rng):
    """square boxes at one centre each, turned by just under and just over pi / 2, just over pi, 8 rad (above 2.5 pi: folds to a
    negative value and stays matched) and 1e-3 rad"""
    gts, preds = [], []
    for k, (rg, d) in enumerate(((0.4, math.pi / 2 - 2e-3), (0.4, math.pi / 2 + 2e-3), (-0.4, math.pi + 2e-3), (4.0, -8.0), (1.0, 1e-3))):
        g = gt_row(rng, 'Car', 2 * k * NX + 3 + k, rot=rg)
        g['box'][3] = g['box'][4] = 2.0
        gts.append(g)
        x, y, z, l, w, h, rot = g['box']
        preds.append(dict(name='Car', score=0.9 - 0.1 * k, box=[x, y, z, l * 0.99, w * 0.99, h, rot + d]))
    return gts, preds


@functools.lru_cache(maxsize=None)
def crafted_scene():
    """11 frames -> (gt_annos, pred_annos).  No Cyclist GT row and no Truck prediction anywhere."""
    names = ['Car', 'Bus', 'Truck', 'Pedestrian', 'Tricycle']
    no_truck = ['Car', 'Bus', 'Pedestrian', 'Cyclist']
    empty = to_annos([], [])

    def first(rng):
        g = [gt_row(rng, 'Car', 4 * NX + 5), gt_row(rng, 'Pedestrian', 5 * NX + 7)]
        return g, [det_of(rng, g[0], 0.9, u=0.9)]
    frames = [until_margins(first, 1),
              sized_frame(2, names, 33, 129),
              sized_frame(3, ['Car'], 1, 63),
              sized_frame(4, ['Car', 'Bus'], 2, 64),
              sized_frame(5, ['Pedestrian', 'Truck'], 2, 65),
              until_margins(lambda rng: ([gt_row(rng, 'Bus', 17)], []), 6),
              until_margins(lambda rng: ([], [filler(rng, 'Cyclist', 40, 0.5)]), 7),
              empty,
              until_margins(band_edges_frame, 8),
              until_margins(headings_frame, 9),
              until_margins(lambda rng: (lambda g: ([g], [det_of(rng, g, 0.7, u=0.9)]))(gt_row(rng, 'Bus', 77)), 10)]
    for g, p in frames:
        p['name'][p['name'] == 'Truck'] = 'Car'
        assert 'Cyclist' not in g['name'] and 'Truck' not in p['name']
    return [f[0] for f in frames], [f[1] for f in frames]


@functools.lru_cache(maxsize=None)
def golden_scene():
    """14 frames -> (gt_annos, pred_annos): all five names and an unknown one, rows in every band for every class, more than 51
    matched Vehicle scores, exactly one Cyclist GT row beyond 50 m."""
    by_band = {b: [s for s in range(NX * NY) if slot_band(s) == b] for b in (0, 1, 2)}
    frames = []
    for f in range(14):
        def build(rng, f=f):
            near = list(rng.permutation(by_band[0] + by_band[1]))
            far = list(rng.permutation(by_band[2]))
            gts, preds = [], []
            plan = [('Car', 4), ('Bus', 2), ('Truck', 2), ('Pedestrian', 3), ('Tricycle', 1)]
            for name, n in plan:
                for i in range(n):
                    gts.append(gt_row(rng, name, far.pop() if i == 0 and (f + len(gts)) % 2 == 0 else near.pop()))
            for i in range(2):
                gts.append(gt_row(rng, 'Cyclist', far.pop() if (f == 5 and i == 0) else near.pop()))
            for i, g in enumerate(gts):
                lone = f == 5 and g['name'] == 'Cyclist' and i == len(gts) - 2          # the one Cyclist row beyond 50 m: a true positive
                if lone or rng.rand() < 0.75:
                    preds.append(det_of(rng, g, round(float(rng.uniform(0.3, 0.95)), 3), u=rng.uniform(0.88, 0.97), jitter=0.02,
                                        name=g['name'] if g['name'] in FIVE else 'Car'))
                for _ in range(0 if lone else rng.randint(0, 3)):
                    other = FIVE[rng.randint(5)] if rng.rand() < 0.15 else None
                    preds.append(det_of(rng, g, round(float(rng.uniform(0.05, 0.95)), 3), name=other or (g['name'] if g['name'] in FIVE else 'Car')))
            for name in FIVE:
                preds.append(filler(rng, name, (far if rng.rand() < 0.5 else near).pop(), round(float(rng.uniform(0.05, 0.6)), 3)))
            for p in preds:                                   # the same orientation a full turn away: only the fold matches these
                if rng.rand() < 0.2:
                    p['box'][6] -= math.copysign(2 * math.pi, p['box'][6])
            return gts, [preds[i] for i in rng.permutation(len(preds))]
        frames.append(until_margins(build, GOLDEN_SEEDS[f]))
    return [f[0] for f in frames], [f[1] for f in frames]


def pack_annos(gt_annos, pred_annos):
    """-> dict of flat arrays for an .npz"""
    cat = lambda annos, k, w=None: np.concatenate([np.asarray(a[k]).reshape((-1,) if w is None else (-1, w)) for a in annos])      # noqa: E731
    return dict(gt_count=np.array([len(a['name']) for a in gt_annos]), pred_count=np.array([len(a['name']) for a in pred_annos]),
                gt_name=cat(gt_annos, 'name').astype('<U16'), gt_boxes=cat(gt_annos, 'boxes_3d', 7).astype(np.float64),
                pred_name=cat(pred_annos, 'name').astype('<U16'), pred_boxes=cat(pred_annos, 'boxes_3d', 7).astype(np.float32),
                pred_score=cat(pred_annos, 'score').astype(np.float32))


def unpack_annos(z):
    go, po = (np.concatenate([[0], np.cumsum(z[k])]) for k in ('gt_count', 'pred_count'))
    gts = [dict(name=z['gt_name'][go[f]:go[f + 1]], boxes_3d=z['gt_boxes'][go[f]:go[f + 1]]) for f in range(len(go) - 1)]
    preds = [dict(name=z['pred_name'][po[f]:po[f + 1]], boxes_3d=z['pred_boxes'][po[f]:po[f + 1]], score=z['pred_score'][po[f]:po[f + 1]])
             for f in range(len(po) - 1)]
    return gts, preds
