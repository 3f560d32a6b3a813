"""Scene builders for the KITTI evaluator (``gdmae_hip.evaluation.kitti_eval`` / ``kitti_eval_numpy``) on which the
official statistics have ONE answer in any arithmetic.  Not a test.

A frame lives on 192 slots: a 16 x 12 ground grid with 8 m pitch (camera x, z) and a 16 x 12 grid of 150 x 120 px image cells.  A GT
row takes a slot; a detection "of" a GT row is that row shifted along its length (3-D) and sideways (image) to overlaps drawn from
bands between the thresholds; fillers and detections over DontCare boxes take slots of their own, so they overlap no GT row.  GT
annos are fp64 with two decimals (label files), detection annos fp32 (network outputs).

``margins_hold`` is asserted on every frame that leaves this file; a frame is regenerated from the next seed until it holds:
  * every pair overlap of every metric and every detection / DontCare overlap is >= 1e-3 away from 0.7, 0.5 and 0.25;
  * two detections with a positive overlap with the same GT row differ in it by >= 1e-3, or are exact copies of each other;
  * box heights are >= 1e-2 away from 25 and 40, truncations >= 1e-3 away from .15 / .3 / .5.
Under these margins tp / fp / fn, the threshold counts and the thresholds themselves are integers / fp32 values that must be equal."""
import functools
import math

import numpy as np

from gdmae_hip import evaluation
from pcdet.models.roi_heads import proposal_targets as pt

MARGIN = 1e-3
OVERLAP_THRESHOLDS = (0.7, 0.5, 0.25)
NX, NZ = 16, 12
DIMS = {'Car': (3.9, 1.56, 1.6), 'Van': (5.0, 2.2, 1.9), 'Pedestrian': (0.8, 1.75, 0.6), 'Person_sitting': (0.8, 1.3, 0.6),
        'Cyclist': (1.76, 1.73, 0.6), 'Truck': (6.0, 3.2, 2.5), 'Tram': (6.0, 3.5, 2.4), 'Misc': (2.0, 1.5, 1.5)}      # (l, h, w)
DET_NAME = {'Car': 'Car', 'Van': 'Car', 'Pedestrian': 'Pedestrian', 'Person_sitting': 'Pedestrian', 'Cyclist': 'Cyclist', 'Truck': 'Car',
            'Tram': 'Car', 'Misc': 'Pedestrian'}
BANDS = ((0.05, 0.2), (0.3, 0.45), (0.55, 0.65), (0.75, 0.95))
HEIGHTS = (62.0, 45.0, 33.0, 28.0, 21.0)


@functools.lru_cache(maxsize=None)
def _bev(a, b):
    return pt.exact_bev_overlap(a, b)


def bev_overlap(a, b):
    """the package's exact fp64 clipping, remembered per pair (the subsets of a scene repeat its frames)"""
    return _bev(tuple(float(v) for v in a), tuple(float(v) for v in b))


statement = functools.partial(evaluation.kitti_eval_numpy, bev_overlap=bev_overlap, stages=True)


def slot_ground(s):
    return -60.0 + 8.0 * (s % NX), 6.0 + 8.0 * (s // NX)


def slot_image(s):
    return 20.0 + 150.0 * (s % NX), 20.0 + 120.0 * (s // NX)


def gt_row(rng, name, slot, height=62.0, occluded=0, truncated=0.0):
    l, h, w = (np.array(DIMS[name]) * (1 + 0.1 * rng.uniform(-1, 1, 3))).round(2)
    x, z = (np.array(slot_ground(slot)) + rng.uniform(-0.5, 0.5, 2)).round(2)
    ry = round(float(rng.uniform(-math.pi, math.pi)), 2)
    x1, y1 = (np.array(slot_image(slot)) + rng.uniform(0, 10, 2)).round(2)
    width = round(float(rng.uniform(50, 110)), 2)
    return dict(name=name, truncated=truncated, occluded=occluded, alpha=round(ry - math.atan2(x, z), 2), bbox=[x1, y1, x1 + width, y1 + height],
                dimensions=[l, h, w], location=[x, round(float(1.6 + rng.uniform(-0.1, 0.1)), 2), z], rotation_y=ry)


def dontcare_row(rng, slot, width=100.0, height=80.0):
    x1, y1 = slot_image(slot)
    return dict(name='DontCare', truncated=-1.0, occluded=-1, alpha=-10.0, bbox=[x1, y1, x1 + width, y1 + height], dimensions=[-1.0, -1.0, -1.0],
                location=[-1000.0, -1000.0, -1000.0], rotation_y=-10.0)


def shift_for(u):
    """relative shift of one of two equal intervals that leaves an IoU of u"""
    return (1.0 - u) / (1.0 + u)


def det_of(rng, g, score, u3=None, u2=None, name=None, height=None, dyaw=None, exact=False):
    """a detection of GT row g: shifted along its length to a BEV IoU of about u3 and sideways in the image to an IoU of about u2"""
    band = lambda: rng.uniform(*BANDS[rng.randint(len(BANDS))])      # noqa: E731
    u3, u2 = band() if u3 is None else u3, band() if u2 is None else u2
    l, h, w = g['dimensions']
    x, y, z = g['location']
    ry = g['rotation_y']
    d = dict(name=name or DET_NAME[g['name']], truncated=0.0, occluded=0, score=score)
    if exact:
        d.update(alpha=g['alpha'], bbox=list(g['bbox']), dimensions=[l, h, w], location=[x, y, z], rotation_y=ry)
        return d
    s = shift_for(u3) * l * (1 if rng.rand() < 0.5 else -1)
    dyaw = rng.uniform(-0.1, 0.1) if dyaw is None else dyaw
    x1, y1, x2, y2 = g['bbox']
    sx = shift_for(u2) * (x2 - x1) * (1 if rng.rand() < 0.5 else -1)
    y2 = y2 if height is None else y1 + height
    d.update(alpha=g['alpha'] + dyaw + rng.uniform(-0.3, 0.3), bbox=[x1 + sx, y1, x2 + sx, y2],
             dimensions=list(np.array([l, h, w]) * (1 + 0.05 * rng.uniform(-1, 1, 3))),
             location=[x + s * math.cos(ry), y + rng.uniform(-0.1, 0.1), z - s * math.sin(ry)], rotation_y=ry + dyaw)      # ry turns clockwise in (x, z)
    return d


def filler(rng, name, slot, score, height=None):
    g = gt_row(rng, name if name in DIMS else 'Car', slot, height=height or HEIGHTS[rng.randint(len(HEIGHTS))])
    g.update(name=name, score=score, truncated=0.0, occluded=0)
    return g


def det_over(rng, dc, slot, score, inside, name='Car', height=50.0):
    """a detection in a free ground slot whose image box lies with the fraction ``inside`` of its area in the DontCare box dc"""
    d = filler(rng, name, slot, score, height=height)
    x1, y1, x2, _ = dc['bbox']
    w = 60.0
    left = x2 - inside * w                                    # the right part of the box sticks out of the DontCare box
    d['bbox'] = [left, y1 + 5.0, left + w, y1 + 5.0 + height]
    assert y1 + 5.0 + height <= dc['bbox'][3] and left >= x1
    return d


def to_annos(gts, dts):
    def pack(rows, det):
        f = np.float32 if det else np.float64
        a = dict(name=np.array([r['name'] for r in rows], dtype='<U16'), truncated=np.array([r['truncated'] for r in rows], f),
                 occluded=np.array([r['occluded'] for r in rows], np.int64), alpha=np.array([r['alpha'] for r in rows], f),
                 bbox=np.array([r['bbox'] for r in rows], f).reshape(-1, 4), dimensions=np.array([r['dimensions'] for r in rows], f).reshape(-1, 3),
                 location=np.array([r['location'] for r in rows], f).reshape(-1, 3), rotation_y=np.array([r['rotation_y'] for r in rows], f))
        if det:
            a['score'] = np.array([r['score'] for r in rows], f)
        return a
    return pack(gts, False), pack(dts, True)


def frame_overlaps(g, d):
    """the statement's fp64 overlaps of one frame of annos -> ((3, D, G), (D, NC))"""
    geo = lambda a: dict(bbox=a['bbox'], geo=np.concatenate([a['location'], a['dimensions'], a['rotation_y'][:, None]], axis=1))      # noqa: E731
    return evaluation.kitti_statement_overlaps(geo(g), geo(d), g['bbox'][g['name'] == 'DontCare'], bev_overlap)


def margins_hold(g, d, why=None):
    why = [] if why is None else why
    ov, dc = frame_overlaps(g, d)
    for t in OVERLAP_THRESHOLDS:
        if ov.size and np.abs(ov - t).min() < MARGIN:
            why.append(('pair overlap', t))
        if dc.size and np.abs(dc - t).min() < MARGIN:
            why.append(('DontCare overlap', t))
    rows = np.concatenate([d['bbox'], d['dimensions'], d['location'], d['rotation_y'][:, None], d['alpha'][:, None], d['score'][:, None]], axis=1)
    for m in range(3):
        for i in range(ov.shape[2]):
            js = np.nonzero(ov[m, :, i] > 0)[0]
            js = js[np.argsort(ov[m, js, i])]
            for a, b in zip(js[:-1], js[1:]):
                if ov[m, b, i] - ov[m, a, i] < MARGIN and not (np.array_equal(rows[a], rows[b]) and d['name'][a] == d['name'][b]):
                    why.append(('competing detections', m, i, int(a), int(b)))
    for a in (g, d):
        h = (a['bbox'][:, 3] - a['bbox'][:, 1]).astype(np.float64)
        if h.size and min(np.abs(np.abs(h) - 25).min(), np.abs(np.abs(h) - 40).min()) < 1e-2:
            why.append('height')
    for t in evaluation.KITTI_MAX_TRUNCATION:
        if g['truncated'].size and np.abs(g['truncated'] - t).min() < MARGIN:
            why.append('truncation')
    return not why


def build_frame(seed, maker, tries=200):
    """maker(rng) -> (gt rows, detection rows): the first of the seeds seed, seed + 1000, .. whose frame keeps the margins"""
    for k in range(tries):
        g, d = to_annos(*maker(np.random.RandomState(seed + 1000 * k)))
        if margins_hold(g, d):
            return g, d
    raise AssertionError(f"no frame with the margins in {tries} seeds from {seed}")


GT_NAMES = ('Car', 'Pedestrian', 'Van', 'Person_sitting', 'DontCare', 'Truck', 'Tram', 'Car', 'Pedestrian')


def random_frame(rng, n_gt, n_dt, gt_names=GT_NAMES, filler_names=('Car', 'Pedestrian', 'Cyclist'), p_near=0.7, p_top=0.3):
    """n_gt GT rows (row 0, when there is one, a fully visible Car that only the LAST detection matches: the deciding detection is the
    last of its frame) and n_dt detections: near a random GT row / over a DontCare box with probability p_near, fillers otherwise."""
    slots = [int(s) for s in rng.permutation(NX * NZ)]
    gts = []
    for i in range(n_gt):
        s = slots.pop()
        name = 'Car' if i == 0 else gt_names[rng.randint(len(gt_names))]
        if name == 'DontCare':
            gts.append(dontcare_row(rng, s))
        elif i == 0:
            gts.append(gt_row(rng, name, s))
        else:
            gts.append(gt_row(rng, name, s, height=HEIGHTS[rng.randint(len(HEIGHTS))], occluded=int(rng.choice([0, 0, 1, 2, 3])),
                              truncated=float(rng.choice([0.0, 0.0, 0.2, 0.4, 0.7]))))
    dts, score, used = [], 0.5, [0] * n_gt
    for k in range(n_dt):
        score = score if (k and rng.rand() < 0.1) else float(np.float32(rng.uniform(0.05, 0.95)))      # now and then the previous score again
        if gts and k == n_dt - 1:
            dts.append(det_of(rng, gts[0], float(np.float32(0.97)), u3=0.9, u2=0.9))
        elif n_gt > 1 and rng.rand() < p_near and min(used[1:]) < 3:
            i = int(rng.choice([i for i in range(1, n_gt) if used[i] < 3]))      # at most three detections near one GT row
            g, used[i] = gts[i], used[i] + 1
            if g['name'] == 'DontCare':
                dts.append(det_over(rng, g, slots.pop(), score, inside=float(rng.choice([1.0, 0.6, 0.4, 0.1])), name=str(rng.choice(['Car', 'Pedestrian']))))
            else:
                r = rng.rand()
                u3, u2 = (rng.uniform(*BANDS[-1]), rng.uniform(*BANDS[-1])) if rng.rand() < p_top else (None, None)
                dts.append(det_of(rng, g, score, u3=u3, u2=u2, name=None if r < 0.85 else 'Cyclist', height=21.0 if 0.5 < r < 0.6 else None))
        else:
            dts.append(filler(rng, filler_names[rng.randint(len(filler_names))], slots.pop(), score))
    return gts, dts


def special_frame(rng):
    """the crafted frame of the GPU scenes: one of everything the matching distinguishes"""
    slots = list(range(NX * NZ))[::-1]
    f32 = lambda v: float(np.float32(v))      # noqa: E731
    car = [gt_row(rng, 'Car', slots.pop()), gt_row(rng, 'Car', slots.pop(), height=33.0, occluded=1),
           gt_row(rng, 'Car', slots.pop(), height=30.0, occluded=2, truncated=0.4), gt_row(rng, 'Car', slots.pop(), occluded=3),
           gt_row(rng, 'Car', slots.pop()), gt_row(rng, 'Car', slots.pop()), gt_row(rng, 'Car', slots.pop())]
    van, ped, sit = gt_row(rng, 'Van', slots.pop()), gt_row(rng, 'Pedestrian', slots.pop()), gt_row(rng, 'Person_sitting', slots.pop())
    dc = [dontcare_row(rng, slots.pop()), dontcare_row(rng, slots.pop())]
    others = [gt_row(rng, 'Tram', slots.pop()), gt_row(rng, 'Truck', slots.pop()), gt_row(rng, 'Pedestrian', slots.pop(), height=28.0, truncated=0.2)]
    gts = car[:2] + [dc[0]] + car[2:4] + [van, ped, sit, dc[1]] + others + car[4:]
    dts = [
        det_of(rng, car[1], f32(0.8), u3=0.85, u2=0.8),
        det_of(rng, car[0], f32(0.6), u3=0.6, u2=0.6),                      # equal scores on two detections of one GT row: pass 1 takes
        det_of(rng, car[0], f32(0.6), u3=0.85, u2=0.85),                    # the lower index, pass 2 the larger overlap
        det_of(rng, car[2], f32(0.7), u3=0.8, u2=0.9, height=21.0),         # under the height limit of every difficulty
        det_of(rng, car[2], f32(0.65), u3=0.9, u2=0.8, height=33.0),        # under the limit of "easy" only
        det_of(rng, car[3], f32(0.9), u3=0.9, u2=0.9),
        det_of(rng, van, f32(0.75), u3=0.8, u2=0.8),                        # a Car detection on a Van: assigned, neither tp nor fp
        det_of(rng, ped, f32(0.55), u3=0.6, u2=0.6), det_of(rng, ped, f32(0.5), u3=0.35, u2=0.8),
        det_of(rng, sit, f32(0.45), u3=0.6, u2=0.6),
        det_of(rng, others[2], f32(0.4), u3=0.7, u2=0.62),
        det_over(rng, dc[0], slots.pop(), f32(0.85), inside=1.0), det_over(rng, dc[0], slots.pop(), f32(0.35), inside=0.4),
        det_over(rng, dc[1], slots.pop(), f32(0.3), inside=0.6, name='Pedestrian'), det_over(rng, dc[1], slots.pop(), f32(0.25), inside=0.1),
        filler(rng, 'Cyclist', slots.pop(), f32(0.7)), filler(rng, 'Cyclist', slots.pop(), f32(0.2)),      # no Cyclist GT anywhere
        det_of(rng, others[0], f32(0.33), u3=0.8, u2=0.8),                  # a Car detection on a Tram: a false positive
        det_of(rng, car[4], f32(0.95), exact=True),                         # an exact copy of a GT box
        det_of(rng, car[4], f32(0.95), exact=True),                         # and a copy of the copy
    ]
    aligned = det_of(rng, car[5], f32(0.92), exact=True)                    # nearly aligned: the same box turned by 1e-3 rad
    aligned['rotation_y'] += 1e-3
    dts.append(aligned)
    # car[6]: three boxes at the prefilter distance (centres apart by the two half-diagonals + 1e-3 m), displaced along the diagonal
    l, _, w = car[6]['dimensions']
    x, y, z = car[6]['location']
    ang = math.atan2(w, l) - car[6]['rotation_y']                        # the direction of a corner (rotation_y turns clockwise)
    for k, delta in enumerate((-0.05, 5e-4, 1.1e-2)):                        # a corner inside; inside the filter, disjoint; outside
        d = filler(rng, 'Car', slots.pop(), f32(0.15 + 0.01 * k))
        dist = math.hypot(l, w) + delta
        d.update(dimensions=list(car[6]['dimensions']), rotation_y=car[6]['rotation_y'],
                 location=[x + dist * math.cos(ang), y, z + dist * math.sin(ang)])
        dts.append(d)
    dts.append(det_of(rng, car[6], f32(0.99), u3=0.9, u2=0.9))              # the deciding detection is the last of the frame
    return gts, dts


def nearly_aligned_pair(g, d):
    """(detection row, GT row) as BEV boxes of the special frame's nearly aligned pair"""
    rect = lambda a, i: [a['location'][i, 0], a['location'][i, 2], 0.0, a['dimensions'][i, 0], a['dimensions'][i, 2], 0.0, -a['rotation_y'][i]]      # noqa: E731
    j = int(np.nonzero(d['score'] == np.float32(0.92))[0][0])
    i = int(np.argmin(np.abs(g['location'][:, 0] - d['location'][j, 0]) + np.abs(g['location'][:, 2] - d['location'][j, 2])))
    return rect(d, j), rect(g, i)


# (GT rows, detections) of the frames of the crafted scene after the special frame: detections 0, 1, 63, 64, 65, 129; GT rows 0, 1, 2, 33
CRAFTED_COUNTS = ((0, 5), (3, 0), (1, 1), (2, 63), (4, 64), (5, 65), (33, 129), (0, 0), (6, 12), (3, 7))


@functools.lru_cache(maxsize=None)
def crafted_scene():
    """11 frames -> (gt_annos, dt_annos): no Cyclist GT and no Truck detection anywhere"""
    names = tuple(n for n in GT_NAMES if n != 'Cyclist')
    frames = [build_frame(7, special_frame)]
    for k, (n_gt, n_dt) in enumerate(CRAFTED_COUNTS):
        frames.append(build_frame(100 + k, lambda rng: random_frame(rng, n_gt, n_dt, names)))      # noqa: B023
    return [f[0] for f in frames], [f[1] for f in frames]


def golden_scene(n_frames=14):
    """the scene of tests/golden/kitti_eval.npz: every class, every ignored value, more than 41 matched Car scores"""
    names = GT_NAMES + ('Cyclist', 'Pedestrian') * 3 + ('Car',) * 7
    frames = [build_frame(500 + k, lambda rng: random_frame(rng, 22, 36, names, p_near=0.85, p_top=0.75)) for k in range(n_frames)]
    return [f[0] for f in frames], [f[1] for f in frames]


ANNO_KEYS = ('name', 'truncated', 'occluded', 'alpha', 'bbox', 'dimensions', 'location', 'rotation_y')


def pack_annos(gt_annos, dt_annos):
    """annos -> flat dict of arrays for an .npz (rows concatenated, frame counts kept)"""
    z = {'gt_count': np.array([len(a['name']) for a in gt_annos]), 'dt_count': np.array([len(a['name']) for a in dt_annos])}
    for side, annos, keys in (('gt', gt_annos, ANNO_KEYS), ('dt', dt_annos, ANNO_KEYS + ('score',))):
        for k in keys:
            z[f'{side}_{k}'] = np.concatenate([a[k] for a in annos], axis=0)
    return z


def unpack_annos(z):
    out = []
    for side, keys in (('gt', ANNO_KEYS), ('dt', ANNO_KEYS + ('score',))):
        off = np.concatenate([[0], np.cumsum(z[f'{side}_count'])])
        out.append([{k: z[f'{side}_{k}'][off[f]:off[f + 1]] for k in keys} for f in range(len(off) - 1)])
    return out[0], out[1]
