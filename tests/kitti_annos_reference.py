"""Scene builders for the KITTI annos of the detections (``gdmae_hip.evaluation.kitti_annos_numpy`` / ``gdmae_kitti_annos``)
on which every arithmetic decides the same way.  Not a test.

A frame is a set of lidar boxes [x, y, z, dx, dy, dz, heading] (fp32) with scores, 1-based labels and one of three KITTI-like
calibrations, each with its own image shape.  ``rows_hold`` is true for every row that leaves this file (a candidate row that misses
it is replaced by the next one of the same seed):
  * every corner's rectified |z| is >= 0.1 m (the projection divides by it);
  * the clipped image-box height is >= 1e-2 px away from 25 and 40 (the flags of ``kitti_clean_data``);
  * every unclipped edge is >= 1e-3 px away from 0 and from width - 1 / height - 1 (whether an edge is clipped).
``corner_geometry`` is a second, matrix-form evaluation of the projection in fp64, independent of the statement's own lines."""
import functools
import math

import numpy as np

from gdmae_hip import evaluation

THREE = ['Car', 'Pedestrian', 'Cyclist']
SWAPPED = ['Pedestrian', 'Car']                 # a class_names order that is not KITTI's
DIMS = {'Car': (3.9, 1.6, 1.56), 'Pedestrian': (0.8, 0.6, 1.73), 'Cyclist': (1.76, 0.6, 1.73)}      # (dx, dy, dz)

_f = lambda rows: np.array(rows, np.float32)      # noqa: E731
CALIBS = [
    dict(P2=_f([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]]),
         R0=_f([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459], [0.007402527, 0.004351614, 0.9999631]]),
         Tr_velo2cam=_f([[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                         [0.9998621, 0.00752379, 0.01480755, -0.2717806]])),
    dict(P2=_f([[707.0493, 0.0, 604.0814, 45.75831], [0.0, 707.0493, 180.5066, -0.3454157], [0.0, 0.0, 1.0, 0.004981016]]),
         R0=_f([[0.9999128, 0.01009263, -0.008511932], [-0.01012729, 0.9999406, -0.004037671], [0.008470675, 0.004123522, 0.9999556]]),
         Tr_velo2cam=_f([[0.006927964, -0.9999722, -0.002757829, -0.02457729], [-0.001162982, 0.002749836, -0.9999955, -0.06127237],
                         [0.9999753, 0.006931141, -0.001143899, -0.3321029]])),
    dict(P2=_f([[718.856, 0.0, 607.1928, 45.38225], [0.0, 718.856, 185.2157, -0.1130887], [0.0, 0.0, 1.0, 0.003779761]]),
         R0=_f([[0.9999454, 0.007259129, -0.007519551], [-0.007292213, 0.9999638, -0.004381729], [0.007487471, 0.004436324, 0.9999621]]),
         Tr_velo2cam=_f([[0.007967514, -0.9999679, -0.0008462264, -0.01377769], [-0.002771053, 0.000824171, -0.9999958, -0.05542117],
                         [0.9999644, 0.007969825, -0.002764397, -0.2918589]])),
]
SHAPES = [(375, 1242), (370, 1224), (376, 1241)]          # (height, width)


class CalibObject:
    """the attributes of the reference's ``Calibration`` that the annos read"""

    def __init__(self, d):
        self.P2, self.R0, self.V2C = d['P2'], d['R0'], d['Tr_velo2cam']


def corner_geometry(boxes, calib):
    """boxes (n, 7) fp32 -> (rect z (n, 8), u (n, 8), v (n, 8)) of the eight corners in fp64, unclipped: matrix form"""
    b = np.asarray(boxes, np.float32).astype(np.float64)
    P, R, V = (np.asarray(calib[k], np.float32).astype(np.float64) for k in ('P2', 'R0', 'Tr_velo2cam'))
    bottom = np.concatenate([b[:, :2], b[:, 2:3] - b[:, 5:6] / 2, np.ones((len(b), 1))], axis=1)
    loc = bottom @ V.T @ R.T
    l, w, h, ry = b[:, 3], b[:, 4], b[:, 5], -b[:, 6] - np.pi / 2
    sx, sz = np.array([1, 1, -1, -1, 1, 1, -1, -1]) / 2.0, np.array([1, -1, -1, 1, 1, -1, -1, 1]) / 2.0
    local = np.stack([l[:, None] * sx, np.concatenate([np.zeros((len(b), 4)), -np.repeat(h[:, None], 4, axis=1)], axis=1), w[:, None] * sz], axis=2)
    rot = np.zeros((len(b), 3, 3))
    rot[:, 0, 0], rot[:, 0, 2], rot[:, 1, 1], rot[:, 2, 0], rot[:, 2, 2] = np.cos(ry), -np.sin(ry), 1.0, np.sin(ry), np.cos(ry)
    corners = np.einsum('nki,nij->nkj', local, rot) + loc[:, None, :]
    hom = np.concatenate([corners, np.ones((len(b), 8, 1))], axis=2) @ P.T
    with np.errstate(divide='ignore', invalid='ignore'):
        return corners[:, :, 2], hom[:, :, 0] / corners[:, :, 2], hom[:, :, 1] / corners[:, :, 2]


def image_boxes(boxes, calib, shape):
    """-> (unclipped (n, 4), clipped (n, 4)) fp64 image boxes"""
    _, u, v = corner_geometry(boxes, calib)
    raw = np.stack([u.min(axis=1), v.min(axis=1), u.max(axis=1), v.max(axis=1)], axis=1)
    hi = np.array([shape[1] - 1, shape[0] - 1, shape[1] - 1, shape[0] - 1], np.float64)
    return raw, np.clip(raw, 0.0, hi)


def rows_hold(boxes, calib, shape):
    """(n) bool: the margins of the module's header"""
    z, _, _ = corner_geometry(boxes, calib)
    raw, clipped = image_boxes(boxes, calib, shape)
    hi = np.array([shape[1] - 1, shape[0] - 1, shape[1] - 1, shape[0] - 1], np.float64)
    height = np.abs(clipped[:, 3] - clipped[:, 1])
    ok = (np.abs(z) >= 0.1).all(axis=1) & np.isfinite(raw).all(axis=1)
    ok &= (np.abs(height - 25) >= 1e-2) & (np.abs(height - 40) >= 1e-2)
    ok &= (np.abs(raw) >= 1e-3).all(axis=1) & (np.abs(raw - hi) >= 1e-3).all(axis=1)
    return ok


def candidate_rows(rng, n, n_classes):
    """n random rows over the whole lidar range, behind the sensor included: (boxes (n, 7) fp32, labels (n) int64)"""
    names = THREE[:n_classes] if n_classes <= 3 else THREE
    labels = rng.randint(1, n_classes + 1, n).astype(np.int64)
    dims = np.array([DIMS[names[(k - 1) % len(names)]] for k in labels]).reshape(n, 3) * (1 + 0.15 * rng.uniform(-1, 1, (n, 3)))
    x = np.where(rng.rand(n) < 0.9, rng.uniform(3.0, 75.0, n), rng.uniform(-20.0, 3.0, n))
    y = rng.uniform(-1.0, 1.0, n) * np.maximum(np.abs(x) * 0.9, 4.0)
    zc = rng.uniform(-1.9, 0.6, n)
    heading = rng.uniform(-2.0 * math.pi, 2.0 * math.pi, n)
    return np.concatenate([np.stack([x, y, zc], axis=1), dims, heading[:, None]], axis=1).astype(np.float32), labels


def random_frame(seed, n, ci, n_classes=3):
    """-> dict(boxes (n, 7), scores (n), labels (n), calib index): the first n candidates of the seed that keep the margins"""
    rng = np.random.RandomState(seed)
    boxes, labels = candidate_rows(rng, 2 * n + 16, n_classes)
    keep = np.nonzero(rows_hold(boxes, CALIBS[ci], SHAPES[ci]))[0][:n]
    assert len(keep) == n, (seed, n, len(keep))
    scores = rng.uniform(0.05, 0.99, n).astype(np.float32)
    return dict(boxes=np.ascontiguousarray(boxes[keep]), scores=scores, labels=np.ascontiguousarray(labels[keep]), calib=ci)


PI32 = float(np.float32(math.pi))
# (x, y, z, class, heading): one of everything the projection and the flags distinguish, for calibration 0
SPECIAL = [
    (6.0, 3.2, -0.8, 'Car', 0.0),               # clipped at the left edge
    (6.0, -3.2, -0.8, 'Car', 0.0),              # clipped at the right edge
    (5.0, 0.3, -0.2, 'Car', PI32 / 2),          # near: clipped at the top and at the bottom
    (10.0, 0.0, 8.0, 'Car', -PI32 / 2),         # above the image: both rows clip to 0, height 0, flag 1 everywhere
    (0.5, 0.4, -0.8, 'Car', 0.0),               # straddles the camera plane: corners on both sides of z = 0
    (-15.0, 0.0, -0.8, 'Car', PI32),            # y = 0 and x < 0: the branch cut of atan2(-y, x)
    (-15.0, -0.0, -0.8, 'Pedestrian', -PI32),   # ... with y = -0.0
    (20.0, 1.0, -0.8, 'Car', 4.0),              # headings beyond pi, tall enough for every difficulty
    (22.0, -4.0, -0.8, 'Pedestrian', -5.5),
    (24.0, 6.0, -0.8, 'Cyclist', 7.0),
    (42.0, 2.0, -0.8, 'Car', 0.3),              # between 25 and 40 px: flag 1 for "easy" only
    (45.0, -6.0, -0.8, 'Pedestrian', 0.3),
    (47.0, 9.0, -0.8, 'Cyclist', 0.3),
    (70.0, 3.0, -0.8, 'Car', 1.0),              # under 25 px: flag 1 for every difficulty
    (74.0, -3.0, -0.6, 'Pedestrian', 1.0),
    (74.0, 8.0, -0.6, 'Cyclist', 1.0),
]


def special_frame(seed=11, tries=200):
    """the crafted rows with a seeded jitter of the dimensions (regenerated from the next seed until every row keeps the margins)"""
    for k in range(tries):
        rng = np.random.RandomState(seed + 1000 * k)
        boxes = np.array([[x, y, z, *(np.array(DIMS[name]) * (1 + 0.02 * rng.uniform(-1, 1, 3))), h] for x, y, z, name, h in SPECIAL], np.float32)
        if rows_hold(boxes, CALIBS[0], SHAPES[0]).all():
            labels = np.array([THREE.index(name) + 1 for _, _, _, name, _ in SPECIAL], np.int64)
            return dict(boxes=boxes, scores=rng.uniform(0.1, 0.9, len(boxes)).astype(np.float32), labels=labels, calib=0)
    raise AssertionError(f"no special frame with the margins in {tries} seeds from {seed}")


def reached(frame):
    """what a frame reaches: the set of edge names of the issue's list"""
    ci = frame['calib']
    boxes = frame['boxes']
    z, _, _ = corner_geometry(boxes, CALIBS[ci])
    raw, clipped = image_boxes(boxes, CALIBS[ci], SHAPES[ci])
    h, w = SHAPES[ci]
    inside = (raw[:, 2] > 0) & (raw[:, 0] < w - 1) & (raw[:, 3] > 0) & (raw[:, 1] < h - 1) & (z > 0).all(axis=1)
    out = set()
    for name, hit in (('clip left', inside & (raw[:, 0] < 0)), ('clip top', inside & (raw[:, 1] < 0)), ('clip right', inside & (raw[:, 2] > w - 1)),
                      ('clip bottom', inside & (raw[:, 3] > h - 1)), ('outside, height 0', (clipped[:, 3] == clipped[:, 1]) & (z > 0).all(axis=1)),
                      ('straddles the camera plane', (z > 0).any(axis=1) & (z < 0).any(axis=1)),
                      ('heading 0', boxes[:, 6] == 0), ('heading pi/2', boxes[:, 6] == np.float32(PI32 / 2)),
                      ('heading -pi/2', boxes[:, 6] == np.float32(-PI32 / 2)), ('heading pi', boxes[:, 6] == np.float32(PI32)),
                      ('heading -pi', boxes[:, 6] == np.float32(-PI32)), ('heading beyond pi', np.abs(boxes[:, 6]) > 3.2),
                      ('branch cut', (boxes[:, 1] == 0) & (boxes[:, 0] < 0))):
        if hit.any():
            out.add(name)
    return out


EDGES = {'clip left', 'clip top', 'clip right', 'clip bottom', 'outside, height 0', 'straddles the camera plane', 'heading 0', 'heading pi/2',
         'heading -pi/2', 'heading pi', 'heading -pi', 'heading beyond pi', 'branch cut'}


@functools.lru_cache(maxsize=None)
def golden_scene():
    """the frames of tests/golden/kitti_annos.npz -> (frames, class_names per frame): the special frame, one frame per calibration,
    an empty frame, and a frame whose labels mean ['Pedestrian', 'Car']"""
    frames = [special_frame(), random_frame(21, 14, 0), random_frame(22, 11, 1), random_frame(23, 0, 1), random_frame(24, 13, 2),
              random_frame(25, 9, 2, n_classes=2)]
    return frames, [THREE] * 5 + [SWAPPED]


def statement(frame, class_names, calib=None):
    ci = frame['calib']
    return evaluation.kitti_annos_numpy(frame['boxes'], frame['scores'], frame['labels'], CALIBS[ci] if calib is None else calib, SHAPES[ci],
                                        class_names)


def batch_dict(frames, first_id=0):
    """the entries of a ``batch_dict`` that the annos read"""
    return {'calib': [CalibObject(CALIBS[f['calib']]) for f in frames], 'image_shape': np.array([SHAPES[f['calib']] for f in frames], np.int32),
            'frame_id': ['%06d' % (first_id + i) for i in range(len(frames))]}


def _eval_frame(rng, ci, n_gt, n_near, n_far):
    """GT lidar boxes in front of the camera, detections near them (shifted along the heading, turned a little) and fillers"""
    names = [THREE[i % 3] for i in range(n_gt)]
    x = rng.uniform(8.0, 60.0, n_gt)
    gt = np.array([[x[i], rng.uniform(-0.45, 0.45) * x[i], rng.uniform(-0.9, -0.6), *(np.array(DIMS[names[i]]) * (1 + 0.1 * rng.uniform(-1, 1, 3))),
                    rng.uniform(-math.pi, math.pi)] for i in range(n_gt)], np.float32).reshape(n_gt, 7)
    gt_labels = np.array([THREE.index(n) + 1 for n in names], np.int64)
    det, det_labels = [], []
    for k in range(n_near):
        i = k % n_gt
        u = rng.uniform(*[(0.3, 0.45), (0.55, 0.65), (0.75, 0.95)][rng.randint(3)])
        s = (1.0 - u) / (1.0 + u) * gt[i, 3] * (1 if rng.rand() < 0.5 else -1)
        b = gt[i].astype(np.float64)
        b[0], b[1], b[6] = b[0] + s * math.cos(b[6]), b[1] + s * math.sin(b[6]), b[6] + rng.uniform(-0.1, 0.1)
        det.append(b)
        det_labels.append(gt_labels[i] if rng.rand() < 0.85 else 1 + (gt_labels[i] % 3))
    far, far_labels = candidate_rows(rng, n_far, 3)
    det = np.concatenate([np.array(det, np.float32).reshape(-1, 7), far], axis=0)
    det_labels = np.concatenate([np.array(det_labels, np.int64), far_labels])
    order = rng.permutation(len(det))
    return (dict(boxes=gt, scores=np.ones(n_gt, np.float32), labels=gt_labels, calib=ci),
            dict(boxes=np.ascontiguousarray(det[order]), scores=rng.uniform(0.05, 0.99, len(det)).astype(np.float32),
                 labels=np.ascontiguousarray(det_labels[order]), calib=ci))


EVAL_COUNTS = ((6, 9, 4), (5, 0, 0), (7, 12, 5), (0, 0, 3), (6, 10, 2))      # (GT rows, detections near them, fillers) per frame


@functools.lru_cache(maxsize=None)
def eval_scene():
    """-> (GT annos, detection frames, the statement's detection annos): GT annos are the statement's annos of lidar GT boxes with
    ``occluded`` / ``truncated`` drawn per row.  Every frame keeps the margins of this module and those of the evaluator's scenes
    (tests/kitti_eval_reference.py ``margins_hold``: overlaps 1e-3 away from 0.7 / 0.5 / 0.25, competing detections, heights,
    truncations); a frame is regenerated from the next seed until it does."""
    import kitti_eval_reference as kr
    gts, frames, annos = [], [], []
    for k, (n_gt, n_near, n_far) in enumerate(EVAL_COUNTS):
        for t in range(200):
            rng = np.random.RandomState(300 + k + 1000 * t)
            ci = k % 3
            g, d = _eval_frame(rng, ci, n_gt, n_near, n_far)
            if not (rows_hold(g['boxes'], CALIBS[ci], SHAPES[ci]).all() and rows_hold(d['boxes'], CALIBS[ci], SHAPES[ci]).all()):
                continue
            ga, da = statement(g, THREE), statement(d, THREE)
            ga = {key: ga[key] for key in ANNO_KEYS if key not in ('score', 'boxes_lidar')}
            ga['occluded'] = rng.choice([0, 0, 1, 2, 3], n_gt).astype(np.int64)
            ga['truncated'] = rng.choice([0.0, 0.0, 0.2, 0.4, 0.7], n_gt).astype(np.float32)
            if n_gt == 0:
                ga['name'] = np.zeros(0, dtype='<U10')
            if kr.margins_hold(ga, dict(da, name=np.asarray(da['name'], dtype='<U10'))):
                gts.append(ga), frames.append(d), annos.append(da)
                break
        else:
            raise AssertionError(f"no evaluator frame {k} with the margins")
    return gts, frames, annos


ANNO_KEYS = ('name', 'truncated', 'occluded', 'alpha', 'bbox', 'dimensions', 'location', 'rotation_y', 'score', 'boxes_lidar')


def pack_golden(frames, annos):
    """frames and the reference's per-sample dicts -> flat dict of arrays for an .npz"""
    z = {'count': np.array([len(f['scores']) for f in frames]), 'calib': np.array([f['calib'] for f in frames])}
    for k in ('boxes', 'scores', 'labels'):
        z['in_' + k] = np.concatenate([f[k] for f in frames], axis=0)
    for k in ANNO_KEYS:
        parts = [np.asarray(a[k]) for a in annos if len(a['score'])]
        z['ref_' + k] = np.concatenate(parts, axis=0)
    return z


def unpack_golden(z):
    """-> (frames, the reference's per-sample dicts; a frame without rows has none: its dict is None)"""
    off = np.concatenate([[0], np.cumsum(z['count'])])
    frames, annos = [], []
    for f in range(len(off) - 1):
        a, b = int(off[f]), int(off[f + 1])
        frames.append(dict(boxes=z['in_boxes'][a:b], scores=z['in_scores'][a:b], labels=z['in_labels'][a:b], calib=int(z['calib'][f])))
        annos.append({k: z['ref_' + k][a:b] for k in ANNO_KEYS} if b > a else None)
    return frames, annos
