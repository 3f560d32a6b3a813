"""Plain numpy reference of the RoI pooling contract and a builder of scenes on which the contract has one answer.

Not a test.  Geometry decisions (point filter, patch spans, in-box test, voxel indices) are made in fp64; farthest-point
sampling runs in fp32 exactly as specified: d = (dx dx + dy dy) + dz dz, minimum updated on d < d2, largest minimum wins, ties to
the lowest row, start at the lowest row.  Next to its result the reference returns the margin of every decision, per point: the
distance to the nearest xy / z face of any RoI of its sample and the distance of its voxel coordinates from the nearest
integer, so that a scene can keep away from what the contract leaves implementation-defined.

Scenes: every coordinate (points, RoI centres and sizes) is a multiple of 1/64 with |coordinate| < 128, so FPS distances are
exact in fp32 and ties are genuine and frequent.  Points whose face margin is below 1e-4 m or whose voxel margin is below 1e-3
cells are dropped (at most 1 % of a scene, asserted)."""
import numpy as np

FACE_MARGIN = 1e-4       # metres
VOXEL_MARGIN = 1e-3      # cells
SHIPPED = dict(num_dvs_points=1024, num_fps_points=256, lambda_=0.18, delta=50.0, pool_extra_width=(0.8, 0.8, 0.8),
               num_boxes_per_patch=32)
WAYMO_RANGE = np.array([-74.88, -74.88, -2, 74.88, 74.88, 4.0], dtype=np.float32)


def patch_grid(point_cloud_range):
    r = np.asarray(point_cloud_range, dtype=np.float32).astype(np.float64)
    lo = np.round(r[:2] - 1)
    hi = np.round(r[3:5] + 1)
    return lo.astype(np.float32), (int(round(hi[0] - lo[0])), int(round(hi[1] - lo[1])))


def _box64(roi, extra):
    c = roi[:3].astype(np.float64)
    d = roi[3:6].astype(np.float64) + np.asarray(extra, dtype=np.float32).astype(np.float64)
    return c, d, float(roi[6])


def _local(xyz, c, heading):
    """lidar -> box frame (rotation by -heading), fp64"""
    s = xyz.astype(np.float64) - c
    ca, sa = np.cos(-heading), np.sin(-heading)
    return np.stack([s[:, 0] * ca - s[:, 1] * sa, s[:, 0] * sa + s[:, 1] * ca, s[:, 2]], axis=1)


def _resolution(c, lambda_, delta):
    return max(0.02, float(np.float32(lambda_)) * np.exp(-np.sqrt((c * c).sum()) / float(np.float32(delta))))


def pair_margins(points, rois, params):
    """Per point: (face margin, voxel margin) = minima over the RoIs of its sample (voxel: over the RoIs it lies inside)."""
    n = points.shape[0]
    face = np.full(n, np.inf)
    voxel = np.full(n, np.inf)
    for b in range(rois.shape[0]):
        rows = np.nonzero(points[:, 0] == b)[0]
        for roi in rois[b]:
            c, d, h = _box64(roi, params['pool_extra_width'])
            loc = _local(points[rows, 1:4], c, h)
            a = np.abs(loc)
            fx, fy, fz = a[:, 0] - (d[0] / 2 + 1e-5), a[:, 1] - (d[1] / 2 + 1e-5), a[:, 2] - d[2] / 2
            # a face only decides for points that the other two tests let through (with slack)
            near = (fx < FACE_MARGIN) & (fy < FACE_MARGIN) & (fz < FACE_MARGIN)
            m = np.minimum(np.minimum(np.abs(fx), np.abs(fy)), np.abs(fz))
            face[rows] = np.minimum(face[rows], np.where(near, m, np.inf))
            inside = (fx < 0) & (fy < 0) & (fz <= 0)
            res = _resolution(c, params['lambda_'], params['delta'])
            v = (loc + d / 2) / res
            vm = np.abs(v - np.round(v)).min(axis=1)
            voxel[rows] = np.minimum(voxel[rows], np.where(inside, vm, np.inf))
    return face, voxel


def roi_size_margin(rois, params):
    """Smallest distance of size / resolution from an integer over all RoIs and axes (the clamp bound ``out`` is a truncation)."""
    worst = np.inf
    for roi in rois.reshape(-1, rois.shape[-1]):
        c, d, _ = _box64(roi, params['pool_extra_width'])
        q = d / _resolution(c, params['lambda_'], params['delta'])
        worst = min(worst, float(np.abs(q - np.round(q)).min()))
    return worst


def fps_fp32(xyz, rounds):
    n = xyz.shape[0]
    mind = np.full(n, np.inf, dtype=np.float32)
    sel = [0]
    for _ in range(1, rounds):
        cur = xyz[sel[-1]]
        dx, dy, dz = xyz[:, 0] - cur[0], xyz[:, 1] - cur[1], xyz[:, 2] - cur[2]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        upd = d < mind
        mind[upd] = d[upd]
        best = mind.max()
        sel.append(int(np.nonzero(mind == best)[0][0]))      # lowest row among the ties
    return np.asarray(sel, dtype=np.int64), mind


def pool_reference(points, rois, point_cloud_range, params):
    """points (N, 4 + C) fp32, rois (B, M, 7) fp32 -> dict(idx (B, M, K) int32, num (B, M) int32, feats (B M, K, 3 + C + 6) fp32,
    glob (B M, K, 3) fp32, cand: list of the kept representative rows per RoI (ascending), voxels: their voxel indices,
    face / voxel: per-point decision margins)."""
    points = np.asarray(points, dtype=np.float32)
    rois = np.asarray(rois, dtype=np.float32)
    B, M = rois.shape[:2]
    K, C = params['num_fps_points'], points.shape[1] - 4
    rng = np.asarray(point_cloud_range, dtype=np.float32).astype(np.float64)
    lo, (X, Y) = patch_grid(point_cloud_range)
    lo = lo.astype(np.float64)
    p64 = points[:, 1:4].astype(np.float64)
    keep = (p64[:, 0] >= rng[0]) & (p64[:, 0] <= rng[3]) & (p64[:, 1] >= rng[1]) & (p64[:, 1] <= rng[4])
    px = np.clip(np.trunc(p64[:, 0] - lo[0]).astype(np.int64), 0, X - 1)
    py = np.clip(np.trunc(p64[:, 1] - lo[1]).astype(np.int64), 0, Y - 1)
    out = dict(idx=np.zeros((B, M, K), np.int32), num=np.zeros((B, M), np.int32), feats=np.zeros((B * M, K, 3 + C + 6), np.float32),
               glob=np.zeros((B * M, K, 3), np.float32), cand=[], voxels=[])
    for b in range(B):
        mine = keep & (points[:, 0] == b)
        lists = {}                                       # occupied patch -> RoI list, capped, in RoI order
        for r in range(M):
            c, d, h = _box64(rois[b, r], params['pool_extra_width'])
            ch, sh = np.cos(h), np.sin(h)
            qx = np.array([-d[0], d[0], d[0], -d[0]]) / 2
            qy = np.array([-d[1], -d[1], d[1], d[1]]) / 2
            ax, ay = qx * ch - qy * sh + c[0], qx * sh + qy * ch + c[1]
            sx0, sy0 = int(np.trunc(ax.min() - lo[0])), int(np.trunc(ay.min() - lo[1]))
            sx1, sy1 = int(np.trunc(ax.max() - lo[0])), int(np.trunc(ay.max() - lo[1]))
            for yy in range(max(sy0, 0), min(sy1, Y - 1) + 1):
                for xx in range(max(sx0, 0), min(sx1, X - 1) + 1):
                    lst = lists.setdefault((yy, xx), [])
                    if len(lst) < params['num_boxes_per_patch']:
                        lst.append(r)
        for r in range(M):
            c, d, h = _box64(rois[b, r], params['pool_extra_width'])
            rows = np.nonzero(mine)[0]
            rows = rows[[r in lists.get((int(py[i]), int(px[i])), ()) for i in rows]] if rows.size else rows
            loc = _local(points[rows, 1:4], c, h)
            inside = (np.abs(loc[:, 2]) <= d[2] / 2) & (np.abs(loc[:, 0]) < d[0] / 2 + 1e-5) & (np.abs(loc[:, 1]) < d[1] / 2 + 1e-5)
            rows, loc = rows[inside], loc[inside]
            res = _resolution(c, params['lambda_'], params['delta'])
            bound = np.trunc(d / res).astype(np.int64)
            vox = np.minimum(np.maximum(np.trunc((loc + d / 2) / res).astype(np.int64), 0), bound - 1)
            reps = {}
            for row, v in zip(rows, map(tuple, vox)):     # rows ascend: the first row of a voxel is its lowest
                reps.setdefault(v, row)
            order = sorted(reps.items(), key=lambda kv: kv[1])[:params['num_dvs_points']]
            cand = np.asarray([row for _, row in order], dtype=np.int64)
            out['cand'].append(cand)
            out['voxels'].append([v for v, _ in order])
            n = cand.shape[0]
            out['num'][b, r] = n
            if n == 0:
                continue
            sel, _ = fps_fp32(points[cand, 1:4], min(K, n))
            got = cand[[sel[s] if s < n else sel[s % n] for s in range(K)]]
            o = b * M + r
            out['idx'][b, r] = got
            g64 = points[got, 1:4].astype(np.float64)
            out['feats'][o, :, :3] = _local(g64, rois[b, r, :3].astype(np.float64), h)
            out['feats'][o, :, 3:3 + C] = points[got, 4:]
            half = rois[b, r, 3:6] / np.float32(2)
            out['feats'][o, :, 3 + C:3 + C + 3] = -half
            out['feats'][o, :, 3 + C + 3:] = half
            out['glob'][o] = points[got, 1:4]
    out['face'], out['voxel'] = pair_margins(points, rois, params)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------
def q64(v):
    """nearest multiple of 1/64 as fp32 (exact)"""
    return (np.round(np.asarray(v, dtype=np.float64) * 64) / 64).astype(np.float32)


def make_rois(rng, B, M, centre_lo, centre_hi, headings=None):
    """(B, M, 7) fp32: centres / sizes on the 1/64 lattice, headings over the full circle."""
    rois = np.zeros((B, M, 7), dtype=np.float32)
    rois[..., 0] = q64(rng.uniform(centre_lo[0], centre_hi[0], (B, M)))
    rois[..., 1] = q64(rng.uniform(centre_lo[1], centre_hi[1], (B, M)))
    rois[..., 2] = q64(rng.uniform(0.0, 1.5, (B, M)))
    rois[..., 3] = q64(rng.uniform(1.0, 5.0, (B, M)))
    rois[..., 4] = q64(rng.uniform(0.8, 2.2, (B, M)))
    rois[..., 5] = q64(rng.uniform(1.2, 2.2, (B, M)))
    rois[..., 6] = (rng.uniform(-np.pi, np.pi, (B, M)) if headings is None else headings).astype(np.float32)
    return rois


def settle_sizes(rois, params):
    """Grow a RoI size by 1/64 m steps until size / resolution is 5e-3 away from a whole number (in place; padded rows stay zero)."""
    for roi in rois.reshape(-1, rois.shape[-1]):
        if not roi.any():
            continue
        for k in range(3):
            while True:
                c, d, _ = _box64(roi, params['pool_extra_width'])
                q = d[k] / _resolution(c, params['lambda_'], params['delta'])
                if abs(q - np.round(q)) > 5e-3:
                    break
                roi[3 + k] += np.float32(1 / 64)
    return rois


def points_in_roi(rng, roi, extra, n, slack=0.3):
    """n lattice points around the enlarged RoI (some just outside)"""
    d = roi[3:6].astype(np.float64) + np.asarray(extra, dtype=np.float64) + slack
    loc = rng.uniform(-0.5, 0.5, (n, 3)) * d
    h = float(roi[6])
    x = loc[:, 0] * np.cos(h) - loc[:, 1] * np.sin(h) + roi[0]
    y = loc[:, 0] * np.sin(h) + loc[:, 1] * np.cos(h) + roi[1]
    return q64(np.stack([x, y, loc[:, 2] + roi[2]], axis=1))


def lattice_block(roi, extra, step=0.25):
    """every lattice point of pitch ``step`` inside the (axis-aligned) enlarged RoI, kept 1/32 m off the faces"""
    d = roi[3:6].astype(np.float64) + np.asarray(extra, dtype=np.float64)
    axes = [np.arange(-np.floor((d[k] / 2 - 1 / 32) / step), np.floor((d[k] / 2 - 1 / 32) / step) + 1) * step + roi[k] for k in range(3)]
    g = np.stack(np.meshgrid(*axes, indexing='ij'), axis=-1).reshape(-1, 3)
    return q64(g)


def assemble(rng, per_sample_xyz, C=2, shuffle=True):
    """list (per sample) of (n, 3) -> points (N, 4 + C) fp32 with seeded features, rows shuffled across the batch"""
    rows = []
    for b, xyz in enumerate(per_sample_xyz):
        f = rng.uniform(0, 1, (xyz.shape[0], C)).astype(np.float32)
        rows.append(np.concatenate([np.full((xyz.shape[0], 1), b, np.float32), xyz.astype(np.float32), f], axis=1))
    pts = np.concatenate(rows, axis=0) if rows else np.zeros((0, 4 + C), np.float32)
    if shuffle and pts.shape[0]:
        pts = pts[rng.permutation(pts.shape[0])]
    return np.ascontiguousarray(pts, dtype=np.float32)


def make_safe(points, rois, params, max_drop=0.01):
    """Drop the points whose decisions are within the margins; at most ``max_drop`` of the scene."""
    assert np.abs(points[:, 1:4]).max(initial=0) < 128 and np.all(points[:, 1:4] * 64 == np.round(points[:, 1:4] * 64))
    assert roi_size_margin(rois, params) > VOXEL_MARGIN, "a RoI size is within the margin of a whole number of voxels"
    face, voxel = pair_margins(points, rois, params)
    ok = (face >= FACE_MARGIN) & (voxel >= VOXEL_MARGIN)
    dropped = int((~ok).sum())
    assert dropped <= max_drop * max(points.shape[0], 1), f"{dropped} of {points.shape[0]} points are within the decision margins"
    return np.ascontiguousarray(points[ok])


# ---------------------------------------------------------------------------------------------------------------------------
# the scenes of tests/test_roi_pool_{cpu,gpu}.py: name -> (points, rois, point_cloud_range, params); built and solved once
# ---------------------------------------------------------------------------------------------------------------------------
LDS_TABLE_FILL = 3072      # distinct voxels the kernel's LDS table accepts in one pass (csrc/roi_pool.hip RP_FILL)


def _scene_shipped():
    rng = np.random.default_rng(11)
    P = SHIPPED
    B, M = 2, 12
    rois = make_rois(rng, B, M, (-60, -60), (60, 60), headings=np.linspace(-np.pi, np.pi, B * M, endpoint=False).reshape(B, M))
    rois[0, 0, :6] = [1.0, 1.0, 0.5, 6.0, 6.0, 3.0]                 # large, near the origin: > 1024 voxels (the cap)
    rois[0, 0, 6] = 0.0
    rois[0, 1, :2] = [74.0, -30.0]                                  # partly outside the xy range
    rois[1, 2, :2] = [-20.0, 74.5]
    rois[0, 5, :3] = [-70.0, -70.0, 3.5]                            # no points
    settle_sizes(rois, P)
    xyz = [[], []]
    for b in range(B):
        for r in range(M):
            if (b, r) == (0, 0):
                xyz[b].append(lattice_block(rois[b, r], P['pool_extra_width'], step=0.5))
            elif (b, r) == (0, 5):
                continue                                            # no points
            elif (b, r) == (1, 3):
                xyz[b].append(points_in_roi(rng, rois[b, r], P['pool_extra_width'], 60))      # < 256 voxels: repeat padding
            else:
                xyz[b].append(points_in_roi(rng, rois[b, r], P['pool_extra_width'], 420 if r % 2 == 0 else 110))
        xyz[b].append(q64(np.concatenate([rng.uniform(-76, 76, (150, 2)), rng.uniform(-1, 3, (150, 1))], axis=1)))
    pts = assemble(rng, [np.concatenate(v) for v in xyz])
    return make_safe(pts, rois, P), rois, WAYMO_RANGE, P


def _scene_tiny():
    rng = np.random.default_rng(12)
    P = dict(SHIPPED, num_dvs_points=16, num_fps_points=8)
    rois = settle_sizes(make_rois(rng, 1, 4, (-30, -30), (30, 30)), P)
    xyz = np.concatenate([points_in_roi(rng, rois[0, r], P['pool_extra_width'], n) for r, n in enumerate((120, 100, 5, 75))])
    pts = assemble(rng, [xyz])
    return make_safe(pts, rois, P), rois, WAYMO_RANGE, P


def _scene_box_cap():
    rng = np.random.default_rng(13)
    P = dict(SHIPPED, num_boxes_per_patch=32)
    one = settle_sizes(make_rois(rng, 1, 1, (10.2, 10.2), (10.8, 10.8)), P)
    rois = np.repeat(one, 40, axis=1)
    pts = assemble(rng, [points_in_roi(rng, rois[0, 0], P['pool_extra_width'], 300)])
    return make_safe(pts, rois, P), rois, WAYMO_RANGE, P


def _scene_one_by_one():
    rng = np.random.default_rng(14)
    rois = settle_sizes(make_rois(rng, 1, 1, (-5, -5), (5, 5)), SHIPPED)
    pts = assemble(rng, [points_in_roi(rng, rois[0, 0], SHIPPED['pool_extra_width'], 400)])
    return make_safe(pts, rois, SHIPPED), rois, WAYMO_RANGE, SHIPPED


def _scene_empty_sample():
    """sample 1 has RoIs and no points"""
    rng = np.random.default_rng(15)
    rois = settle_sizes(make_rois(rng, 2, 3, (-20, -20), (20, 20)), SHIPPED)
    xyz = np.concatenate([points_in_roi(rng, rois[0, r], SHIPPED['pool_extra_width'], 150) for r in range(3)])
    pts = assemble(rng, [xyz, np.zeros((0, 3), np.float32)])
    return make_safe(pts, rois, SHIPPED), rois, WAYMO_RANGE, SHIPPED


def _scene_padded_rois():
    """the RoIs of sample 1 are all zero-padded rows (an empty first stage); points around the origin fall into their enlarged box"""
    rng = np.random.default_rng(16)
    rois = settle_sizes(make_rois(rng, 2, 3, (-20, -20), (20, 20)), SHIPPED)
    rois[1] = 0
    xyz0 = np.concatenate([points_in_roi(rng, rois[0, r], SHIPPED['pool_extra_width'], 150) for r in range(3)])
    xyz1 = q64(rng.uniform(-1, 1, (200, 3)))
    pts = assemble(rng, [xyz0, xyz1])
    return make_safe(pts, rois, SHIPPED), rois, WAYMO_RANGE, SHIPPED


def _scene_lds_overflow():
    """one RoI with more distinct voxels than the LDS table takes in one pass"""
    rng = np.random.default_rng(17)
    rois = np.zeros((1, 2, 7), np.float32)
    rois[0, 0] = [0.5, 0.5, 1.0, 4.0, 4.0, 2.0, 0.0]
    rois[0, 1] = [20.0, 5.0, 1.0, 4.0, 2.0, 1.5, 1.0]
    settle_sizes(rois, SHIPPED)
    xyz = np.concatenate([lattice_block(rois[0, 0], SHIPPED['pool_extra_width'], step=0.25),
                          points_in_roi(rng, rois[0, 1], SHIPPED['pool_extra_width'], 200)])
    pts = assemble(rng, [xyz])
    return make_safe(pts, rois, SHIPPED), rois, WAYMO_RANGE, SHIPPED


SCENES = {'shipped': _scene_shipped, 'tiny': _scene_tiny, 'box_cap': _scene_box_cap, 'one_by_one': _scene_one_by_one,
          'empty_sample': _scene_empty_sample, 'padded_rois': _scene_padded_rois, 'lds_overflow': _scene_lds_overflow}
_SOLVED = {}


def scene(name):
    """(points, rois, point_cloud_range, params, reference result) - computed once per process, never modified"""
    if name not in _SOLVED:
        pts, rois, pcr, P = SCENES[name]()
        ref = pool_reference(pts, rois, pcr, P)
        for a in (pts, rois, *[v for v in ref.values() if isinstance(v, np.ndarray)]):
            a.setflags(write=False)
        _SOLVED[name] = (pts, rois, pcr, P, ref)
    return _SOLVED[name]


def run_module(name, device='cpu'):
    """The scene through ``RoILocalDFVSPool3dV2.pool`` on ``device`` -> (idx, num, feats, glob) numpy"""
    import torch
    from pcdet.ops.patch_ops import patch_ops_utils as po
    pts, rois, pcr, P, _ = scene(name)
    lo, (X, Y) = patch_grid(pcr)
    layer = po.RoILocalDFVSPool3dV2(pc_range=np.array([lo[0], lo[1], 0, lo[0] + X, lo[1] + Y, 0], np.float32),
                                    patch_size=np.array([1.0, 1.0, -1.0], np.float32), num_dvs_points=P['num_dvs_points'],
                                    num_fps_points=P['num_fps_points'], hash_size=4099, lambda_=P['lambda_'], delta=P['delta'],
                                    pool_extra_width=list(P['pool_extra_width']), num_boxes_per_patch=P['num_boxes_per_patch'])
    out = layer.pool(torch.from_numpy(pts.copy()).to(device), torch.from_numpy(rois.copy()).to(device),
                     range_xy=[pcr[0], pcr[1], pcr[3], pcr[4]])
    return [t.cpu().numpy() for t in out]
