"""Crafted scenes for the fine-tune input tests (not a test).  Everything is built on a 1/64 m lattice (features on 1/256), every
candidate owns one database entry, and points that would sit within 1e-3 m of a boundary they are tested against (a face of a
valid sampled box, the xy range after the frame's transformation) are left out while the scene is built, so that the numpy
statement's float64 decisions and an fp32 kernel's cannot differ.  The tests assert those margins on the finished scene."""
import numpy as np

import finetune_input_reference as fr
from oracle import input_oracle as io

CLASS_NAMES = ["Vehicle", "Pedestrian", "Cyclist"]
GROUPS = ["Vehicle", "Pedestrian"]                    # SAMPLE_GROUPS order
PC_RANGE = np.array([-40, -40, -2, 40, 40, 4], np.float32)
SAMPLER_CFG = {"NAME": "gt_sampling", "SAMPLE_GROUPS": ["Vehicle:8", "Pedestrian:4"], "LIMIT_WHOLE_SCENE": True, "REMOVE_POINTS": True,
               "REMOVE_EXTRA_WIDTH": [0.25, 0.25, 0.125], "NUM_POINT_FEATURES": 5, "PREPARE": {}}
WORLD_CFG = [{"NAME": "random_world_flip", "PROBABILITY": 0.5, "ALONG_AXIS_LIST": ["x", "y"]},
             {"NAME": "random_world_rotation", "PROBABILITY": 1.0, "WORLD_ROT_ANGLE": [-0.78539816, 0.78539816]},
             {"NAME": "random_world_scaling", "PROBABILITY": 1.0, "WORLD_SCALE_RANGE": [0.95, 1.05]}]
AUG_CFG = [SAMPLER_CFG] + WORLD_CFG
MARGIN = 1e-3
SIZES = {"Vehicle": (4.0, 2.0, 1.5), "Pedestrian": (0.5, 0.5, 1.75), "Cyclist": (1.75, 0.75, 1.5), "Sign": (1.0, 1.0, 2.0)}


def lat(v, q=64):
    return np.round(np.asarray(v, np.float64) * q) / q


def box(name, x, y, heading=0.0, z=0.5, size=None):
    return name, np.array([x, y, z, *(size or SIZES[name]), heading], np.float32)


def _margin_ok(viol):
    inside = (viol <= 0).all(1)
    m = np.where(inside, (-viol).min(1), np.where(viol > 0, viol, 0).max(1))
    return m >= MARGIN


def _range_ok(pts, pr):
    p = io.augment_frame(pts, pr["flip_x"], pr["flip_y"], pr["angle"], pr["scale"])[:, :2].astype(np.float64)
    r = PC_RANGE.astype(np.float64)
    return _margin_ok(np.concatenate([r[:2] - p, p - r[3:5]], 1))


def _box_ok(pts, b):
    b = np.asarray(b, np.float64)
    c, s = np.cos(-b[6]), np.sin(-b[6])
    sx, sy = pts[:, 0].astype(np.float64) - b[0], pts[:, 1].astype(np.float64) - b[1]
    viol = np.stack([np.abs(pts[:, 2] - b[2]) - b[5] / 2, np.abs(sx * c - sy * s) - (b[3] / 2 + 1e-2), np.abs(sx * s + sy * c) - (b[4] / 2 + 1e-2)], 1)
    return _margin_ok(viol)


def build(seed, frames_spec, params):
    """frames_spec: per frame {'gt': [(name, box)], 'cand': [(name, box, n_points)], 'n': scene points, 'extent': half width of
    the scene cloud}.  -> scene dict (library inputs, the statement's ``cands``, database arrays)."""
    g = np.random.default_rng(seed)
    db_pts, db_off, db_boxes, db_names = [], [], [], []
    frames, gt_boxes, gt_names, candidates, cands = [], [], [], [], []
    per_class = {n: 0 for n in CLASS_NAMES}
    row = 0
    for spec, pr in zip(frames_spec, params):
        gb = np.stack([b for _, b in spec["gt"]]) if spec["gt"] else np.zeros((0, 7), np.float32)
        names = [n for n, _ in spec["gt"]]
        cb = np.stack([b for _, b, _ in spec["cand"]]) if spec["cand"] else np.zeros((0, 7), np.float32)
        cn = [n for n, _, _ in spec["cand"]]
        grp = [GROUPS.index(n) for n in cn]
        assert grp == sorted(grp), "candidates come group by group"
        valid = fr.select(gb, cb, grp, len(GROUPS), {"pair": np.inf})
        ex = spec.get("extent", 45.0)
        n = spec["n"]
        m = n + n // 32 + 16 if n else 0                      # a few spare points: the margin filter removes some
        pts = np.concatenate([lat(g.uniform(-ex, ex, (m, 2))), lat(g.uniform(-1.5, 3.5, (m, 1))), g.integers(0, 256, (m, 2)) / 256], 1).astype(np.float32)
        keep = _range_ok(pts, pr)
        for k in np.flatnonzero(valid):
            big = cb[k].astype(np.float64)
            big[3:6] = (cb[k, 3:6] + np.asarray(SAMPLER_CFG["REMOVE_EXTRA_WIDTH"], np.float32)).astype(np.float64)
            keep &= _box_ok(pts, big)
        keep[np.flatnonzero(keep)[n:]] = False                 # exactly n scene points
        assert keep.sum() == n
        frames.append(np.ascontiguousarray(pts[keep]))
        gt_boxes.append(gb)
        gt_names.append(names)
        obj, drawn = [], {}
        for (name, b, npts) in spec["cand"]:
            half = b[3:6].astype(np.float64) / 2
            m = npts + npts // 16 + 16
            lp = np.concatenate([lat(g.uniform(-half, half, (m, 3))), g.integers(0, 256, (m, 2)) / 256], 1).astype(np.float32)
            world = lp.copy()
            world[:, :3] += b[:3]
            lp = np.ascontiguousarray(lp[_range_ok(world, pr)][:npts])       # exactly npts object points
            assert len(lp) == npts
            obj.append(lp)
            db_pts.append(lp)
            db_off.append((row, row + len(lp)))
            row += len(lp)
            db_boxes.append(b)
            db_names.append(name)
            drawn.setdefault(name, []).append(per_class[name])
            per_class[name] += 1
        candidates.append([(n, np.asarray(drawn[n], np.int64)) for n in GROUPS if n in drawn])
        cands.append({"boxes": cb, "names": cn, "group": grp, "points": obj} if spec["cand"] else None)
    return {"frames": frames, "gt_boxes": gt_boxes, "gt_names": gt_names, "params": params, "candidates": candidates, "cands": cands,
            "db": {"points": np.concatenate(db_pts) if db_pts else np.zeros((0, 5), np.float32), "offsets": np.asarray(db_off, np.int64).reshape(-1, 2),
                   "boxes": np.stack(db_boxes) if db_boxes else np.zeros((0, 7), np.float32), "names": db_names}}


def statement(scene, **kw):
    return fr.pipeline(scene["frames"], scene["gt_boxes"], scene["gt_names"], CLASS_NAMES, PC_RANGE, scene["params"], cands=scene["cands"],
                       n_groups=len(GROUPS), extra_width=SAMPLER_CFG["REMOVE_EXTRA_WIDTH"], **kw)


PARAMS4 = [{"flip_x": False, "flip_y": True, "angle": -0.4, "scale": 0.97}, {"flip_x": True, "flip_y": False, "angle": 0.3, "scale": 1.02},
           {"flip_x": True, "flip_y": True, "angle": 0.7, "scale": 1.0}, {"flip_x": False, "flip_y": False, "angle": 0.0, "scale": 1.04}]


def crafted():
    """The sampling scene of the GPU test (B = 4)."""
    f0 = {"gt": [], "n": 120, "cand": [
        (*box("Vehicle", 0, 0, 0.25), 40), (*box("Vehicle", 1, 0.5, -0.5), 30),          # a mutual pair: both dropped
        (*box("Vehicle", 20, 0, 1.0), 25), (*box("Pedestrian", 10, 10, 0.5), 12), (*box("Pedestrian", -10, -10, 2.0), 9)]}
    f1 = {"gt": [box("Vehicle", 0, 0, 0.0), box("Pedestrian", 10, 0, 0.5), box("Sign", 20, 0, 0.0)], "n": 260, "cand": [
        (*box("Vehicle", 1, 0.5, 0.25), 20),                       # 0: hit by the GT vehicle
        (*box("Vehicle", 10.25, 0.25, 1.0), 20),                   # 1: hit by the GT pedestrian
        (*box("Vehicle", 20.5, 0, -0.25), 20),                     # 2: hit by the box with a foreign name
        (*box("Vehicle", 0, 10, 0.5), 35),                         # 3: valid; a pedestrian candidate lands on it
        (*box("Vehicle", 39.5, 0, 0.0), 60),                       # 4: valid; its points straddle the +x face after the transformation
        (*box("Vehicle", 38, 16.25, 0.0, z=3.5, size=(4.0, 2.0, 2.0)), 15),   # 5: valid; top above the range, one bottom corner inside
        (*box("Vehicle", 34, 38, 0.0), 15),                        # 6: valid; leaves the range entirely
        (*box("Pedestrian", 2.75, 1.25, 0.0), 10),                 # 7: over candidate 0, which is invalid -> valid
        (*box("Pedestrian", 0.5, 10.5, 0.75), 10),                 # 8: over candidate 3, which is valid -> dropped
        (*box("Pedestrian", -20, -20, 1.5), 10)]}                  # 9: valid
    f2 = {"gt": [box("Cyclist", 5, 5, 0.5)], "n": 0, "cand": [(*box("Vehicle", -5, -5, 0.5), 30), (*box("Pedestrian", 15, -5, 0.0), 8)]}
    gt3 = [box("Vehicle", -28 + 8 * k, -20, 0.25 * k) for k in range(8)] + [box("Pedestrian", -20 + 8 * k, 20, 0.5 * k) for k in range(4)]
    f3 = {"gt": gt3, "n": 300, "cand": []}                         # every LIMIT_WHOLE_SCENE quota is met by the frame itself
    return build(5, [f0, f1, f2, f3], PARAMS4)


def _grid_frame(g, n_scene, cand_points, n_gt=3):
    """GT boxes and candidates on an 8 m grid (cells never touch); every third candidate sits on a GT box or on its neighbour."""
    cells = [(x, y) for x in range(-32, 33, 8) for y in range(-32, 33, 8)]
    order = g.permutation(len(cells))
    gt = [box(CLASS_NAMES[k % 3], *cells[order[k]], heading=float(g.integers(-6, 7)) / 4) for k in range(n_gt)]
    cand, nv = [], sum(1 for k in range(len(cand_points)) if k % 2 == 0)
    for k, npts in enumerate(cand_points):
        name = "Vehicle" if k < nv else "Pedestrian"
        if k % 3 == 2:
            x, y = gt[k % n_gt][1][0] + 0.25, gt[k % n_gt][1][1] + 0.125
        else:
            x, y = cells[order[n_gt + k]]
        cand.append((*box(name, x, y, heading=float(g.integers(-6, 7)) / 4), npts))
    return {"gt": gt, "cand": cand, "n": n_scene}


def seams(total_hint):
    """Scan seams.  'small': below GD_SCAN_SINGLE_MAX rows in one workgroup's loop; 'tile': just above one GD_SCAN_TILE (4096 rows),
    an object segment and a frame boundary astride row 4096, a one-point candidate, an empty frame; 'multi': above
    GD_SCAN_SINGLE_MAX (65536), where the scan runs as tiles of 4096 rows, an object segment astride row 8192 and a frame boundary
    astride row 65536 - the lengths are chosen from the counts the margin filter leaves, so they are found by construction."""
    g = np.random.default_rng(17)
    if total_hint == "small":
        spec = [_grid_frame(g, 500, [20, 1, 30, 12]), {"gt": [], "cand": [], "n": 0}, _grid_frame(g, 700, [16, 9, 40])]
    elif total_hint == "tile":
        # rows: frame 0 = 60 + 1 + 50 object rows and 3900 scene rows (4011), frame 1 empty, frame 2 opens with a 400-point object
        # (rows 4011 - 4411, astride the seam at 4096; the tile before the seam holds the frame boundary): 4581 rows
        spec = [_grid_frame(g, 3900, [60, 1, 50]), {"gt": [], "cand": [], "n": 0}, _grid_frame(g, 150, [400, 20])]
    else:
        # rows: frame 0 ends at 8150, frame 1 opens with a 1500-point object astride row 8192 and ends at 9700, frame 2 ends at
        # 65525, frame 3 opens with a 3000-point object astride row 65536: 69430 rows
        spec = [_grid_frame(g, 8100, [30, 20]), _grid_frame(g, 40, [1500, 10]), _grid_frame(g, 55800, [25]), _grid_frame(g, 900, [3000, 5])]
    return build(23, spec, [PARAMS4[k % 4] for k in range(len(spec))])


def limits(n_cand, n_gt):
    """One frame with n_gt GT boxes on a 3.25 m grid (1 m boxes) and n_cand candidates, half of them on a GT box."""
    cells = [(x, y) for x in np.arange(-38, 39, 3.25) for y in np.arange(-38, 39, 3.25)]
    assert len(cells) >= n_gt + n_cand
    gt = [box("Cyclist" if k % 5 else "Sign", *cells[k], heading=0.25 * (k % 7), size=(1.0, 1.0, 1.0)) for k in range(n_gt)]
    cand = []
    for k in range(n_cand):
        name = "Vehicle" if k < n_cand // 2 else "Pedestrian"
        x, y = (cells[k][0] + 0.25, cells[k][1] + 0.25) if (k % 2 and k < n_gt) else cells[n_gt + k]
        cand.append((*box(name, x, y, heading=0.5 * (k % 5), size=(1.0, 1.0, 1.0)), 2))
    ident = {"flip_x": False, "flip_y": False, "angle": 0.0, "scale": 1.0}
    return build(3, [{"gt": gt, "cand": cand, "n": 20}], [ident])


def load_golden():
    """tests/golden/finetune_input.npz (make_golden_finetune_input.py) -> (npz, frames, gt_boxes, gt_names, params, perms)."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "finetune_input.npz"))
    nf = int(z["n_frames"])
    params = [{"flip_x": bool(z["flip_x"][i]), "flip_y": bool(z["flip_y"][i]), "angle": float(z["angle"][i]), "scale": float(z["scale"][i])}
              for i in range(nf)]
    return (z, [z[f"frame{i}"] for i in range(nf)], [z[f"boxes{i}"] for i in range(nf)], [z[f"names{i}"].tolist() for i in range(nf)], params,
            [z[f"perm{i}"].astype(np.int64) for i in range(nf)])
