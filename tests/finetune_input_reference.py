"""Plain numpy statement of the fine-tune input contract.  Not a test: the CPU and GPU tests of the fine-tune
input pipeline compare against it, and tests/golden/make_golden_finetune_input.py pins its augmentation / range / collate half to
the reference's own functions.

    gt_sampling -> random_world_flip -> random_world_rotation -> random_world_scaling -> heading limit_period
      -> class selection + class column -> mask_points_and_boxes_outside_range -> shuffle_points -> collate_batch

Geometry DECISIONS are taken in float64 (pair overlap: oracle.iou3d_oracle.exact_overlap; point in box; corner / point in range);
the transformations are float32, operation by operation, as the reference's numpy / torch code performs them.  Every decision
reports its margin, so that a test can first assert that its scene keeps every decision away from the boundary an fp32 kernel
may legitimately place a hair differently:

  pair      overlap area of a hit pair [m^2], or the gap between the two rectangles of a miss [m]
  inbox     a point against an (enlarged) box: inside -> smallest slack to the three face pairs, outside -> largest violation [m]
            (the amount by which a face would have to move for the DECISION to change)
  range     a transformed point against the closed xy range, same convention [m]
  corner    a transformed box corner against the closed 3-D range, same convention [m]
"""
import math

import numpy as np

from oracle import input_oracle as io
from oracle.iou3d_oracle import exact_overlap

F32 = np.float32
IN_BOX_MARGIN = 1e-2


def _rect(b):
    c, s = math.cos(float(b[6])), math.sin(float(b[6]))
    hx, hy = float(b[3]) / 2, float(b[4]) / 2
    return [(float(b[0]) + lx * c - ly * s, float(b[1]) + lx * s + ly * c) for lx, ly in ((-hx, -hy), (hx, -hy), (hx, hy), (-hx, hy))]


def _pt_seg(p, a, b):
    dx, dy = b[0] - a[0], b[1] - a[1]
    L2 = dx * dx + dy * dy
    t = 0.0 if L2 == 0 else min(1.0, max(0.0, ((p[0] - a[0]) * dx + (p[1] - a[1]) * dy) / L2))
    return math.hypot(p[0] - a[0] - t * dx, p[1] - a[1] - t * dy)


def rect_gap(a, b):
    """Distance between two DISJOINT rotated rectangles (vertex to edge, both ways)."""
    ra, rb = _rect(a), _rect(b)
    return min(min(_pt_seg(p, rb[k], rb[(k + 1) % 4]) for p in ra for k in range(4)),
               min(_pt_seg(p, ra[k], ra[(k + 1) % 4]) for p in rb for k in range(4)))


def _hit(a, b, margins):
    far = math.hypot(float(a[0]) - float(b[0]), float(a[1]) - float(b[1])) - (math.hypot(a[3], a[4]) + math.hypot(b[3], b[4])) / 2
    if far > 1.0:                    # the circumscribed circles are more than a metre apart: a miss, with at least that gap
        margins["pair"] = min(margins["pair"], far)
        return False
    ov = exact_overlap(a, b)
    margins["pair"] = min(margins["pair"], ov if ov > 0 else rect_gap(a, b))
    return ov > 0


def select(gt_boxes, cand_boxes, cand_group, n_groups, margins):
    """Collision rule (database_sampler.py:242-251): -> valid flag per candidate."""
    existing = [np.asarray(b, np.float64) for b in gt_boxes]
    valid = np.zeros(len(cand_boxes), bool)
    for g in range(n_groups):
        idx = [c for c in range(len(cand_boxes)) if cand_group[c] == g]
        ok = []
        for c in idx:
            hit = False
            for e in existing:
                hit |= _hit(cand_boxes[c], e, margins)
            for k in idx:
                if k != c:
                    hit |= _hit(cand_boxes[c], cand_boxes[k], margins)
            if not hit:
                ok.append(c)
        for c in ok:
            valid[c] = True
            existing.append(np.asarray(cand_boxes[c], np.float64))
    return valid


def _slack(viol):
    """viol: per face pair, how far OUTSIDE the value lies (negative = inside by that much) -> (inside?, decision margin)."""
    viol = np.asarray(viol, np.float64)
    inside = bool((viol <= 0).all())
    return inside, float((-viol).min() if inside else viol[viol > 0].max())


def points_in_box(xyz, box, margins):
    """roiaware_pool3d.cpp:128-140 in float64: |z - cz| <= dz/2, |lx| < dx/2 + 1e-2, |ly| < dy/2 + 1e-2 in the frame rotated by
    -heading (the strict / closed difference is invisible at a non-zero margin)."""
    b = np.asarray(box, np.float64)
    p = np.asarray(xyz, np.float64)
    c, s = math.cos(-b[6]), math.sin(-b[6])
    sx, sy = p[:, 0] - b[0], p[:, 1] - b[1]
    lx, ly = sx * c - sy * s, sx * s + sy * c
    viol = np.stack([np.abs(p[:, 2] - b[2]) - b[5] / 2, np.abs(lx) - (b[3] / 2 + IN_BOX_MARGIN), np.abs(ly) - (b[4] / 2 + IN_BOX_MARGIN)], 1)
    inside = (viol[:, 0] <= 0) & (viol[:, 1] < 0) & (viol[:, 2] < 0)
    if len(p):
        m = np.where(inside, (-viol).min(1), np.where(viol > 0, viol, 0).max(1))
        margins["inbox"] = min(margins["inbox"], float(m.min()))
    return inside


def transform_boxes(boxes, pr):
    """fp32, operation by operation (data_augmentor.py:68-82, :107-108, :136, :247; common_utils.py:85-88)."""
    b = np.array(boxes, dtype=F32, copy=True).reshape(-1, 7)
    if pr["flip_x"]:
        b[:, 1] = -b[:, 1]
        b[:, 6] = -b[:, 6]
    if pr["flip_y"]:
        b[:, 0] = -b[:, 0]
        b[:, 6] = -(b[:, 6] + F32(np.pi))
    c, s = F32(np.cos(np.float64(pr["angle"]))), F32(np.sin(np.float64(pr["angle"])))
    b[:, :3] = b[:, :3] @ np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]], F32)
    b[:, 6] += F32(pr["angle"])
    b[:, :6] *= F32(pr["scale"])
    h = b[:, 6]
    b[:, 6] = h - np.floor(h / F32(2 * np.pi) + F32(0.5)) * F32(2 * np.pi)
    return b


def corners(b):
    """boxes_to_corners_3d (box_utils.py:28-53) of one box, float64 -> (8, 3)."""
    b = np.asarray(b, np.float64)
    t = np.array([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]], np.float64) / 2
    l = t * b[3:6]
    c, s = math.cos(b[6]), math.sin(b[6])
    return np.stack([l[:, 0] * c - l[:, 1] * s, l[:, 0] * s + l[:, 1] * c, l[:, 2]], 1) + b[:3]


def boxes_in_range(boxes, pc_range, min_num_corners, margins):
    r = np.asarray(pc_range, np.float64)
    keep = np.zeros(len(boxes), bool)
    for i, b in enumerate(boxes):
        n = 0
        for p in corners(b):
            inside, m = _slack(np.concatenate([r[:3] - p, p - r[3:]]))
            margins["corner"] = min(margins["corner"], m)
            n += inside
        keep[i] = n >= min_num_corners
    return keep


def points_in_range(p, pc_range, margins):
    r = np.asarray(pc_range, np.float64)
    q = np.asarray(p[:, :2], np.float64)
    viol = np.concatenate([r[:2] - q, q - r[3:5]], 1)
    inside = (viol <= 0).all(1)
    if len(q):
        m = np.where(inside, (-viol).min(1), np.where(viol > 0, viol, 0).max(1))
        margins["range"] = min(margins["range"], float(m.min()))
    return inside


def pipeline(frames, gt_boxes, gt_names, class_names, pc_range, params, cands=None, n_groups=0, extra_width=(0.0, 0.0, 0.0),
             remove_points=True, min_num_corners=1, perms=None):
    """cands: per frame None or {'boxes' (k, 7), 'names' (k), 'group' (k), 'points' [k arrays (n, F) of LOCAL points]}.
    -> {'points' (N, 1 + F), 'gt_boxes' (B, max_gt, 8), 'num_gt', 'kept' (points per frame), 'valid' (per frame), 'margins'}."""
    margins = {"pair": math.inf, "inbox": math.inf, "range": math.inf, "corner": math.inf}
    class_names = list(class_names)
    out_pts, out_boxes, kept, valids = [], [], [], []
    for b, (f, pr) in enumerate(zip(frames, params)):
        gb = np.asarray(gt_boxes[b], F32).reshape(-1, 7)
        names = np.asarray(gt_names[b]).astype(str).reshape(-1)
        sel = np.array([n in class_names for n in names], bool)
        boxes = gb[sel]
        cls = [class_names.index(n) + 1 for n in names[sel]]
        pts = np.asarray(f, F32)
        cd = cands[b] if cands is not None else None
        if cd is not None and len(cd["boxes"]):
            cb = np.asarray(cd["boxes"], F32).reshape(-1, 7)
            valid = select(gb, cb, list(cd["group"]), n_groups, margins)
            obj = [np.concatenate([np.asarray(p, F32)[:, :3] + cb[k, :3], np.asarray(p, F32)[:, 3:]], 1) for k, p in enumerate(cd["points"]) if valid[k]]
            if remove_points and valid.any():
                inside = np.zeros(len(pts), bool)
                for k in np.flatnonzero(valid):
                    big = cb[k].astype(np.float64)
                    big[3:6] = (cb[k, 3:6] + np.asarray(extra_width, F32)).astype(np.float64)
                    inside |= points_in_box(pts[:, :3], big, margins)
                pts = pts[~inside]
            pts = np.concatenate(obj + [pts]).astype(F32)
            boxes = np.concatenate([boxes, cb[valid]])
            cls += [class_names.index(n) + 1 for n in np.asarray(cd["names"]).astype(str)[valid]]
        else:
            valid = np.zeros(0, bool)
        valids.append(valid)
        p = io.augment_frame(pts, pr["flip_x"], pr["flip_y"], pr["angle"], pr["scale"])
        p = p[points_in_range(p, pc_range, margins)]
        kept.append(p.shape[0])
        if perms is not None:
            p = p[perms[b]]
        out_pts.append(np.pad(p, ((0, 0), (1, 0)), mode="constant", constant_values=b))
        tb = transform_boxes(boxes, pr)
        tb = np.concatenate([tb, np.asarray(cls, F32).reshape(-1, 1)], 1)
        out_boxes.append(tb[boxes_in_range(tb[:, :7], pc_range, min_num_corners, margins)])
    num_gt = [len(x) for x in out_boxes]
    gt = np.zeros((len(frames), max(num_gt) if num_gt else 0, 8), F32)
    for b, x in enumerate(out_boxes):
        gt[b, :len(x)] = x
    return {"points": np.concatenate(out_pts, 0).astype(F32), "gt_boxes": gt, "num_gt": num_gt, "kept": kept, "valid": valids,
            "margins": margins}
