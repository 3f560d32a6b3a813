"""Plain numpy statement of the fine-tune input contract with ``random_world_translation`` and ``random_world_drop`` (DESIGN §7l,
"translation and drop").  Not a test.  It adds to tests/finetune_input_reference.py, whose functions it calls:

    gt_sampling -> flip -> rotation -> scaling -> translation -> drop -> heading limit_period -> range masks -> shuffle -> collate

  translate      numpy's in-place ``float32 += float64`` (data_augmentor.py:162-164): fp64 sum, one rounding to fp32
  eligible rows  of a frame's virtual rows (every candidate's object points in candidate order, then the scene points): the rows the
                 reference's ``points`` holds after gt_sampling
  drop_count     Python's ``int(q * n)`` with q = ``1 - DROP_RATIO`` (data_augmentor.py:50)
  hashed_keys    the device's counter-based keys in numpy uint64: upper half of splitmix64's finaliser on
                 ``seed + (j + 1) * 0x9E3779B97F4A7C15``, j = the row's index among the frame's virtual rows
  kept_rows      the first k of a stable sort of the eligible rows by key (ties go to the lower row), as ascending row indices
"""
import math

import numpy as np

import finetune_input_reference as fr
from oracle import input_oracle as io

F32 = np.float32
U64 = np.uint64


def translate(a, t):
    """a (n, >= 3) float32, t (3) float64 -> a copy whose columns 0-2 went through the reference's own statement."""
    a = np.array(a, dtype=F32, copy=True)
    a[:, :3] += np.asarray(t, np.float64).reshape(1, 3)
    return a


def drop_count(q, n):
    return int(q * n)


def hashed_keys(seed, n):
    with np.errstate(over="ignore"):
        z = U64(int(seed) & 0xFFFFFFFFFFFFFFFF) + (np.arange(n, dtype=U64) + U64(1)) * U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        z = z ^ (z >> U64(31))
    return (z >> U64(32)).astype(np.uint32)


def kept_rows(keys, eligible, k):
    """keys (n) uint32 over the virtual rows, eligible (n) bool -> ascending virtual rows of the k kept ones."""
    rows = np.flatnonzero(eligible)
    order = np.argsort(np.asarray(keys)[rows], kind="stable")[:k]
    return np.sort(rows[order])


def virtual_rows(frame, gt_boxes, cand, n_groups, extra_width, remove_points, margins):
    """-> (rows (n, F) float32 before the world transformation, eligible (n) bool, valid (candidates) bool)."""
    pts = np.asarray(frame, F32)
    if cand is None or not len(cand["boxes"]):
        return pts, np.ones(len(pts), bool), np.zeros(0, bool)
    cb = np.asarray(cand["boxes"], F32).reshape(-1, 7)
    valid = fr.select(np.asarray(gt_boxes, F32).reshape(-1, 7), cb, list(cand["group"]), n_groups, margins)
    obj = [np.concatenate([np.asarray(p, F32)[:, :3] + cb[k, :3], np.asarray(p, F32)[:, 3:]], 1) for k, p in enumerate(cand["points"])]
    el = [np.full(len(p), bool(valid[k])) for k, p in enumerate(obj)]
    inside = np.zeros(len(pts), bool)
    if remove_points:
        for k in np.flatnonzero(valid):
            big = cb[k].astype(np.float64)
            big[3:6] = (cb[k, 3:6] + np.asarray(extra_width, F32)).astype(np.float64)
            inside |= fr.points_in_box(pts[:, :3], big, margins)
    return np.concatenate(obj + [pts]).astype(F32), np.concatenate(el + [~inside]), valid


def pipeline(frames, gt_boxes, gt_names, class_names, pc_range, params, cands=None, n_groups=0, extra_width=(0.0, 0.0, 0.0),
             remove_points=True, min_num_corners=1, perms=None, translation=True, drop_keys=None):
    """fr.pipeline with the two augmentors.  params: fr.pipeline's dicts plus 'translate' (3 float64), 'drop_q', 'drop_seed' (absent:
    zero translation, q = 1).  translation: the augmentor is in the list (the add is performed, also with t = 0).  drop_keys: per frame
    None or uint32 keys over the virtual rows, instead of the hashed ones.
    -> fr.pipeline's dict plus 'drop_n', 'drop_k' and 'rows' (per frame the virtual rows the drop kept, before the range mask)."""
    margins = {"pair": math.inf, "inbox": math.inf, "range": math.inf, "corner": math.inf}
    class_names = list(class_names)
    out_pts, out_boxes, kept, valids, drop_n, drop_k, rows_out = [], [], [], [], [], [], []
    for b, (f, pr) in enumerate(zip(frames, params)):
        gb = np.asarray(gt_boxes[b], F32).reshape(-1, 7)
        names = np.asarray(gt_names[b]).astype(str).reshape(-1)
        sel = np.array([n in class_names for n in names], bool)
        boxes = gb[sel]
        cls = [class_names.index(n) + 1 for n in names[sel]]
        cd = cands[b] if cands is not None else None
        rows, eligible, valid = virtual_rows(f, gb, cd, n_groups, extra_width, remove_points, margins)
        if len(valid):
            boxes = np.concatenate([boxes, np.asarray(cd["boxes"], F32).reshape(-1, 7)[valid]])
            cls += [class_names.index(n) + 1 for n in np.asarray(cd["names"]).astype(str)[valid]]
        valids.append(valid)
        n = int(eligible.sum())
        k = drop_count(float(pr.get("drop_q", 1.0)), n)
        keys = drop_keys[b] if drop_keys is not None and drop_keys[b] is not None else hashed_keys(pr.get("drop_seed", 0), len(rows))
        keep = kept_rows(keys, eligible, k)
        drop_n.append(n)
        drop_k.append(k)
        rows_out.append(keep)
        p = io.augment_frame(rows[keep], pr["flip_x"], pr["flip_y"], pr["angle"], pr["scale"])
        if translation:
            p = translate(p, pr.get("translate", np.zeros(3)))
        p = p[fr.points_in_range(p, pc_range, margins)]
        kept.append(p.shape[0])
        if perms is not None:
            p = p[perms[b]]
        out_pts.append(np.pad(p, ((0, 0), (1, 0)), mode="constant", constant_values=b))
        tb = fr.transform_boxes(boxes, pr)
        if translation:
            tb = translate(tb, pr.get("translate", np.zeros(3)))
        tb = np.concatenate([tb, np.asarray(cls, F32).reshape(-1, 1)], 1)
        out_boxes.append(tb[fr.boxes_in_range(tb[:, :7], pc_range, min_num_corners, margins)])
    num_gt = [len(x) for x in out_boxes]
    gt = np.zeros((len(frames), max(num_gt) if num_gt else 0, 8), F32)
    for b, x in enumerate(out_boxes):
        gt[b, :len(x)] = x
    return {"points": np.concatenate(out_pts, 0).astype(F32), "gt_boxes": gt, "num_gt": num_gt, "kept": kept, "valid": valids,
            "margins": margins, "drop_n": drop_n, "drop_k": drop_k, "rows": rows_out}
