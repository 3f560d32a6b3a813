"""Scenes and fixture loader shared by the CPU and GPU tests of random_world_translation / random_world_drop in the fine-tune input
pipeline (not a test)."""
import os

import numpy as np

import finetune_input_scenes as sc

IDENT = {"flip_x": False, "flip_y": False, "angle": 0.0, "scale": 1.0}
T_ISSUE = np.array([0.212, -0.312, 0.051], np.float64)
TRANSLATE_CFG = {"NAME": "random_world_translation", "PROBABILITY": 0.5, "NOISE_TRANSLATE_STD": [0.2, 0.2, 0.2]}
DROP_CFG = {"NAME": "random_world_drop", "PROBABILITY": 0.5, "DROP_RATIO": 0.1}
WAYMO_RANGE = np.array([-74.88, -74.88, -2, 74.88, 74.88, 4.0], np.float32)
UNIFORMITY_SEEDS = [0x1234567 + 0x9E3779B1 * s for s in range(256)]
UNIFORMITY_ROWS, UNIFORMITY_BOUNDS = 4096, (84, 172)          # Binomial(256, 1/2) +- 5.5 sigma


def translation_scene(n=4000, m=6):
    """One frame of n points uniform over +-75 m (row index in the last column) and m boxes, for the bit-exactness of the add."""
    g = np.random.default_rng(3)
    pts = np.concatenate([g.uniform(-75, 75, (n, 2)), g.uniform(-2, 4, (n, 1)), g.integers(0, 256, (n, 1)) / 256, np.arange(n)[:, None]], 1).astype(np.float32)
    boxes = np.concatenate([g.uniform(-60, 60, (m, 2)), g.uniform(-1, 2, (m, 1)), g.uniform(1, 5, (m, 3)), g.uniform(-3, 3, (m, 1))], 1).astype(np.float32)
    return pts, boxes, ["Vehicle", "Pedestrian", "Cyclist", "Vehicle", "Sign", "Vehicle"][:m]


def indexed_frame(n, seed, extent=30.0):
    """n points well inside sc.PC_RANGE, 4 columns, the row index in the last one."""
    g = np.random.default_rng(seed)
    return np.concatenate([g.uniform(-extent, extent, (n, 2)), g.uniform(-1, 3, (n, 1)), np.arange(n)[:, None]], 1).astype(np.float32)


def crafted_with_drop():
    """sc.crafted() (invalid candidates, removed scene points, a frame without scene points, a frame without candidates) with a
    translation whose range decisions keep 1e-3 m of margin and a drop in frames 0, 2 and 3."""
    s = sc.crafted()
    t = [np.array([0.203125, -0.296875, 0.046875]), np.zeros(3), np.array([-0.109375, 0.140625, 0.015625]), np.array([0.0625, 0.03125, -0.125])]
    q = [1 - 0.1, 1.0, 1 - 0.5, 1 - 0.3]
    s["params"] = [dict(p, translate=t[b], drop_q=q[b], drop_seed=77 + 1000003 * b) for b, p in enumerate(s["params"])]
    return s


def load_golden():
    """tests/golden/finetune_input_aug.npz (make_golden_finetune_input_aug.py) -> (npz, frames, gt_boxes, gt_names, params, keys):
    keys[b][row] = the row's position in the reference's recorded choice (rows it dropped: the frame's row count)."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "finetune_input_aug.npz"))
    nf = int(z["n_frames"])
    params = [{"flip_x": bool(z["flip_x"][i]), "flip_y": bool(z["flip_y"][i]), "angle": float(z["angle"][i]), "scale": float(z["scale"][i]),
               "translate": z["translate"][i].astype(np.float64), "drop_q": float(z["drop_q"][i]), "drop_seed": 0} for i in range(nf)]
    frames = [z[f"frame{i}"] for i in range(nf)]
    keys = []
    for i, f in enumerate(frames):
        k = np.full(len(f), len(f), np.uint32)
        k[z[f"choice{i}"]] = np.arange(len(z[f"choice{i}"]), dtype=np.uint32)
        keys.append(k)
    return z, frames, [z[f"boxes{i}"] for i in range(nf)], [z[f"names{i}"].tolist() for i in range(nf)], params, keys


def golden_perms(z, kept_idx):
    """kept_idx: per frame the row-index column of the rows a pipeline kept, in its (ascending) order -> the permutation that puts them
    into the order of the reference's output (its choice order)."""
    exp = z["expected_points"]
    return [np.searchsorted(kept_idx[b], exp[exp[:, 0] == b][:, -1]).astype(np.int64) for b in range(int(z["n_frames"]))]
