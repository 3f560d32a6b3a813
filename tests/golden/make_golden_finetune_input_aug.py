"""Golden vectors for random_world_translation and random_world_drop in the fine-tune input pipeline ("translation and
drop").  Works as make_golden_finetune_input.py does: it runs the REFERENCE's own functions (imported through ref_harness) on seeded
synthetic frames WITH gt_boxes in the dict, on the augmentor list of waymo_models/gd_mae_ts.yaml - DataAugmentor.random_world_flip /
_rotation / _scaling / _translation / _drop called unbound, the heading limit_period of DataAugmentor.forward,
box_utils.mask_boxes_outside_range_numpy, common_utils.mask_points_by_range and DatasetTemplate.collate_batch.  The points carry an
extra last column with their row index, so the fixture records WHICH rows the reference's drop kept and in what order.  np.random is
seeded per frame (SEED + frame): the library's host draws follow the reference's stream up to and including the drop's enable draw,
not behind it (the reference draws its k-subset there, the library a seed).  Run in the build container:
    python tests/golden/make_golden_finetune_input_aug.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd"), os.path.join(REPO, "tests"), HERE]

import ref_harness  # noqa: E402
import finetune_input_aug_reference as far  # noqa: E402

ref_harness.install()
# stand-ins for what the reference modules import and the functions under test never touch (as make_golden_finetune_input.py)
for name in ("pcdet.datasets.augmentor", "pcdet.datasets.processor", "pcdet.ops.iou3d_nms", "pcdet.ops.roiaware_pool3d"):
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(ref_harness.REF, *name.split("."))]
    sys.modules[name] = m
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
for name, attrs in (("pcdet.utils.file_client", ()), ("pcdet.ops.iou3d_nms.iou3d_nms_utils", ()),
                    ("pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils", ()),
                    ("pcdet.datasets.processor.data_processor", ("DataProcessor",)),
                    ("pcdet.datasets.processor.point_feature_encoder", ("PointFeatureEncoder",))):
    m = types.ModuleType(name)
    for a in attrs:
        setattr(m, a, type(a, (), {}))
    sys.modules[name] = m
    setattr(sys.modules[name.rsplit(".", 1)[0]], name.rsplit(".", 1)[1], m)
DataAugmentor = ref_harness.ref("pcdet.datasets.augmentor.data_augmentor").DataAugmentor
common_utils = ref_harness.ref("pcdet.utils.common_utils")
box_utils = ref_harness.ref("pcdet.utils.box_utils")
DatasetTemplate = ref_harness.ref("pcdet.datasets.dataset").DatasetTemplate

PC_RANGE = np.array([-74.88, -74.88, -2, 74.88, 74.88, 4.0], np.float32)
CLASS_NAMES = ["Vehicle", "Pedestrian", "Cyclist"]
# tools/cfgs/waymo_models/gd_mae_ts.yaml:45-63 (gdmae_hip.configs.waymo_two_stage_data_cfg, which the harness's pcdet shadows here)
CFG = [
    {"NAME": "random_world_flip", "PROBABILITY": 0.5, "ALONG_AXIS_LIST": ["y"]},
    {"NAME": "random_world_rotation", "PROBABILITY": 0.7, "WORLD_ROT_ANGLE": [-3.14159265, 3.14159265]},
    {"NAME": "random_world_scaling", "PROBABILITY": 0.5, "WORLD_SCALE_RANGE": [0.9, 1.1]},
    {"NAME": "random_world_translation", "PROBABILITY": 0.5, "NOISE_TRANSLATE_STD": [0.2, 0.2, 0.2]},
    {"NAME": "random_world_drop", "PROBABILITY": 0.5, "DROP_RATIO": 0.1},
]
SEED = 4100
N_POINTS = (2000, 1900)


def main():
    from gdmae_hip import input_pipeline as ip
    cfg = CFG
    g = np.random.default_rng(29)
    frames, boxes, names = [], [], []
    for n in N_POINTS:
        xyz = g.uniform(-90, 90, (n, 3)).astype(np.float32)
        xyz[:, 2] = g.uniform(-2, 4, n)
        feats = (g.integers(0, 256, (n, 2)) / 256).astype(np.float32)
        frames.append(np.concatenate([xyz, feats, np.arange(n, dtype=np.float32)[:, None]], 1))      # last column: the row index
        m = int(g.integers(6, 11))
        bx = np.concatenate([g.uniform(-72, 72, (m, 2)), g.uniform(-1.5, 3.0, (m, 1)), g.uniform(0.6, 6.0, (m, 2)), g.uniform(0.8, 2.5, (m, 1)),
                             g.uniform(-np.pi, np.pi, (m, 1))], 1)
        bx[0, :2] = (g.uniform(73.5, 76.5), g.uniform(-30, 30))          # astride the +x face before the rotation
        bx[1, :2] = (g.uniform(-40, 40), g.uniform(-100, -90))           # far outside
        boxes.append(bx.astype(np.float32))
        names.append(np.asarray(g.choice(CLASS_NAMES + ["Sign"], m, p=[0.4, 0.25, 0.2, 0.15]), dtype=str))

    samples, params, rec = [], [], []
    for i, f in enumerate(frames):
        np.random.seed(SEED + i)
        d = {"points": f.copy(), "gt_boxes": boxes[i].copy(), "transformation_3d_list": [], "transformation_3d_params": {}}
        d = DataAugmentor.random_world_flip(None, d, cfg[0])
        d = DataAugmentor.random_world_rotation(None, d, cfg[1])
        d = DataAugmentor.random_world_scaling(None, d, cfg[2])
        pre_pts, pre_boxes = d["points"].copy(), d["gt_boxes"].copy()
        d = DataAugmentor.random_world_translation(None, d, cfg[3])
        post_pts, post_boxes = d["points"].copy(), d["gt_boxes"].copy()
        d = DataAugmentor.random_world_drop(None, d, cfg[4])
        assert d["points"].dtype == np.float32 and d["gt_boxes"].dtype == np.float32
        t = d["transformation_3d_params"]
        tr = np.asarray(t["random_world_translation"], np.float64).reshape(3)
        choice = d["points"][:, -1].astype(np.int64)
        assert np.array_equal(d["points"], post_pts[choice])
        dropped = len(choice) < len(f)
        params.append({"flip_x": "x" in t["random_world_flip"], "flip_y": "y" in t["random_world_flip"], "angle": float(t["random_world_rotation"]),
                       "scale": float(t["random_world_scaling"]), "translate": tr, "drop_q": 1 - cfg[4]["DROP_RATIO"] if dropped else 1.0, "drop_seed": 0})
        rec.append({"pre_pts": pre_pts, "pre_boxes": pre_boxes, "post_pts": post_pts, "post_boxes": post_boxes, "choice": choice, "dropped": dropped})
        d["gt_boxes"][:, 6] = common_utils.limit_period(d["gt_boxes"][:, 6], offset=0.5, period=2 * np.pi)
        sel = np.array([n in CLASS_NAMES for n in names[i]], bool)
        gb = d["gt_boxes"][sel]
        gb = np.concatenate([gb, np.array([CLASS_NAMES.index(n) + 1 for n in names[i][sel]], np.float32).reshape(-1, 1)], 1)
        gb = gb[box_utils.mask_boxes_outside_range_numpy(gb, PC_RANGE, min_num_corners=1)]
        pts = d["points"]
        pts = pts[common_utils.mask_points_by_range(pts, PC_RANGE)]
        samples.append({"points": pts, "gt_boxes": gb})
    col = DatasetTemplate.collate_batch(samples)
    exp_pts, exp_gt = col["points"].astype(np.float32), col["gt_boxes"]
    assert exp_gt.dtype == np.float32
    assert any(r["dropped"] for r in rec) and not all(r["dropped"] for r in rec), "need a frame that drops and one that does not"
    assert any(np.any(p["translate"] != 0) for p in params), "need a frame with the translation enabled"

    # the statement's translation, k and kept set on the reference's own intermediate arrays: bit for bit
    keys = []
    for i, (p, r) in enumerate(zip(params, rec)):
        assert np.array_equal(far.translate(r["pre_pts"], p["translate"]), r["post_pts"])
        assert np.array_equal(far.translate(r["pre_boxes"], p["translate"]), r["post_boxes"])
        n = len(frames[i])
        assert far.drop_count(p["drop_q"], n) == len(r["choice"])
        k = np.full(n, n, np.uint32)                                    # a row's key: its position in the recorded choice
        k[r["choice"]] = np.arange(len(r["choice"]), dtype=np.uint32)
        keys.append(k)
        assert np.array_equal(far.kept_rows(k, np.ones(n, bool), len(r["choice"])), np.sort(r["choice"]))
    # the whole statement against the reference's output: the reference leaves the kept rows in the order of its choice, the statement
    # in row order; perms puts the statement's rows (after the range mask) into the reference's order
    st = far.pipeline(frames, boxes, names, CLASS_NAMES, PC_RANGE, params, drop_keys=keys)
    perms, off = [], 0
    for b, s in enumerate(samples):
        mine = st["points"][off:off + st["kept"][b], -1]
        assert st["kept"][b] == len(s["points"]) and (np.diff(mine) > 0).all()
        perms.append(np.searchsorted(mine, s["points"][:, -1]).astype(np.int64))
        off += st["kept"][b]
    st = far.pipeline(frames, boxes, names, CLASS_NAMES, PC_RANGE, params, drop_keys=keys, perms=perms)
    assert st["points"].shape == exp_pts.shape and st["gt_boxes"].shape == exp_gt.shape
    assert np.array_equal(st["points"][:, 0], exp_pts[:, 0]) and np.array_equal(st["points"][:, 4:], exp_pts[:, 4:])
    assert np.array_equal(st["gt_boxes"][:, :, 7], exp_gt[:, :, 7])
    err_coord = max(np.abs(st["points"] - exp_pts).max(), np.abs(st["gt_boxes"][:, :, :6] - exp_gt[:, :, :6]).max())
    err_head = np.abs(st["gt_boxes"][:, :, 6] - exp_gt[:, :, 6]).max()
    assert err_coord <= 1e-5 and err_head <= 1e-6, (err_coord, err_head)

    # the library's host draws, from the same per-frame seeds, against what the reference drew
    pipe_cfg = CFG
    for i, p in enumerate(params):
        np.random.seed(SEED + i)
        w = ip.draw_world_params(pipe_cfg[:3])
        tr = ip.draw_translation(pipe_cfg[3])
        q, _ = ip.draw_drop(pipe_cfg[4])
        assert w == {k: p[k] for k in ("flip_x", "flip_y", "angle", "scale")} and np.array_equal(tr, p["translate"]) and q == p["drop_q"], i

    np.savez_compressed(
        os.path.join(HERE, "finetune_input_aug.npz"), pc_range=PC_RANGE, n_frames=len(frames), class_names=np.asarray(CLASS_NAMES), seed=SEED,
        **{f"frame{i}": f for i, f in enumerate(frames)}, **{f"boxes{i}": b for i, b in enumerate(boxes)},
        **{f"names{i}": n for i, n in enumerate(names)}, **{f"choice{i}": r["choice"].astype(np.int32) for i, r in enumerate(rec)},
        **{f"pre_points{i}": r["pre_pts"][:, :3] for i, r in enumerate(rec)}, **{f"pre_boxes{i}": r["pre_boxes"] for i, r in enumerate(rec)},
        **{f"post_points{i}": r["post_pts"][:, :3] for i, r in enumerate(rec)}, **{f"post_boxes{i}": r["post_boxes"] for i, r in enumerate(rec)},
        flip_x=np.array([p["flip_x"] for p in params]), flip_y=np.array([p["flip_y"] for p in params]),
        angle=np.array([p["angle"] for p in params], np.float64), scale=np.array([p["scale"] for p in params], np.float64),
        translate=np.stack([p["translate"] for p in params]), drop_q=np.array([p["drop_q"] for p in params], np.float64),
        dropped=np.array([r["dropped"] for r in rec]), expected_points=exp_pts, expected_gt_boxes=exp_gt,
        num_gt=np.asarray(st["num_gt"], np.int32), err_coord=np.float64(err_coord), err_heading=np.float64(err_head))
    print("wrote finetune_input_aug.npz: frames", [f.shape[0] for f in frames], "kept by the drop", [len(r["choice"]) for r in rec],
          "translate", [p["translate"].tolist() for p in params], "kept boxes", st["num_gt"],
          "max |statement - reference|: coordinates", err_coord, "headings", err_head)


if __name__ == "__main__":
    main()
