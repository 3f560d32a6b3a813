"""Golden vectors for the fine-tune input pipeline: runs the REFERENCE's own functions (imported from /root/reference
through ref_harness) on seeded synthetic frames WITH gt_boxes in the dict - DataAugmentor.random_world_flip / _rotation / _scaling,
the heading limit_period of DataAugmentor.forward, box_utils.mask_boxes_outside_range_numpy, common_utils.mask_points_by_range, the
np.random.permutation shuffle and DatasetTemplate.collate_batch - and records the index sequence of the reference's
DataBaseSampler.sample_with_fixed_number.  Stores inputs, the decisions the reference drew and its collated output, and asserts
that tests/finetune_input_reference.py reproduces them.  Run in the build container:
    python tests/golden/make_golden_finetune_input.py

DataBaseSampler.__call__ itself needs the reference's compiled CPU IoU / point-in-box extensions, which are not built here: the
sampling half of the contract is pinned by the numpy statement and closed-form cases (tests/test_finetune_input_cpu.py).
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd"), os.path.join(REPO, "tests"), HERE]

import ref_harness  # noqa: E402
import finetune_input_reference as fr  # noqa: E402

ref_harness.install()
# stand-ins for what the reference modules import and the functions under test never touch (cv2, the file client, the compiled
# IoU / RoI-aware pooling extensions, the voxel generator wrapper)
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
DataBaseSampler = ref_harness.ref("pcdet.datasets.augmentor.database_sampler").DataBaseSampler
DataAugmentor = ref_harness.ref("pcdet.datasets.augmentor.data_augmentor").DataAugmentor
common_utils = ref_harness.ref("pcdet.utils.common_utils")
box_utils = ref_harness.ref("pcdet.utils.box_utils")
DatasetTemplate = ref_harness.ref("pcdet.datasets.dataset").DatasetTemplate

PC_RANGE = np.array([-74.88, -74.88, -2, 74.88, 74.88, 4.0], np.float32)
CLASS_NAMES = ["Vehicle", "Pedestrian", "Cyclist"]
CFG = [
    {"NAME": "random_world_flip", "PROBABILITY": 0.5, "ALONG_AXIS_LIST": ["x", "y"]},
    {"NAME": "random_world_rotation", "PROBABILITY": 1.0, "WORLD_ROT_ANGLE": [-0.78539816, 0.78539816]},
    {"NAME": "random_world_scaling", "PROBABILITY": 1.0, "WORLD_SCALE_RANGE": [0.95, 1.05]},
]
# the sampler's own run: a database of 7 + 3 entries, quotas 3 and 2, five frames whose own objects lower the quota
DB_SIZES = {"Vehicle": 7, "Pedestrian": 3}
SAMPLE_GROUPS = ["Vehicle:3", "Pedestrian:2"]
SAMPLER_NAMES = [[], ["Vehicle", "Sign"], ["Pedestrian"], ["Vehicle", "Vehicle", "Cyclist"], []]


def reference_draw(sampler, groups, class_num, gt_names):
    """Lines 230-235 of DataBaseSampler.__call__ (LIMIT_WHOLE_SCENE) around the reference's sample_with_fixed_number."""
    out = []
    for name, group in groups.items():
        group["sample_num"] = str(int(class_num[name]) - int(np.sum(name == np.asarray(gt_names, dtype=str))))
        if int(group["sample_num"]) > 0:
            out.append((name, np.asarray(sampler.sample_with_fixed_number(name, group), np.int64)))
    return out


def main():
    g = np.random.default_rng(11)
    frames, boxes, names = [], [], []
    for n in (3000, 2500, 1, 3500):
        xyz = g.uniform(-90, 90, (n, 3)).astype(np.float32)
        xyz[:, 2] = g.uniform(-2, 4, n)
        frames.append(np.concatenate([xyz, (g.integers(0, 256, (n, 2)) / 256).astype(np.float32)], 1))      # 8-bit features: a smaller file
        m = int(g.integers(6, 13))
        bx = np.concatenate([g.uniform(-72, 72, (m, 2)), g.uniform(-1.5, 3.0, (m, 1)), g.uniform(0.6, 6.0, (m, 2)), g.uniform(0.8, 2.5, (m, 1)),
                             g.uniform(-np.pi, np.pi, (m, 1))], 1)
        bx[0, :2] = (g.uniform(73.5, 76.5), g.uniform(-30, 30))          # straddles the +x face of the range (before the rotation)
        bx[1, :2] = (g.uniform(-40, 40), g.uniform(-100, -90))           # far outside
        bx[2, 2] = g.uniform(3.6, 4.4)                                   # straddles the top face
        boxes.append(bx.astype(np.float32))
        names.append(np.asarray(g.choice(CLASS_NAMES + ["Sign"], m, p=[0.4, 0.25, 0.2, 0.15]), dtype=str))

    sampler = DataBaseSampler.__new__(DataBaseSampler)                   # no __init__: no files, no backend
    sampler.use_shared_memory = False                                    # read by its __del__
    sampler.db_infos = {k: list(range(v)) for k, v in DB_SIZES.items()}
    class_num = {x.split(":")[0]: x.split(":")[1] for x in SAMPLE_GROUPS}
    groups = {k: {"sample_num": class_num[k], "pointer": len(sampler.db_infos[k]), "indices": np.arange(len(sampler.db_infos[k]))} for k in class_num}

    np.random.seed(321)
    state0 = np.random.get_state()
    samples, params, perms, draws = [], [], [], []
    for i, f in enumerate(frames):
        draws.append(reference_draw(sampler, groups, class_num, SAMPLER_NAMES[i]))       # gt_sampling comes first in the queue
        d = {"points": f.copy(), "gt_boxes": boxes[i].copy(), "transformation_3d_list": [], "transformation_3d_params": {}}
        d = DataAugmentor.random_world_flip(None, d, CFG[0])
        d = DataAugmentor.random_world_rotation(None, d, CFG[1])
        d = DataAugmentor.random_world_scaling(None, d, CFG[2])
        d["gt_boxes"][:, 6] = common_utils.limit_period(d["gt_boxes"][:, 6], offset=0.5, period=2 * np.pi)
        t = d["transformation_3d_params"]
        params.append({"flip_x": "x" in t["random_world_flip"], "flip_y": "y" in t["random_world_flip"],
                       "angle": float(t["random_world_rotation"]), "scale": float(t["random_world_scaling"])})
        sel = np.array([n in CLASS_NAMES for n in names[i]], bool)                           # dataset.py:138-144
        gb = d["gt_boxes"][sel]
        gb = np.concatenate([gb, np.array([CLASS_NAMES.index(n) + 1 for n in names[i][sel]], np.float32).reshape(-1, 1)], 1)
        assert gb.dtype == np.float32
        gb = gb[box_utils.mask_boxes_outside_range_numpy(gb, PC_RANGE, min_num_corners=1)]
        pts = d["points"]
        pts = pts[common_utils.mask_points_by_range(pts, PC_RANGE)]
        perm = np.random.permutation(pts.shape[0])
        perms.append(perm)
        samples.append({"points": pts[perm], "gt_boxes": gb})
    draws.append(reference_draw(sampler, groups, class_num, SAMPLER_NAMES[4]))
    col = DatasetTemplate.collate_batch(samples)
    exp_pts, exp_gt = col["points"].astype(np.float32), col["gt_boxes"]
    assert exp_gt.dtype == np.float32

    # the numpy statement with the recorded decisions must reproduce the reference
    st = fr.pipeline(frames, boxes, names, CLASS_NAMES, PC_RANGE, params, perms=perms)
    assert st["points"].shape == exp_pts.shape and st["gt_boxes"].shape == exp_gt.shape, (st["gt_boxes"].shape, exp_gt.shape)
    assert st["num_gt"] == [len(s["gt_boxes"]) for s in samples]
    assert np.array_equal(st["points"][:, 0], exp_pts[:, 0]) and np.array_equal(st["points"][:, 4:], exp_pts[:, 4:])
    assert np.array_equal(st["gt_boxes"][:, :, 7], exp_gt[:, :, 7])
    err_coord = max(np.abs(st["points"] - exp_pts).max(), np.abs(st["gt_boxes"][:, :, :6] - exp_gt[:, :, :6]).max())
    err_head = np.abs(st["gt_boxes"][:, :, 6] - exp_gt[:, :, 6]).max()
    assert err_coord <= 1e-5 and err_head <= 1e-6, (err_coord, err_head)

    # and the library's host draws, from the same np.random state, must agree with what the reference drew
    from gdmae_hip import input_pipeline as ip
    np.random.set_state(state0)
    sstate = ip.sampler_state({"SAMPLE_GROUPS": SAMPLE_GROUPS, "LIMIT_WHOLE_SCENE": True}, DB_SIZES, CLASS_NAMES)
    for i in range(5):
        mine = ip.draw_candidates(sstate, SAMPLER_NAMES[i])
        assert [n for n, _ in mine] == [n for n, _ in draws[i]] and all(np.array_equal(a[1], b[1]) for a, b in zip(mine, draws[i])), (i, mine, draws[i])
        if i < 4:
            assert ip.draw_world_params(CFG) == params[i]
            assert np.array_equal(np.random.permutation(len(perms[i])), perms[i])

    flat = [(i, CLASS_NAMES.index(n), int(v)) for i, dr in enumerate(draws) for n, idx in dr for v in idx]
    np.savez_compressed(
        os.path.join(HERE, "finetune_input.npz"), pc_range=PC_RANGE, n_frames=len(frames), class_names=np.asarray(CLASS_NAMES),
        **{f"frame{i}": f for i, f in enumerate(frames)}, **{f"perm{i}": p.astype(np.int32) for i, p in enumerate(perms)},
        **{f"boxes{i}": b for i, b in enumerate(boxes)}, **{f"names{i}": n for i, n in enumerate(names)},
        flip_x=np.array([p["flip_x"] for p in params]), flip_y=np.array([p["flip_y"] for p in params]),
        angle=np.array([p["angle"] for p in params], np.float64), scale=np.array([p["scale"] for p in params], np.float64),
        expected_points=exp_pts, expected_gt_boxes=exp_gt, num_gt=np.asarray(st["num_gt"], np.int32),
        err_coord=np.float64(err_coord), err_heading=np.float64(err_head),
        sampler_seed=321, sampler_groups=np.asarray(SAMPLE_GROUPS), sampler_db_names=np.asarray(list(DB_SIZES)),
        sampler_db_sizes=np.asarray(list(DB_SIZES.values()), np.int32),
        **{f"sampler_names{i}": np.asarray(n, dtype="U16") for i, n in enumerate(SAMPLER_NAMES)},
        sampler_draws=np.asarray(flat, np.int32).reshape(-1, 3))                 # rows [frame, class, index into the class's list]
    print("wrote finetune_input.npz: frames", [f.shape[0] for f in frames], "boxes", [len(b) for b in boxes], "kept boxes", st["num_gt"],
          "max |statement - reference|: coordinates", err_coord, "headings", err_head, "margins", st["margins"])


if __name__ == "__main__":
    main()
