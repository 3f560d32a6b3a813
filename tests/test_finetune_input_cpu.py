"""Fine-tune input pipeline, CPU half: the numpy statement against the reference golden, the host draws against the
sequence the reference's sampler produced, closed-form sampling cases, the database reader and the refusals."""
import os
import pickle

import numpy as np
import pytest
import torch

import finetune_input_reference as fr
import finetune_input_scenes as sc
from gdmae_hip import configs, input_pipeline as ip, lib as L

REF_YAML = "/root/reference/tools/cfgs/waymo_models/gd_mae.yaml"
CPU = torch.device("cpu")


def test_statement_matches_reference_golden():
    z, frames, boxes, names, params, perms = sc.load_golden()
    st = fr.pipeline(frames, boxes, names, z["class_names"].tolist(), z["pc_range"], params, perms=perms)
    ep, eg = z["expected_points"], z["expected_gt_boxes"]
    assert st["points"].shape == ep.shape and st["gt_boxes"].shape == eg.shape and st["num_gt"] == z["num_gt"].tolist()
    assert np.array_equal(st["points"][:, 0], ep[:, 0]) and np.array_equal(st["points"][:, 4:], ep[:, 4:])
    assert np.array_equal(st["gt_boxes"][:, :, 7], eg[:, :, 7])
    assert np.abs(st["points"] - ep).max() <= float(z["err_coord"])
    assert np.abs(st["gt_boxes"][:, :, :6] - eg[:, :, :6]).max() <= float(z["err_coord"])
    assert np.abs(st["gt_boxes"][:, :, 6] - eg[:, :, 6]).max() <= float(z["err_heading"])
    assert any(0 < n < len(b) for n, b in zip(st["num_gt"], boxes))          # some boxes were dropped, some kept


def test_candidates_and_world_parameters_are_drawn_like_the_reference():
    """The recorded run: per frame the sampler's draws (two groups, 7 and 3 database entries, the pointer wraps twice), then the
    world parameters, then the reference's shuffle draw."""
    z, frames, boxes, names, params, perms = sc.load_golden()
    sizes = dict(zip(z["sampler_db_names"].tolist(), z["sampler_db_sizes"].tolist()))
    cls = z["class_names"].tolist()
    state = ip.sampler_state({"SAMPLE_GROUPS": z["sampler_groups"].tolist(), "LIMIT_WHOLE_SCENE": True}, sizes, cls)
    rec = z["sampler_draws"]
    np.random.seed(int(z["sampler_seed"]))
    permutations = 0
    for i in range(5):
        before = [g["pointer"] for g in state["groups"]]
        mine = ip.draw_candidates(state, z[f"sampler_names{i}"].tolist())
        permutations += sum(g["pointer"] < b for g, b in zip(state["groups"], before))
        flat = [(i, cls.index(n), int(v)) for n, idx in mine for v in idx]
        assert flat == [tuple(r) for r in rec[rec[:, 0] == i].tolist()], i
        if i < 4:
            assert ip.draw_world_params(ip.FINETUNE_AUG_CONFIG[1:]) == params[i]
            assert np.array_equal(np.random.permutation(len(perms[i])), perms[i])
    assert permutations >= 4                                                   # first fill of both classes + at least two wraps


U = (1.0, 1.0, 1.0)


def _select(gt, cand, group, n_groups=2):
    return fr.select(np.asarray(gt, np.float32).reshape(-1, 7), np.asarray(cand, np.float32).reshape(-1, 7), group, n_groups, {"pair": np.inf}).tolist()


def _b(x, y, h=0.0):
    return [x, y, 0.0, *U, h]


def test_closed_form_collision_rule():
    assert _select([], [_b(0, 0), _b(1.5, 0)], [0, 0]) == [True, True]                # 0.5 m apart
    assert _select([], [_b(0, 0), _b(0.5, 0)], [0, 0]) == [False, False]              # a mutual pair: both dropped
    # the existing boxes are ALL of the frame's GT boxes: the pipeline passes those with a foreign name too
    s = fr.pipeline([np.zeros((0, 5), np.float32)], [np.asarray([_b(0, 0)], np.float32)], [["Sign"]], ["Vehicle"], [-9, -9, -2, 9, 9, 4],
                    [{"flip_x": False, "flip_y": False, "angle": 0.0, "scale": 1.0}],
                    cands=[{"boxes": [_b(0.5, 0), _b(4, 0)], "names": ["Vehicle", "Vehicle"], "group": [0, 0], "points": [np.zeros((1, 5), np.float32)] * 2}], n_groups=1)
    assert s["valid"][0].tolist() == [False, True] and s["num_gt"] == [1] and s["kept"] == [1]
    assert _select([], [_b(0, 0), _b(0.5, 0)], [0, 1]) == [True, False]               # second group over a first-group VALID one
    assert _select([_b(0, 0)], [_b(0.75, 0), _b(1.5, 0)], [0, 1]) == [False, True]    # ... over a first-group INVALID one: valid


def test_closed_form_point_removal():
    box = np.array([2.0, 1.0, 0.5, 4.0, 2.0, 1.0, 0.5], np.float64)
    ax = np.array([np.cos(0.5), np.sin(0.5)])
    on_axis = lambda d, z=0.5: [2.0 + d * ax[0], 1.0 + d * ax[1], z]          # noqa: E731
    pts = np.array([on_axis(2.0 + 0.005), on_axis(2.0 + 0.02), on_axis(0.0, 1.0), on_axis(0.0, 1.0 + 1e-6)], np.float64)
    m = {"inbox": np.inf}
    assert fr.points_in_box(pts, box, m).tolist() == [True, False, True, False]       # inside = removed from the scene
    assert m["inbox"] == 0.0                                                          # |z - cz| = dz / 2 exactly sits ON the face


def test_database_reader_and_prepare(tmp_path):
    pts = np.arange(50, dtype=np.float32).reshape(10, 5)
    info = lambda name, a, b, n, d: {"name": name, "global_data_offset": [a, b], "box3d_lidar": np.arange(7, dtype=np.float64) + a,      # noqa: E731
                                     "num_points_in_gt": n, "difficulty": d, "path": "unused"}
    with open(tmp_path / "a.pkl", "wb") as f:
        pickle.dump({"Vehicle": [info("Vehicle", 0, 3, 3, 0), info("Vehicle", 3, 4, 1, 0)], "Pedestrian": [info("Pedestrian", 4, 6, 2, -1)]}, f)
    with open(tmp_path / "b.pkl", "wb") as f:
        pickle.dump({"Vehicle": [info("Vehicle", 6, 10, 4, 1)]}, f)
    np.save(tmp_path / "g.npy", pts)
    db = ip.GtDatabase.from_reference_files([tmp_path / "a.pkl", tmp_path / "b.pkl"], tmp_path / "g.npy")
    assert db.names.tolist() == ["Vehicle", "Vehicle", "Vehicle", "Pedestrian"]          # a second file extends the class's list
    assert db.offsets.tolist() == [[0, 3], [3, 4], [6, 10], [4, 6]] and db.boxes.dtype == np.float32 and db.boxes[2, 0] == 6.0
    assert db.class_index["Vehicle"].tolist() == [0, 1, 2] and db.class_index["Pedestrian"].tolist() == [3]
    p = db.prepare({"filter_by_min_points": ["Vehicle:2", "Pedestrian:0"], "filter_by_difficulty": [-1]})
    assert p.offsets.tolist() == [[0, 3], [6, 10]] and p.names.tolist() == ["Vehicle", "Vehicle"] and p.points is db.points
    assert db.prepare({"filter_by_min_points": ["Pedestrian:3"]}).names.tolist() == ["Vehicle"] * 3
    with pytest.raises(NotImplementedError, match="PREPARE"):
        db.prepare({"filter_by_road": 1})
    with open(tmp_path / "c.pkl", "wb") as f:
        pickle.dump({"Vehicle": [{"name": "Vehicle", "box3d_lidar": np.zeros(7), "path": "x.bin"}]}, f)
    with pytest.raises(NotImplementedError, match="global offsets"):
        ip.GtDatabase.from_reference_files(tmp_path / "c.pkl", tmp_path / "g.npy")


def _db():
    return ip.GtDatabase(np.zeros((4, 5), np.float32), [[0, 2], [2, 4]], np.zeros((2, 7)), ["Vehicle", "Pedestrian"], [2, 2], [0, 0])


@pytest.mark.parametrize("key,val,msg", [("USE_ROAD_PLANE", True, "USE_ROAD_PLANE"), ("DATABASE_WITH_FAKELIDAR", True, "DATABASE_WITH_FAKELIDAR"),
                                         ("FADE_EPOCH", 5, "FADE_EPOCH")])
def test_sampler_options_refused_by_name(key, val, msg):
    cfg = dict(sc.SAMPLER_CFG, **{key: val})
    with pytest.raises(NotImplementedError, match=msg):
        ip.GpuFinetuneInputPipeline(sc.PC_RANGE, sc.CLASS_NAMES, [cfg] + sc.WORLD_CFG, _db(), device=CPU)
    with pytest.raises(NotImplementedError, match=msg):                                 # also without a database: the config is refused
        ip.GpuFinetuneInputPipeline(sc.PC_RANGE, sc.CLASS_NAMES, [cfg] + sc.WORLD_CFG, None, device=CPU)


def test_other_refusals_by_name():
    for name in ("random_world_translation", "random_world_drop", "random_local_rotation"):
        with pytest.raises(NotImplementedError, match=name):
            ip.GpuFinetuneInputPipeline(sc.PC_RANGE, sc.CLASS_NAMES, sc.AUG_CFG + [{"NAME": name, "PROBABILITY": 1.0}], _db(), device=CPU)
    with pytest.raises(NotImplementedError, match="global offsets"):
        ip.GtDatabase(np.zeros((4, 5), np.float32), None, np.zeros((2, 7)), ["Vehicle", "Pedestrian"])
    with pytest.raises(NotImplementedError, match="7 columns"):
        ip.GtDatabase(np.zeros((4, 5), np.float32), [[0, 2], [2, 4]], np.zeros((2, 9)), ["Vehicle", "Pedestrian"])
    pipe = ip.GpuFinetuneInputPipeline(sc.PC_RANGE, sc.CLASS_NAMES, sc.AUG_CFG, _db(), device=CPU)       # accepted: BACKEND, USE_SHARED_MEMORY
    ip.GpuFinetuneInputPipeline(sc.PC_RANGE, sc.CLASS_NAMES, [dict(sc.SAMPLER_CFG, USE_SHARED_MEMORY=True, BACKEND={"NAME": "HardDiskBackend"})], _db(), device=CPU)
    with pytest.raises(NotImplementedError, match="7 columns"):
        pipe([np.zeros((1, 5), np.float32)], [np.zeros((1, 9), np.float32)], [["Vehicle"]])


@pytest.mark.parametrize("n_gt,n_cand,msg", [(0, 65, "more than 64 candidates"), (449, 0, "more than 448 existing boxes")])
def test_limits_are_a_clean_error_return_of_the_library(n_gt, n_cand, msg):
    """The frame table is checked on the host before anything is launched: no device pointer is touched."""
    desc = np.array([[0, 3, 2, 0], [5, n_gt, n_cand, 2]], np.int32)
    z3 = L.host_f32([0, 0, 0])
    rc = L.load().gdmae_gt_sample_select(None, desc.ctypes.data, None, None, 2, 2, None, L.host_f32([0] * 6), z3, 1, 8, None, None, None, None, None, None)
    assert rc != 0 and msg in L.load().gdmae_last_error().decode()
    with pytest.raises(L.GdmaeHipError, match=msg):
        L.call("gdmae_gt_sample_select", None, desc.ctypes.data, None, None, 2, 2, None, L.host_f32([0] * 6), z3, 1, 8, None, None, None, None, None, None)


def test_finetune_data_cfg_equals_the_yaml():
    if not os.path.exists(REF_YAML):
        pytest.skip("the reference's waymo_models/gd_mae.yaml is not on this machine")
    import yaml
    with open(REF_YAML) as f:
        y = yaml.safe_load(f)["DATA_CONFIG"]
    aug, proc = configs.waymo_finetune_data_cfg()
    assert aug == y["DATA_AUGMENTOR"]["AUG_CONFIG_LIST"] and proc == y["DATA_PROCESSOR"]
    assert aug == list(ip.FINETUNE_AUG_CONFIG) and aug[1:] == list(ip.SSL_AUG_CONFIG)


def test_crafted_scene_conditions():
    """What the GPU test relies on, checked on the statement alone: the scene holds every case it names, every pair decision has
    1e-2 m^2 of overlap or 1e-2 m of gap, every point / corner decision is 1e-3 m from its boundary."""
    s = sc.crafted()
    st = sc.statement(s, perms=None)
    m = st["margins"]
    assert m["pair"] >= 1e-2 and m["inbox"] >= 1e-3 and m["range"] >= 1e-3 and m["corner"] >= 1e-3, m
    assert st["valid"][0].tolist() == [False, False, True, True, True]
    assert st["valid"][1].tolist() == [False, False, False, True, True, True, True, True, False, True]
    assert st["valid"][2].tolist() == [True, True] and len(s["frames"][2]) == 0 and st["kept"][2] > 0
    assert len(st["valid"][3]) == 0 and st["num_gt"][3] == 12
    state = ip.sampler_state(sc.SAMPLER_CFG, {"Vehicle": 9, "Pedestrian": 9}, sc.CLASS_NAMES)
    assert ip.draw_candidates(state, s["gt_names"][3]) == []                        # frame 3 meets every quota by itself
    r = sc.PC_RANGE.astype(np.float64)
    tb = fr.transform_boxes(s["cands"][1]["boxes"], s["params"][1])
    inside = [int(((fr.corners(b) >= r[:3]) & (fr.corners(b) <= r[3:])).all(1).sum()) for b in tb]
    assert inside[5] == 1 and inside[6] == 0 and inside[4] == 4
    obj4 = s["cands"][1]["points"][4].copy()
    obj4[:, :3] += s["cands"][1]["boxes"][4][:3]
    k = fr.points_in_range(sc.io.augment_frame(obj4, **s["params"][1]), sc.PC_RANGE, {"range": np.inf})
    assert 0 < k.sum() < len(k)                                                     # object points on both sides of the range
    assert st["num_gt"][1] == 2 + 6 - 1                                             # 2 GT of the classes + 6 valid, one of them out of range
