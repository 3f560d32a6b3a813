"""random_world_translation and random_world_drop in the fine-tune input pipeline ("translation and drop"), CPU half: the
numpy statement (tests/finetune_input_aug_reference.py) against the reference's golden, the host draws against the reference's
recorded decisions, pinned key vectors, the factory's refusals, and the conditions the GPU tests rest on."""
import os

import numpy as np
import pytest
import torch

import finetune_input_aug_reference as far
import finetune_input_aug_scenes as asc
import finetune_input_scenes as sc
from gdmae_hip import configs, input_pipeline as ip

CPU = torch.device("cpu")
REF_CFGS = "/root/reference/tools/cfgs/waymo_models"


def test_statement_reproduces_the_reference_golden():
    z, frames, boxes, names, params, keys = asc.load_golden()
    assert z["dropped"].any() and not z["dropped"].all() and any(np.any(p["translate"] != 0) for p in params)
    for i, p in enumerate(params):
        # the translation on the reference's own arrays before it: bit for bit
        assert far.translate(z[f"pre_points{i}"], p["translate"]).tobytes() == z[f"post_points{i}"].tobytes()
        assert far.translate(z[f"pre_boxes{i}"], p["translate"]).tobytes() == z[f"post_boxes{i}"].tobytes()
        # restated: fp64 sum, one rounding
        assert np.array_equal((z[f"pre_points{i}"].astype(np.float64) + p["translate"]).astype(np.float32), z[f"post_points{i}"])
        choice = z[f"choice{i}"]
        n = len(frames[i])
        assert far.drop_count(p["drop_q"], n) == len(choice) and (len(choice) < n) == bool(z["dropped"][i])
        assert np.array_equal(far.kept_rows(keys[i], np.ones(n, bool), len(choice)), np.sort(choice))
    st = far.pipeline(frames, boxes, names, z["class_names"].tolist(), z["pc_range"], params, drop_keys=keys)
    assert st["drop_n"] == [len(f) for f in frames] and st["drop_k"] == [len(z[f"choice{i}"]) for i in range(len(frames))]
    off = np.concatenate([[0], np.cumsum(st["kept"])])
    perms = asc.golden_perms(z, [st["points"][off[b]:off[b + 1], -1] for b in range(len(frames))])
    st = far.pipeline(frames, boxes, names, z["class_names"].tolist(), z["pc_range"], params, drop_keys=keys, perms=perms)
    ep, eg = z["expected_points"], z["expected_gt_boxes"]
    assert st["points"].shape == ep.shape and st["gt_boxes"].shape == eg.shape and st["num_gt"] == z["num_gt"].tolist()
    assert np.array_equal(st["points"][:, 0], ep[:, 0]) and np.array_equal(st["points"][:, 4:], ep[:, 4:])       # frames, rows, order
    assert np.array_equal(st["gt_boxes"][:, :, 7], eg[:, :, 7])
    assert np.abs(st["points"] - ep).max() <= float(z["err_coord"])                # the rotation's BLAS against numpy rounding, as §7l
    assert np.abs(st["gt_boxes"][:, :, :6] - eg[:, :, :6]).max() <= float(z["err_coord"])
    assert np.abs(st["gt_boxes"][:, :, 6] - eg[:, :, 6]).max() <= float(z["err_heading"])


def test_host_draws_follow_the_reference_up_to_the_drops_enable_draw():
    z, frames, boxes, names, params, keys = asc.load_golden()
    aug, _ = configs.waymo_two_stage_data_cfg()
    pipe = ip.finetune_input_pipeline(z["pc_range"], z["class_names"].tolist(), aug[1:], None, device=CPU)
    assert type(pipe) is ip.GpuFinetuneAugInputPipeline
    for i, p in enumerate(params):
        np.random.seed(int(z["seed"]) + i)
        mine = pipe._draw_frame_params()
        assert {k: mine[k] for k in ("flip_x", "flip_y", "angle", "scale")} == {k: p[k] for k in ("flip_x", "flip_y", "angle", "scale")}
        assert mine["translate"].dtype == np.float64 and np.array_equal(mine["translate"], p["translate"])      # enable flag and the three normals
        assert mine["drop_q"] == p["drop_q"] and (mine["drop_q"] != 1.0) == bool(z["dropped"][i])
        assert 0 <= mine["drop_seed"] < 2 ** 64
    # a scalar NOISE_TRANSLATE_STD is accepted as in the reference; a disabled translation still draws its three normals
    np.random.seed(5)
    a = ip.draw_translation({"PROBABILITY": 1.0, "NOISE_TRANSLATE_STD": 0.25})
    np.random.seed(5)
    b = ip.draw_translation({"PROBABILITY": 1.0, "NOISE_TRANSLATE_STD": [0.25, 0.25, 0.25]})
    assert np.array_equal(a, b) and np.all(a != 0)
    np.random.seed(5)
    assert np.array_equal(ip.draw_translation({"PROBABILITY": 0.0, "NOISE_TRANSLATE_STD": 0.25}), np.zeros(3))
    after = np.random.random()
    np.random.seed(5)
    ip.draw_translation({"PROBABILITY": 1.0, "NOISE_TRANSLATE_STD": 0.25})
    assert np.random.random() == after


def test_pinned_key_vectors():
    """splitmix64's finaliser on seed + (j + 1) * 0x9E3779B97F4A7C15, upper 32 bits, computed with Python integers."""
    pinned = {0: [3793791033, 1853398634, 113532184, 4169906344], 1: [2433363436, 3203108257, 4170425070, 1908508304],
              0xDEADBEEFCAFEF00D: [2417839973, 2815304804, 431229883, 3886575045]}
    for seed, want in pinned.items():
        assert far.hashed_keys(seed, 4).tolist() == want
        assert ip.drop_keys_of(seed, 4).tolist() == want and ip.drop_keys_of(seed, 4).dtype == np.uint32
    assert np.array_equal(far.hashed_keys(123456789, 5000), ip.drop_keys_of(123456789, 5000))


def test_drop_count_is_pythons_truncated_fp64_product():
    assert far.drop_count(1 - 0.1, 7) == 6 and int(round((1 - 0.1) * 7)) == 6 and 7 - int(0.1 * 7) == 7          # truncation, not n - int(r n)
    assert far.drop_count(1 - 0.1, 180001) == 162000 and round((1 - 0.1) * 180001) == 162001                       # truncation, not rounding
    assert far.drop_count(1.0, 12345) == 12345 and far.drop_count(1 - 1.0, 12345) == 0


def test_kept_rows_ties_go_to_the_lower_row():
    el = np.array([1, 0, 1, 1, 0, 1, 1], bool)
    assert far.kept_rows(np.full(7, 9, np.uint32), el, 3).tolist() == [0, 2, 3]
    assert far.kept_rows(np.array([5, 0, 4, 3, 0, 2, 1], np.uint32), el, 2).tolist() == [5, 6]
    assert far.kept_rows(np.array([3, 3, 1, 3, 3, 1, 3], np.uint32), el, 3).tolist() == [0, 2, 5]
    assert far.kept_rows(np.arange(7, dtype=np.uint32), el, 0).tolist() == []


def test_translation_scene_separates_the_two_roundings():
    pts, boxes, _ = asc.translation_scene()
    v = pts[:, :3]
    a = (v.astype(np.float64) + asc.T_ISSUE).astype(np.float32)
    b = v + asc.T_ISSUE.astype(np.float32)
    frac = float((a != b).mean())
    print("coordinates where fp32 add and fp64 add then round differ:", frac)
    assert frac >= 1e-3
    assert np.array_equal(far.translate(pts, asc.T_ISSUE)[:, :3], a) and np.array_equal(far.translate(pts, asc.T_ISSUE)[:, 3:], pts[:, 3:])


def test_hashed_keys_are_uniform_enough():
    lo, hi = asc.UNIFORMITY_BOUNDS
    n = asc.UNIFORMITY_ROWS
    cnt = np.zeros(n, np.int64)
    for s in asc.UNIFORMITY_SEEDS:
        cnt[far.kept_rows(far.hashed_keys(s, n), np.ones(n, bool), far.drop_count(0.5, n))] += 1
    print("rows kept between", cnt.min(), "and", cnt.max(), "times of", len(asc.UNIFORMITY_SEEDS))
    assert cnt.sum() == 256 * 2048 and lo <= cnt.min() and cnt.max() <= hi


def test_crafted_drop_scene_conditions():
    s = asc.crafted_with_drop()
    st = far.pipeline(s["frames"], s["gt_boxes"], s["gt_names"], sc.CLASS_NAMES, sc.PC_RANGE, s["params"], cands=s["cands"], n_groups=len(sc.GROUPS),
                      extra_width=sc.SAMPLER_CFG["REMOVE_EXTRA_WIDTH"])
    m = st["margins"]
    assert m["pair"] >= 1e-2 and m["inbox"] >= 1e-3 and m["range"] >= 1e-3 and m["corner"] >= 1e-3, m
    rows = [sum(len(p) for p in (c["points"] if c else [])) + len(f) for c, f in zip(s["cands"], s["frames"])]
    assert st["drop_n"][0] < rows[0] and st["drop_n"][1] < rows[1]                  # invalid candidates and removed points are not eligible
    assert st["drop_k"] == [int(p["drop_q"] * n) for p, n in zip(s["params"], st["drop_n"])]
    assert st["drop_k"][1] == st["drop_n"][1] and st["drop_k"][0] < st["drop_n"][0]
    assert all(k <= d for k, d in zip(st["kept"], st["drop_k"])) and any(k < d for k, d in zip(st["kept"], st["drop_k"]))     # range mask after the drop
    # without translation and drop the statement is fr.pipeline
    base = sc.statement(sc.crafted())
    same = far.pipeline(s["frames"], s["gt_boxes"], s["gt_names"], sc.CLASS_NAMES, sc.PC_RANGE, sc.PARAMS4, cands=s["cands"], n_groups=len(sc.GROUPS),
                        extra_width=sc.SAMPLER_CFG["REMOVE_EXTRA_WIDTH"], translation=False)
    assert same["points"].tobytes() == base["points"].tobytes() and same["gt_boxes"].tobytes() == base["gt_boxes"].tobytes()


def _db():
    return ip.GtDatabase(np.zeros((4, 5), np.float32), [[0, 2], [2, 4]], np.zeros((2, 7)), ["Vehicle", "Pedestrian"], [2, 2], [0, 0])


def test_factory_classes_refusals_and_value_errors():
    mk = lambda aug: ip.finetune_input_pipeline(sc.PC_RANGE, sc.CLASS_NAMES, aug, _db(), device=CPU)      # noqa: E731
    assert type(mk(sc.AUG_CFG)) is ip.GpuFinetuneInputPipeline
    assert type(mk(list(ip.FINETUNE_AUG_CONFIG))) is ip.GpuFinetuneInputPipeline
    for tail in ([asc.TRANSLATE_CFG], [asc.DROP_CFG], [asc.TRANSLATE_CFG, asc.DROP_CFG]):
        p = mk(sc.AUG_CFG + tail)
        assert type(p) is ip.GpuFinetuneAugInputPipeline and isinstance(p, ip.GpuFinetuneInputPipeline)
        assert (p.translate_cfg is not None) == (asc.TRANSLATE_CFG in tail) and (p.drop_cfg is not None) == (asc.DROP_CFG in tail)
    for aug in (configs.waymo_iou_finetune_data_cfg()[0], configs.waymo_two_stage_data_cfg()[0]):
        assert type(ip.finetune_input_pipeline(asc.WAYMO_RANGE, sc.CLASS_NAMES, aug, None, device=CPU)) is ip.GpuFinetuneAugInputPipeline
    for name in ("random_local_rotation", "random_world_frustum_dropout"):
        with pytest.raises(NotImplementedError, match=name):
            mk(sc.AUG_CFG + [asc.DROP_CFG, {"NAME": name, "PROBABILITY": 1.0}][::-1])
        with pytest.raises(NotImplementedError, match=name):
            mk(sc.AUG_CFG + [asc.DROP_CFG, {"NAME": name, "PROBABILITY": 1.0}])
        with pytest.raises(NotImplementedError, match=name):
            mk(sc.AUG_CFG + [{"NAME": name, "PROBABILITY": 1.0}])
    with pytest.raises(NotImplementedError, match="random_world_drop is out of order"):
        mk(sc.AUG_CFG + [asc.DROP_CFG, asc.TRANSLATE_CFG])
    with pytest.raises(NotImplementedError, match="random_world_translation is out of order"):
        mk([sc.SAMPLER_CFG, asc.TRANSLATE_CFG] + sc.WORLD_CFG)
    with pytest.raises(NotImplementedError, match="random_world_drop is out of order"):
        mk([sc.SAMPLER_CFG, sc.WORLD_CFG[0], asc.DROP_CFG] + sc.WORLD_CFG[1:])
    with pytest.raises(NotImplementedError, match="random_world_drop appears twice"):
        mk(sc.AUG_CFG + [asc.DROP_CFG, asc.DROP_CFG])
    for r in (-0.01, 1.5):
        with pytest.raises(ValueError, match="DROP_RATIO"):
            mk(sc.AUG_CFG + [dict(asc.DROP_CFG, DROP_RATIO=r)])
    mk(sc.AUG_CFG + [dict(asc.DROP_CFG, DROP_RATIO=0.0)])
    mk(sc.AUG_CFG + [dict(asc.DROP_CFG, DROP_RATIO=1.0)])
    for std in ([0.2, 0.2], [0.1] * 4, []):
        with pytest.raises(ValueError, match="NOISE_TRANSLATE_STD"):
            mk(sc.AUG_CFG + [dict(asc.TRANSLATE_CFG, NOISE_TRANSLATE_STD=std)])
    mk(sc.AUG_CFG + [dict(asc.TRANSLATE_CFG, NOISE_TRANSLATE_STD=0.2)])
    # the existing class keeps refusing both names (tests/test_finetune_input_cpu.py pins that too)
    for cfg in (asc.TRANSLATE_CFG, asc.DROP_CFG):
        with pytest.raises(NotImplementedError, match=cfg["NAME"]):
            ip.GpuFinetuneInputPipeline(sc.PC_RANGE, sc.CLASS_NAMES, sc.AUG_CFG + [cfg], _db(), device=CPU)


@pytest.mark.parametrize("yaml_name,fn", [("gd_mae_iou.yaml", "waymo_iou_finetune_data_cfg"), ("gd_mae_ts.yaml", "waymo_two_stage_data_cfg")])
def test_new_data_cfgs_equal_the_yaml(yaml_name, fn):
    path = os.path.join(REF_CFGS, yaml_name)
    if not os.path.exists(path):
        pytest.skip(f"the reference's waymo_models/{yaml_name} is not on this machine")
    import yaml
    with open(path) as f:
        y = yaml.safe_load(f)["DATA_CONFIG"]
    aug, proc = getattr(configs, fn)()
    assert aug == y["DATA_AUGMENTOR"]["AUG_CONFIG_LIST"] and proc == y["DATA_PROCESSOR"]
    assert configs.waymo_finetune_data_cfg()[0] == list(ip.FINETUNE_AUG_CONFIG)          # building them left the first config alone
