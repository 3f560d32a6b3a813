"""random_world_translation and random_world_drop in the fine-tune input pipeline ("translation and drop"), GPU half:
gdmae_gt_sample_select_aug / _drop_plan / _collate_aug called directly into sentinel-filled buffers (every case twice, bit-equal), and
input_pipeline.finetune_input_pipeline, against the numpy statement tests/finetune_input_aug_reference.py."""
import numpy as np
import pytest
import torch

import finetune_input_aug_reference as far
import finetune_input_aug_scenes as asc
import finetune_input_scenes as sc
from gdmae_hip import configs, input_pipeline as ip, lib as L

pytestmark = pytest.mark.gpu

COORD_TOL = 2e-5          # the project's bound for the rotation's arithmetic (tests/test_finetune_input_gpu.py)
SENTINEL = -7777.0
INT_MAX = 0x7FFFFFFF
BIG_RANGE = np.array([-1e4, -1e4, -1e4, 1e4, 1e4, 1e4], np.float32)


# ---- the C entry points on frames without candidates ------------------------------------------------------------------------------
def _direct_once(frames, pc_range, params=None, translate=None, q=None, seeds=None, keys=None, gt=None, min_corners=1, plan_with_q1=False):
    """frames: B arrays (n, F); gt: None or B arrays (m, 7) of boxes (class 1); translate: None or (B, 3) float64; q: None (no plan) or
    (B) float64; keys: None or B uint32 arrays.  -> dict of host arrays; every output buffer starts filled with a sentinel."""
    dev = torch.device("cuda")
    B, F = len(frames), frames[0].shape[1]
    params = params or [asc.IDENT] * B
    gt = gt if gt is not None else [np.zeros((0, 7), np.float32)] * B
    rows = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
    n_rows = int(rows[-1])
    seg = [(rows[b], rows[b], 0, b, -1, -1, 1, rows[b]) for b in range(B) if len(frames[b])]
    boxes_h = np.concatenate([np.concatenate([np.asarray(g, np.float32).reshape(-1, 7), np.ones((len(g), 1), np.float32)], 1) for g in gt])
    first = np.concatenate([[0], np.cumsum([len(g) for g in gt])])
    desc_h = np.array([[first[b], len(gt[b]), 0, 0] for b in range(B)], np.int32)
    cap = max(max(len(g) for g in gt), 1)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)      # noqa: E731
    raw = t(np.concatenate(frames) if n_rows else np.zeros((1, F)), np.float32)
    seg_d, boxes_d, desc_d = t(np.asarray(seg).reshape(-1, 8), np.int32), t(boxes_h if len(boxes_h) else np.zeros((1, 8)), np.float32), t(desc_h, np.int32)
    tab_d = t(ip.finetune_params_table(params), np.float32)
    tr_d = t(translate, np.float64) if translate is not None else None
    q_d = t(q, np.float64) if q is not None else None
    seeds_d = t(np.asarray(seeds if seeds is not None else np.zeros(B), np.uint64).view(np.int64), np.int64)
    keys_d = t(np.concatenate(keys).view(np.int32), np.int32) if keys is not None and n_rows else None
    i32 = lambda n, v: torch.full((n,), v, dtype=torch.int32, device=dev)                # noqa: E731
    valid, n_valid, num_gt, kept, plan = i32(1, -5), i32(B, -5), i32(B, -5), i32(B + 1, -5), i32(8 * B, -5)
    rm = torch.full((B, ip.MAX_CANDIDATES, 8), SENTINEL, device=dev)
    gt_out = torch.full((B, cap, 8), SENTINEL, device=dev)
    out = torch.full((max(n_rows, 1) + 3, 1 + F), SENTINEL, device=dev)
    lib = L.load()
    ws = torch.empty(lib.gdmae_gt_sample_workspace_bytes(n_rows), dtype=torch.uint8, device=dev)
    dws = torch.empty(lib.gdmae_gt_sample_drop_workspace_bytes(n_rows, B), dtype=torch.uint8, device=dev)
    r6, xy = [float(v) for v in pc_range], [float(pc_range[i]) for i in (0, 1, 3, 4)]
    L.call("gdmae_gt_sample_select_aug", L.ptr(boxes_d), desc_h.ctypes.data, L.ptr(desc_d), None, B, 0, L.ptr(tab_d), L.ptr(tr_d), L.host_f32(r6),
           L.host_f32([0, 0, 0]), min_corners, cap, L.ptr(valid), L.ptr(rm), L.ptr(n_valid), L.ptr(gt_out), L.ptr(num_gt), L.stream())
    use_plan = q is not None and (plan_with_q1 or bool((np.asarray(q) != 1.0).any()))
    if use_plan:
        L.call("gdmae_gt_sample_drop_plan", L.ptr(raw), L.ptr(raw), F, L.ptr(seg_d), len(seg), n_rows, B, L.ptr(boxes_d), L.ptr(valid), L.ptr(rm),
               L.ptr(n_valid), L.ptr(seeds_d), L.ptr(q_d), L.ptr(keys_d), L.ptr(plan), L.ptr(dws), L.stream())
    L.call("gdmae_gt_sample_collate_aug", L.ptr(raw), L.ptr(raw), F, L.ptr(seg_d), len(seg), n_rows, B, L.ptr(tab_d), L.ptr(tr_d), L.ptr(boxes_d),
           L.ptr(valid), L.ptr(rm), L.ptr(n_valid), L.ptr(seeds_d), L.ptr(keys_d), L.ptr(plan) if use_plan else None,
           L.ptr(dws) if use_plan else None, L.host_f32(xy), L.ptr(out), L.ptr(kept), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    return {"out": out.cpu().numpy(), "kept": kept.cpu().numpy(), "plan": plan.cpu().numpy().reshape(B, 8), "gt": gt_out.cpu().numpy(),
            "num_gt": num_gt.cpu().numpy(), "n_valid": n_valid.cpu().numpy(), "used_plan": use_plan}


def _direct(frames, pc_range, **kw):
    """Twice, bit-equal; the rows behind the kept ones still hold the sentinel."""
    a, b = _direct_once(frames, pc_range, **kw), _direct_once(frames, pc_range, **kw)
    for k in ("out", "kept", "plan", "gt", "num_gt", "n_valid"):
        assert a[k].tobytes() == b[k].tobytes(), k
    n = int(a["kept"][-1])
    assert 0 <= n <= sum(len(f) for f in frames) and (a["out"][n:] == SENTINEL).all()
    assert (a["n_valid"] == 0).all()
    return a


def _frame_rows(res, B):
    """-> per frame its output rows (without the batch column)."""
    k = res["kept"].astype(np.int64).copy()
    for b in range(B - 1, -1, -1):
        if k[b] < 0:
            k[b] = k[b + 1]
    assert (np.diff(k) >= 0).all()
    for b in range(B):
        assert (res["out"][k[b]:k[b + 1], 0] == b).all()
    return [res["out"][k[b]:k[b + 1], 1:] for b in range(B)]


def _plan_of(keys, k):
    """[T, admitted ties, J, ties] of all-eligible rows with these keys."""
    if k == 0:
        return [0, 0, -1, 0]
    keys = np.asarray(keys, np.uint32)
    T = np.sort(keys, kind="stable")[k - 1]
    ties, adm = int((keys == T).sum()), k - int((keys < T).sum())
    J = INT_MAX if adm == ties else int(np.flatnonzero(keys == T)[adm - 1])
    return [int(np.array(T, np.uint32).view(np.int32)), adm, J, ties]


# ---- translation ------------------------------------------------------------------------------------------------------------------
def test_translation_is_numpys_float32_plus_float64():
    """Rotation by 0 keeps the statement's pre-translation values exact, so points and boxes are compared bit for bit; a second run
    with a real rotation compares against the translation of the device's own untranslated rows."""
    pts, boxes, names = asc.translation_scene()
    t = asc.T_ISSUE
    pr = [{"flip_x": False, "flip_y": True, "angle": 0.0, "scale": 1.03, "translate": t}]
    pipe = ip.finetune_input_pipeline(asc.WAYMO_RANGE, sc.CLASS_NAMES, list(sc.WORLD_CFG) + [asc.TRANSLATE_CFG], None, shuffle=False)
    out = pipe([pts], [boxes], [names], params=pr)
    st = far.pipeline([pts], [boxes], [names], sc.CLASS_NAMES, asc.WAYMO_RANGE, pr)
    got = out["points"].cpu().numpy()
    assert 0 < len(got) < len(pts) and got.tobytes() == st["points"].tobytes()
    assert out["num_gt"] == st["num_gt"] and out["gt_boxes"].cpu().numpy().tobytes() == st["gt_boxes"].tobytes()
    assert out["drop_n"] is None and out["drop_k"] is None
    plain = pts[:, :3] * np.float32(1.03) * np.array([-1, 1, 1], np.float32) + t.astype(np.float32)      # what v + (float)t would give
    assert (plain[np.isin(np.arange(len(pts)), got[:, -1].astype(int))] != got[:, 1:4]).mean() >= 1e-3

    pr = [{"flip_x": True, "flip_y": False, "angle": 0.4, "scale": 0.97}]
    gt = [boxes]
    base = _direct([pts], BIG_RANGE, params=pr, gt=gt)
    moved = _direct([pts], BIG_RANGE, params=pr, gt=gt, translate=t.reshape(1, 3))
    assert base["kept"][-1] == len(pts) == moved["kept"][-1] and base["num_gt"][0] == len(boxes) == moved["num_gt"][0]
    assert far.translate(base["out"][:len(pts), 1:], t).tobytes() == moved["out"][:len(pts), 1:].tobytes()
    assert far.translate(base["gt"][0], t).tobytes() == moved["gt"][0].tobytes()


def test_translation_moves_points_and_boxes_across_the_range():
    r = asc.WAYMO_RANGE
    pts = np.array([[74.8, 0, 0, 0], [-74.9, 1, 0, 1], [10, 74.7, 0, 2], [10, -74.7, 0, 3], [0, 0, 0, 4]], np.float32)
    t = np.array([[0.212, -0.312, 0.051]])
    # boxes of 2 x 2 x 1 m, heading 0: the corners sit at cx +- 1
    gt = np.array([[75.7, 0, 0, 2, 2, 1, 0], [-76.0, 0, 0, 2, 2, 1, 0], [0, 0, 0, 2, 2, 1, 0], [0, 90, 0, 2, 2, 1, 0]], np.float32)
    a = _direct([pts], r, gt=[gt])
    b = _direct([pts], r, gt=[gt], translate=t)
    assert _frame_rows(a, 1)[0][:, -1].tolist() == [0, 2, 3, 4]                    # -74.9 is outside
    assert _frame_rows(b, 1)[0][:, -1].tolist() == [1, 2, 4]                       # 74.8 + 0.212 and -74.7 - 0.312 left, -74.9 + 0.212 came in
    assert a["num_gt"][0] == 2 and np.array_equal(a["gt"][0, :2, 0], gt[[0, 2], 0]) and not a["gt"][0, 2:].any()
    assert b["num_gt"][0] == 2 and np.array_equal(b["gt"][0, :2, 0], far.translate(gt[[1, 2]], t[0])[:, 0])      # 4 -> 0 and 0 -> 4 corners
    st = far.pipeline([pts], [gt], [["Vehicle"] * 4], ["Vehicle"], r, [dict(asc.IDENT, translate=t[0])])
    assert st["points"][:, 1:].tobytes() == _frame_rows(b, 1)[0].tobytes() and st["gt_boxes"][0].tobytes() == b["gt"][0, :2].tobytes()
    # min_num_corners = 5: the box that came in has 4 corners inside, the one in the middle all 8
    c = _direct([pts], r, gt=[gt], translate=t, min_corners=5)
    assert c["num_gt"][0] == 1 and c["gt"][0, 0, 0] == np.float32(np.float64(np.float32(0)) + 0.212)


def test_zero_translation_turns_negative_zero_into_positive_zero():
    pts = np.array([[-0.0, 2.0, -1.0, 0], [3.0, 1.0, -0.0, 1]], np.float32)          # x' = x * 1 + y * -0 keeps -0 for y > 0
    gt = np.array([[-0.0, 2.0, -0.0, 2, 2, 1, 0]], np.float32)
    a = _direct([pts], asc.WAYMO_RANGE, gt=[gt])
    b = _direct([pts], asc.WAYMO_RANGE, gt=[gt], translate=np.zeros((1, 3)))
    assert np.signbit(a["out"][0, 1]) and np.signbit(a["out"][1, 3]) and np.signbit(a["gt"][0, 0, 0]) and np.signbit(a["gt"][0, 0, 2])
    for v in (b["out"][:2, 1:4], b["gt"][0, 0, :3]):
        assert (v == 0).sum() >= 2 and not np.signbit(v[v == 0]).any()
    assert np.array_equal(a["out"][:2], b["out"][:2]) and np.array_equal(a["gt"], b["gt"])      # equal as numbers


@pytest.mark.parametrize("scene", ["crafted", "tile"])
def test_without_translation_and_drop_the_new_entry_points_equal_the_old(scene):
    s = sc.crafted() if scene == "crafted" else sc.seams("tile")
    db = lambda: ip.GtDatabase(s["db"]["points"], s["db"]["offsets"], s["db"]["boxes"], s["db"]["names"])      # noqa: E731
    run = lambda p: p(s["frames"], s["gt_boxes"], s["gt_names"], params=s["params"], candidates=s["candidates"])      # noqa: E731
    old = run(ip.GpuFinetuneInputPipeline(sc.PC_RANGE, sc.CLASS_NAMES, sc.AUG_CFG, db(), shuffle=False))
    new = run(ip.GpuFinetuneAugInputPipeline(sc.PC_RANGE, sc.CLASS_NAMES, sc.AUG_CFG, db(), shuffle=False))
    assert len(old["points"]) > 0 and old["points"].cpu().numpy().tobytes() == new["points"].cpu().numpy().tobytes()
    assert old["gt_boxes"].cpu().numpy().tobytes() == new["gt_boxes"].cpu().numpy().tobytes() and old["num_gt"] == new["num_gt"]
    assert [v.tolist() for v in old["sampled_valid"]] == [v.tolist() for v in new["sampled_valid"]]


# ---- k and the kept set -----------------------------------------------------------------------------------------------------------
RATIOS = [0.1, 0.3, 0.71, 1.0, 0.0]


@pytest.mark.parametrize("n", [0, 1, 7, 10, 255, 256, 257, 2047, 2048, 2049, 4097, 65537, 180001])
def test_k_and_the_hashed_kept_set(n):
    """One frame per ratio, n eligible rows each: k is Python's int((1 - r) * n) and the kept rows are the statement's."""
    B = len(RATIOS)
    frames = [asc.indexed_frame(n, 100 + b) for b in range(B)]
    q = np.array([1 - r for r in RATIOS], np.float64)
    seeds = np.array([0x9E3779B97F4A7C15 * (b + 1) % 2 ** 64 + n for b in range(B)], np.uint64)
    res = _direct(frames, sc.PC_RANGE, q=q, seeds=seeds)
    want_k = [int((1 - r) * n) for r in RATIOS]
    if n == 7:
        assert want_k[0] == 6
    if n == 180001:
        assert want_k[0] == 162000
    if n == 0:
        assert not res["kept"].any() and not res["plan"][:, :2].any()
        return
    assert res["plan"][:, 0].tolist() == [n] * B and res["plan"][:, 1].tolist() == want_k
    assert want_k[3] == 0 and want_k[4] == n
    got = _frame_rows(res, B)
    for b in range(B):
        keys = far.hashed_keys(int(seeds[b]), n)
        want = far.kept_rows(keys, np.ones(n, bool), want_k[b])
        assert np.array_equal(got[b][:, -1].astype(np.int64), want), (n, b)
        assert got[b].tobytes() == frames[b][want].tobytes()
        assert res["plan"][b, 2:6].tolist() == _plan_of(keys, want_k[b])
    assert res["kept"][3] == res["kept"][4]                                       # r = 1.0 empties the frame


def test_explicit_keys_and_ties():
    n = 700
    g = np.random.default_rng(8)
    two = np.full(n, 7, np.uint32)
    two[200:330] = 3                                                              # a run of 130 ties across row 256
    edge = g.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    edge[g.permutation(n)[:60]] = 0
    edge[g.permutation(n)[:60]] = 0xFFFFFFFF
    cases = [("all equal", np.full(n, 5, np.uint32), 0.5), ("all equal, all kept", np.full(n, 0xFFFFFFFF, np.uint32), 1.0),
             ("descending", (2 ** 32 - 1 - 3 * np.arange(n)).astype(np.uint32), 0.3), ("threshold inside the run", two, 60 / n + 1e-9),
             ("threshold behind the run", two, 180 / n + 1e-9), ("0 and 0xFFFFFFFF, low", edge, 0.05), ("0 and 0xFFFFFFFF, high", edge, 0.97),
             ("0 and 0xFFFFFFFF, all but one", edge, (n - 1) / n + 1e-9), ("all zero", np.zeros(n, np.uint32), 0.5)]
    frames = [asc.indexed_frame(n, 40 + b) for b in range(len(cases))]
    res = _direct(frames, sc.PC_RANGE, q=np.array([c[2] for c in cases]), keys=[c[1] for c in cases])
    got = _frame_rows(res, len(cases))
    for b, (name, keys, q) in enumerate(cases):
        k = int(q * n)
        assert res["plan"][b, :2].tolist() == [n, k], name
        assert np.array_equal(got[b][:, -1].astype(np.int64), far.kept_rows(keys, np.ones(n, bool), k)), name
        assert res["plan"][b, 2:6].tolist() == _plan_of(keys, k), name
    assert got[0][:, -1].tolist() == list(range(350))                             # all equal: the first k rows
    assert got[2][:, -1].tolist() == list(range(n - int(0.3 * n), n))                      # descending: the last k rows
    assert got[3][:, -1].tolist() == list(range(200, 260))                        # ties admitted in row order, across row 256
    assert got[4][:, -1].tolist() == list(range(0, 50)) + list(range(200, 330))
    assert len(got[7]) == n - 1 and res["plan"][7, 2] == -1                        # T = 0xFFFFFFFF


def test_q_one_everywhere_equals_the_call_without_a_plan():
    frames = [asc.indexed_frame(n, 60 + n, extent=45.0) for n in (5000, 0, 300)]   # extent 45 m: the range mask drops rows
    a = _direct(frames, sc.PC_RANGE)
    b = _direct(frames, sc.PC_RANGE, q=np.ones(3), seeds=np.array([1, 2, 3], np.uint64), plan_with_q1=True)
    assert b["used_plan"] and not a["used_plan"] and 0 < a["kept"][-1] < 5300
    assert a["out"].tobytes() == b["out"].tobytes() and a["kept"].tobytes() == b["kept"].tobytes()
    assert b["plan"][:, 0].tolist() == [5000, 0, 300] and b["plan"][:, 1].tolist() == [5000, 0, 300] and b["kept"][1] == -1


# ---- interplay, through the factory -------------------------------------------------------------------------------------------------
def _factory(s, tail, **kw):
    d = s["db"]
    return ip.finetune_input_pipeline(sc.PC_RANGE, sc.CLASS_NAMES, sc.AUG_CFG + tail, ip.GtDatabase(d["points"], d["offsets"], d["boxes"], d["names"]),
                                      shuffle=False, **kw)


def _statement(s, **kw):
    return far.pipeline(s["frames"], s["gt_boxes"], s["gt_names"], sc.CLASS_NAMES, sc.PC_RANGE, s["params"], cands=s["cands"], n_groups=len(sc.GROUPS),
                        extra_width=sc.SAMPLER_CFG["REMOVE_EXTRA_WIDTH"], **kw)


def _compare(out, st):
    gp, ep = out["points"].cpu().numpy(), st["points"]
    assert [v.tolist() for v in out["sampled_valid"]] == [v.tolist() for v in st["valid"]] and out["num_gt"] == st["num_gt"]
    assert out["drop_n"] == st["drop_n"] and out["drop_k"] == st["drop_k"]
    assert gp.shape == ep.shape and np.array_equal(gp[:, 0], ep[:, 0]) and np.array_equal(gp[:, 4:], ep[:, 4:])      # the same rows in the same order
    gb, eb = out["gt_boxes"].cpu().numpy(), st["gt_boxes"]
    assert gb.shape == eb.shape and np.array_equal(gb[:, :, 7], eb[:, :, 7])
    print("max deviation: points", np.abs(gp - ep).max(initial=0), "boxes", np.abs(gb - eb).max(initial=0))
    assert np.abs(gp - ep).max(initial=0) <= COORD_TOL and np.abs(gb[:, :, :6] - eb[:, :, :6]).max(initial=0) <= COORD_TOL
    assert np.array_equal(gb[:, :, 6], eb[:, :, 6])                              # headings: bit-equal, as §7l measured


@pytest.mark.parametrize("keys", ["hashed", "all equal"])
def test_sampling_translation_and_drop_together(keys):
    """Invalid candidates and removed scene points are not eligible; the range mask comes after the drop; frame 1 does not drop; with
    equal keys the first k ELIGIBLE rows of every frame stay."""
    s = asc.crafted_with_drop()
    rows = [sum(len(p) for p in (c["points"] if c else [])) + len(f) for c, f in zip(s["cands"], s["frames"])]
    dk = [np.full(n, 11, np.uint32) for n in rows] if keys == "all equal" else None
    st = _statement(s, drop_keys=dk)
    m = st["margins"]
    assert m["pair"] >= 1e-2 and m["inbox"] >= 1e-3 and m["range"] >= 1e-3 and m["corner"] >= 1e-3, m
    assert st["drop_n"][0] < rows[0] and st["drop_n"][1] < rows[1] and st["drop_k"][1] == st["drop_n"][1]
    assert all(k <= d for k, d in zip(st["kept"], st["drop_k"])) and any(k < d for k, d in zip(st["kept"], st["drop_k"]))
    pipe = _factory(s, [asc.TRANSLATE_CFG, asc.DROP_CFG])
    run = lambda: pipe(s["frames"], s["gt_boxes"], s["gt_names"], params=s["params"], candidates=s["candidates"], drop_keys=dk)      # noqa: E731
    out, again = run(), run()
    _compare(out, st)
    assert out["points"].cpu().numpy().tobytes() == again["points"].cpu().numpy().tobytes() and out["drop_k"] == again["drop_k"]
    # the same through the staged (non-resident) database
    _compare(_factory(s, [asc.TRANSLATE_CFG, asc.DROP_CFG], resident=False)(s["frames"], s["gt_boxes"], s["gt_names"], params=s["params"],
                                                                             candidates=s["candidates"], drop_keys=dk), st)


def test_an_empty_frame_between_dropping_frames():
    s = sc.seams("small")                                                        # frame 1 has no rows at all
    s["params"] = [dict(p, drop_q=q, drop_seed=5 + b) for b, (p, q) in enumerate(zip(s["params"], (0.9, 0.9, 1 - 0.71)))]
    st = _statement(s, translation=False)
    assert st["drop_n"][1] == 0 and st["drop_k"][1] == 0 and st["kept"][1] == 0 and st["drop_k"][2] < st["drop_n"][2]
    _compare(_factory(s, [asc.DROP_CFG])(s["frames"], s["gt_boxes"], s["gt_names"], params=s["params"], candidates=s["candidates"]), st)


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["iou", "ts"])
def test_factory_with_the_shipped_configs_matches_the_statement(which):
    """The shipped list (the crafted scene's sampler entry in place of the yaml's: its database has two classes and its margins were
    built for its REMOVE_EXTRA_WIDTH), explicit decisions, a permutation of every frame's kept rows."""
    aug = (configs.waymo_iou_finetune_data_cfg if which == "iou" else configs.waymo_two_stage_data_cfg)()[0]
    assert [c["NAME"] for c in aug][-1] == "random_world_drop" and ("random_world_translation" in [c["NAME"] for c in aug]) == (which == "ts")
    s = asc.crafted_with_drop()
    if which == "iou":
        s["params"] = [{k: v for k, v in p.items() if k != "translate"} for p in s["params"]]
    d = s["db"]
    pipe = ip.finetune_input_pipeline(sc.PC_RANGE, sc.CLASS_NAMES, [sc.SAMPLER_CFG] + aug[1:], ip.GtDatabase(d["points"], d["offsets"], d["boxes"], d["names"]))
    assert type(pipe) is ip.GpuFinetuneAugInputPipeline
    st = _statement(s, translation=which == "ts")
    g = np.random.default_rng(2)
    perms = [g.permutation(k) for k in st["kept"]]
    st = _statement(s, translation=which == "ts", perms=perms)
    _compare(pipe(s["frames"], s["gt_boxes"], s["gt_names"], params=s["params"], candidates=s["candidates"], perms=perms), st)
    # the yaml's own list builds too, and draws and shuffles reproducibly from the two seeds
    full = ip.finetune_input_pipeline(sc.PC_RANGE, sc.GROUPS, aug, ip.GtDatabase(d["points"], d["offsets"], d["boxes"], d["names"], np.full(len(d["names"]), 50),
                                                                                       np.zeros(len(d["names"]))))

    def run():
        np.random.seed(9)
        torch.manual_seed(9)
        full.state = ip.sampler_state(full.sampler_cfg, full.database, full.class_names)
        o = full(s["frames"], s["gt_boxes"], s["gt_names"])
        return o["points"].cpu().numpy(), o["gt_boxes"].cpu().numpy(), o["drop_n"], o["drop_k"]
    a, b = run(), run()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2:] == b[2:] and len(a[0]) > 0


def test_golden_end_to_end():
    """The reference's own flip / rotation / scaling / translation / drop / masks / collate on the gd_mae_ts list: the library keeps the
    rows the reference kept (keys = position in its recorded choice) and returns them in its order."""
    z, frames, boxes, names, params, keys = asc.load_golden()
    aug = configs.waymo_two_stage_data_cfg()[0][1:]
    pipe = ip.finetune_input_pipeline(z["pc_range"], z["class_names"].tolist(), aug, None, shuffle=False)
    rows = pipe(frames, boxes, names, params=params, drop_keys=keys)
    assert rows["drop_n"] == [len(f) for f in frames] and rows["drop_k"] == [len(z[f"choice{i}"]) for i in range(len(frames))]
    p = rows["points"].cpu().numpy()
    perms = asc.golden_perms(z, [p[p[:, 0] == b][:, -1] for b in range(len(frames))])
    out = pipe(frames, boxes, names, params=params, drop_keys=keys, perms=perms)
    got, exp = out["points"].cpu().numpy(), z["expected_points"]
    assert got.shape == exp.shape and np.array_equal(got[:, 0], exp[:, 0]) and np.array_equal(got[:, 4:], exp[:, 4:])
    assert np.abs(got - exp).max() <= COORD_TOL
    gb, eb = out["gt_boxes"].cpu().numpy(), z["expected_gt_boxes"]
    assert out["num_gt"] == z["num_gt"].tolist() and gb.shape == eb.shape and np.array_equal(gb[:, :, 7], eb[:, :, 7])
    assert np.abs(gb[:, :, :6] - eb[:, :, :6]).max() <= COORD_TOL and np.abs(gb[:, :, 6] - eb[:, :, 6]).max() <= 4 * float(z["err_heading"])


def test_refusals_and_value_errors_by_name():
    s = sc.crafted()
    with pytest.raises(NotImplementedError, match="random_local_rotation"):
        _factory(s, [asc.DROP_CFG, {"NAME": "random_local_rotation", "PROBABILITY": 1.0}])
    with pytest.raises(NotImplementedError, match="random_world_drop is out of order"):
        _factory(s, [asc.DROP_CFG, asc.TRANSLATE_CFG])
    with pytest.raises(ValueError, match="DROP_RATIO"):
        _factory(s, [dict(asc.DROP_CFG, DROP_RATIO=1.01)])
    with pytest.raises(ValueError, match="NOISE_TRANSLATE_STD"):
        _factory(s, [dict(asc.TRANSLATE_CFG, NOISE_TRANSLATE_STD=[0.1, 0.2])])
    with pytest.raises(NotImplementedError, match="random_world_drop"):
        ip.GpuFinetuneInputPipeline(sc.PC_RANGE, sc.CLASS_NAMES, sc.AUG_CFG + [asc.DROP_CFG], None)
    run = lambda p, pr: p(s["frames"], s["gt_boxes"], s["gt_names"], params=pr, candidates=s["candidates"])      # noqa: E731
    with pytest.raises(ValueError, match="random_world_translation is not in the augmentation list"):
        run(_factory(s, [asc.DROP_CFG]), [dict(p, translate=np.zeros(3)) for p in s["params"]])
    with pytest.raises(ValueError, match="random_world_drop is not in the augmentation list"):
        run(_factory(s, [asc.TRANSLATE_CFG]), [dict(p, drop_q=0.5) for p in s["params"]])
    torch.cuda.synchronize()


# ---- uniformity ---------------------------------------------------------------------------------------------------------------------
def test_device_kept_sets_are_the_statements_and_uniform():
    n, (lo, hi) = asc.UNIFORMITY_ROWS, asc.UNIFORMITY_BOUNDS
    frame = asc.indexed_frame(n, 1)
    cnt = np.zeros(n, np.int64)
    for c in range(0, 256, 64):
        seeds = np.array(asc.UNIFORMITY_SEEDS[c:c + 64], np.uint64)
        res = _direct_once([frame] * 64, sc.PC_RANGE, q=np.full(64, 0.5), seeds=seeds)
        for b, rows in enumerate(_frame_rows(res, 64)):
            got = rows[:, -1].astype(np.int64)
            assert np.array_equal(got, far.kept_rows(far.hashed_keys(int(seeds[b]), n), np.ones(n, bool), n // 2))
            cnt[got] += 1
    print("rows kept between", cnt.min(), "and", cnt.max(), "times of 256")
    assert cnt.sum() == 256 * (n // 2) and lo <= cnt.min() and cnt.max() <= hi
