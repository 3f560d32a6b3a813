"""CPU: the plain reference of the geometry plan (tests/plan_reference.py) against the goldens captured from the unmodified
reference project, its self-consistency on every crafted scene (tests/plan_scenes.py), and the host-only refusal of a stage
token capacity that does not fit the packed window scan.  Everything is integer: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import plan_scenes as PS
from helpers import load_case
from plan_reference import reference_plan


@pytest.mark.parametrize("name", ["kitti_b2", "kitti_b2_m75", "waymo_b1"])
def test_reference_plan_reproduces_the_goldens(name):
    z, ds, cfg, _ = load_case(name)
    from pcdet.models.backbones_3d.spt_backbone import stage_plan_args
    B = int(z["batch_size"])
    ref = reference_plan(z["points"], ds.point_cloud_range, ds.voxel_size, ds.grid_size, B,
                         *stage_plan_args(cfg.BACKBONE_3D.SST_BLOCK_LIST), keep_frac=1 - float(z["mask_ratio"]), noise=z["noise"],
                         dec_sources=PS.DEC_SOURCES)
    assert ref["N"] == int(z["keep_count"])
    assert np.array_equal(ref["voxel_coords"], z["voxel_coords"])
    assert np.array_equal(ref["mask"].astype(np.uint8), z["mask"])
    assert np.array_equal(ref["tok_pillar"], np.flatnonzero(z["mask"] == 0))
    for i, st in enumerate(ref["stages"]):
        c = st["tok_cell"]
        byx = np.stack([c // (st["Y"] * st["X"]), (c // st["X"]) % st["Y"], c % st["X"]], axis=-1)
        assert np.array_equal(byx, z[f"st{i}_indices"]), f"stage {i} active set"
        for s, w in enumerate(st["windows"]):
            assert np.array_equal(w["tok_win"], z[f"st{i}_win_id{s}"])
            assert np.array_equal(w["tok_level"], z[f"st{i}_level{s}"])
            assert np.array_equal(w["tok_slot"], z[f"st{i}_slot{s}"])
    _check_consistency(ref, B)


def _check_consistency(ref, B):
    """The relations every consumer of the plan relies on, checked on the reference itself."""
    prev_n = len(ref["tok_pillar"])
    assert np.all(np.diff(ref["tok_pillar"]) > 0)
    for i, st in enumerate(ref["stages"]):
        n = st["n_tok"]
        assert st["map"].shape == (B * st["Y"] * st["X"],) and (st["map"] >= 0).sum() == n
        assert np.array_equal(st["map"][st["tok_cell"]], np.arange(n))
        nb = st["nbr_subm"]
        assert nb.shape == (n, 9) and np.array_equal(nb[:, 4], np.arange(n)) and nb.max(initial=-1) < n
        # submanifold: t' = nbr[t, k]  <=>  t = nbr[t', 8 - k]; the transposed rulebook is the tap-flipped one
        t, k = np.nonzero(nb >= 0)
        assert np.array_equal(nb[nb[t, k], 8 - k], t)
        assert np.array_equal(st["nbr_subm_t"], nb[:, ::-1])
        if st["nbr_down"] is not None:
            nd, ndt = st["nbr_down"], st["nbr_down_t"]
            assert nd.shape == (n, 9) and ndt.shape == (prev_n, 9)
            assert (nd >= 0).any(axis=1).all(), "an active output has an active input"
            o, k = np.nonzero(nd >= 0)
            assert np.array_equal(ndt[nd[o, k], k], o) and (ndt >= 0).sum() == (nd >= 0).sum()
            assert prev_n == 0 or (ndt >= 0).any(axis=1).all(), "every input feeds an output"
        if st["up_sites"] is not None:
            u = st["up_sites"]
            assert u.shape == (n, st["up_s"] ** 2) and len(np.unique(u)) == u.size
        for w in st["windows"]:
            csr = w["csr_tok"]
            assert np.array_equal(np.sort(csr), np.arange(n)), "the CSR is a permutation of the tokens"
            assert w["win_len"].sum() == n == sum(w["n_tok"]) and len(w["win_len"]) == sum(w["n_win"])
            assert np.array_equal(w["win_start"], np.r_[0, np.cumsum(w["win_len"])[:-1]] if len(w["win_len"]) else w["win_start"])
            lo = 0
            for l in range(3):      # windows are level-major, ascending window id inside a level, tokens ascending inside a window
                ids = []
                for q in range(lo, lo + w["n_win"][l]):
                    seg = csr[w["win_start"][q]:w["win_start"][q] + w["win_len"][q]]
                    assert len(seg) > 0 and np.all(np.diff(seg) > 0)
                    assert len(set(w["tok_win"][seg])) == 1 and set(w["tok_level"][seg]) == {l}
                    assert np.array_equal(w["tok_slot"][seg], (q - lo) * (16, 32, 64)[l] + np.arange(len(seg)))
                    ids.append(int(w["tok_win"][seg[0]]))
                assert ids == sorted(set(ids))
                lo += w["n_win"][l]
            assert len(np.unique(w["tok_win"] * 64 + w["tok_pos"])) == n and (w["tok_pos"] >= 0).all() and (w["tok_pos"] < 64).all()
        prev_n = n
    d = ref["dec"]
    if d is not None:
        assert np.array_equal(np.flatnonzero(d["tile_slot"] >= 0), d["tile_list"]) and d["n_act"] == len(d["tile_list"])
        assert np.array_equal(d["tile_slot"][d["tile_list"]], np.arange(d["n_act"]))
        for nbr in d["nbr"]:
            assert (nbr[:, 4] >= 0).all(), "an active site lies in an active tile"


@pytest.mark.parametrize("name", PS.NAMES)
def test_reference_plan_is_self_consistent_on_the_crafted_scenes(name):
    sc, pts, noise, ref = PS.build(name)         # build() asserts what the scene promises (populations per shift, capacities, ...)
    _check_consistency(ref, sc.B)
    assert (ref["dec"] is not None) == (sc.Y % 4 == 0 and sc.X % 4 == 0)
    ws = [st["windows"] for st in ref["stages"]]
    print(f"{name}: cells={sc.B * sc.Y * sc.X} points={len(pts)} pillars={ref['M']} tokens={[st['n_tok'] for st in ref['stages']]} "
          f"window_grid={[sc.B * ((st['X'] + 7) // 8 + 1) * ((st['Y'] + 7) // 8 + 1) for st in ref['stages']]} "
          f"windows={[[sum(w['n_win']) for w in s] for s in ws]} levels_shift0={[w[0]['n_win'] for w in ws]}")


def test_scene_seams_are_reached():
    """The counts the scenes exist for, read from the reference."""
    cells = {n: PS.SCENES[n].B * PS.SCENES[n].Y * PS.SCENES[n].X for n in PS.NAMES}
    assert {4095, 4096, 4097, 65535, 65536, 65537} <= set(cells.values())
    assert {PS.build(n)[3]["M"] for n in ("pillars_4095", "pillars_4096", "pillars_4097")} == {4095, 4096, 4097}
    assert {PS.build(n)[3]["M"] for n in ("cells_65535_full", "cells_65536_full", "cells_65537_full")} == {65535, 65536, 65537}
    for n in ("cells_4095", "cells_4096", "cells_4097", "cells_65535_full", "cells_65536_full", "cells_65537_sparse"):
        st0 = PS.build(n)[3]["stages"][0]
        sc = PS.SCENES[n]
        vc = PS.build(n)[3]["voxel_coords"]
        assert tuple(vc[0][[0, 2, 3]]) == (0, 0, 0) and tuple(vc[-1][[0, 2, 3]]) == (sc.B - 1, sc.Y - 1, sc.X - 1), n
        assert st0["n_tok"] > 0
    full = PS.build("full_24x24")[3]["stages"][0]["windows"][0]
    assert full["n_win"] == [0, 0, 18] and set(full["pop"].tolist()) == {64}      # every un-shifted window is full: levels 0, 1 empty
    kf = {PS.SCENES[n].keep_frac for n in PS.NAMES}
    assert kf == {None, 1.0, 0.25, 0.5} and any(s.coarse_noise and s.keep_frac == 0.5 for s in PS.SCENES.values())
    # coarse noise: ties straddle the keep boundary (the threshold value occurs on both sides of it)
    sc, _, noise, ref = PS.build("pillars_4097")
    nz = noise[:ref["M"]]
    thr = np.sort(nz)[int(ref["M"] * 0.5) - 1]
    assert ((nz == thr) & (ref["mask"] == 0)).any() and ((nz == thr) & (ref["mask"] == 1)).any()
    empty = PS.build("no_pillars")[3]
    assert empty["N"] == 0 and empty["M"] == 0 and all(st["n_tok"] == 0 for st in empty["stages"]) and empty["dec"]["n_act"] == 0
    mid = PS.build("middle_sample_empty")[3]["voxel_coords"][:, 0]
    assert set(mid.tolist()) == {0, 2}
    assert set(PS.build("last_sample_empty")[3]["voxel_coords"][:, 0].tolist()) == {0, 1}


def _layout(cap_points, gx, gy, B=1):
    from gdmae_hip import lib as L
    strides, wins, drops = PS.plan_args()
    P = L.PlanParams()
    P.n_points, P.cap_points, P.n_cols, P.batch_size = cap_points, cap_points, 5, B
    for i in range(3):
        P.lo[i], P.vs[i] = (0.0, 0.0, -1.0)[i], (0.5, 0.5, 2.0)[i]
        P.grid[i] = (gx, gy, 1)[i]
    P.n_stages = len(strides)
    for i, (s, w, d) in enumerate(zip(strides, wins, drops)):
        d = {int(k): v for k, v in d.items()}
        P.stride[i], P.win_x[i], P.win_y[i], P.n_levels[i] = int(s), int(w[0]), int(w[1]), len(d)
        for l in range(len(d)):
            P.drop_lo[i][l], P.drop_hi[i][l] = (int(v) for v in d[l]["drop_range"])
            P.max_tokens[i][l] = int(d[l]["max_tokens"])
    P.masked, P.keep_frac, P.n_dec, P.want_pm = 0, 1.0, 0, 1
    lib = L.load()
    n_ent, total = C.c_int(0), C.c_size_t(0)
    rc = lib.gdmae_geometry_plan_layout(C.byref(P), None, 0, C.byref(n_ent), C.byref(total))
    return rc, lib.gdmae_last_error().decode(), int(total.value)


def test_layout_refuses_a_token_capacity_of_2_pow_21():
    """The packed window scan keeps 21 bits per occupancy level for the token prefix: the plan layout (host only, no kernel) must
    refuse a stage that could hold 2^21 tokens, and accept one token fewer."""
    lim = 1 << 21
    rc, err, _ = _layout(lim, 2048, 1024)                  # 2^21 cells, 2^21 points: capacity min(points, cells) = 2^21
    assert rc != 0 and "2^21" in err and "capacity" in err, (rc, err)
    rc, err, _ = _layout(lim + 5000, 2048, 1028)           # both above
    assert rc != 0 and "2^21" in err and "capacity" in err, (rc, err)
    rc, err, total = _layout(lim - 1, 2048, 1024)          # one point fewer: capacity 2^21 - 1 fits
    assert rc == 0 and total > 0, (rc, err)
    rc, err, total = _layout(lim + 5000, 2048, 1023)       # one row fewer: the cell count bounds the capacity below 2^21
    assert rc == 0 and total > 0, (rc, err)
