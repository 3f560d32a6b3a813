"""Plain CPU reference of the whole geometry plan (NumPy / CPU torch; imports no GPU code).

``reference_plan`` returns every field the two GPU builders return (``gdmae_hip.plan.encoder_plan`` and
``PlanPrefetch.finish``).  It reuses the pieces of ``oracle/`` that are pinned against the reference project's
goldens - ``point_coords``, ``unique_pillars``, ``mae_mask``, ``window_partition`` and the output active set of
``thirdparty.sparse_conv2d`` - and restates the rest from the definitions written down in ``gdmae_hip/plan.py`` and
the comments of ``csrc/partition.hip``:

* ``tok_cell``      linear key (b * Y + y) * X + x of every token, ascending; ``map`` its inverse, -1 for empty cells
* ``nbr_subm``      nbr[t, ky * 3 + kx] = token at (y + ky - 1, x + kx - 1) / -1; ``nbr_subm_t`` = tap-flipped copy
* ``nbr_down``      nbr[o, k] = token of the previous stage at in = 2 * o - 1 + k / -1
* ``nbr_down_t``    the exact inverse relation: nbr_t[i, k] = o  iff  nbr_down[o, k] = i, -1 elsewhere
* ``up_sites``      the s x s full-resolution cells under every token of a stage that tiles the pillar grid
* windows           ``tok_pos`` = ly * wx + lx of the shifted in-window coordinate; windows ordered level-major and by
                    ascending window id inside a level; ``csr_tok`` lists the tokens of a window in ascending order
* decoder tiles     an 8 x 8 tile is active iff a site of its one-site halo is covered by a token of a source stage;
                    ``nbr[g][site, k]`` = tile-compact row (slot * 64 + (y & 7) * 8 + (x & 7)) of site - (ky - 1, kx - 1)

tests/test_plan_reference_cpu.py validates it against the goldens before anything on the GPU is judged by it.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import gdmae_oracle as orc
from oracle import thirdparty as tp


def _drop(drop_info):
    return {int(k): {"max_tokens": int(v["max_tokens"]), "drop_range": [int(v["drop_range"][0]), int(v["drop_range"][1])]}
            for k, v in dict(drop_info).items()}


def _cells_to_byx(cell, Y, X):
    cell = np.asarray(cell, dtype=np.int64)
    return np.stack([cell // (Y * X), (cell // X) % Y, cell % X], axis=-1)


def _lookup(cmap, B, Y, X, b, y, x):
    """map[b, y, x] where (y, x) lies inside the grid, -1 elsewhere (broadcasting integer arrays)."""
    ok = (y >= 0) & (y < Y) & (x >= 0) & (x < X)
    v = cmap.reshape(B, Y, X)[b, np.clip(y, 0, Y - 1), np.clip(x, 0, X - 1)]
    return np.where(ok, v, -1).astype(np.int64)


def upsample_cells(cell, Ys, Xs, s):
    """(n, s * s) full-resolution cells ((b * Y + y) * X + x, Y = Ys * s, X = Xs * s) covered by the stride-s cells."""
    byx = _cells_to_byx(cell, Ys, Xs)
    out = np.empty((len(byx), s * s), dtype=np.int64)
    for dy in range(s):
        for dx in range(s):
            out[:, dy * s + dx] = (byx[:, 0] * (Ys * s) + byx[:, 1] * s + dy) * (Xs * s) + byx[:, 2] * s + dx
    return out


def _windows(byx, Y, X, window_shape, shifted, drop):
    """One shift of one stage from ``orc.window_partition``."""
    wx, wy, wz = (int(v) for v in window_shape)
    n = len(byx)
    coords = torch.from_numpy(np.stack([byx[:, 0], np.zeros(n, np.int64), byx[:, 1], byx[:, 2]], axis=-1).astype(np.int64))
    part = orc.window_partition(coords, [X, Y, 1], [wx, wy, wz], bool(shifted), drop)
    win = part["win_id"].numpy()
    level = part["level"].numpy()
    rank = part["rank"].numpy()
    in_win = part["in_win"].numpy()
    nlev = len(drop)
    # windows level-major, ascending window id inside a level; tokens of a window in ascending token order
    by_win = {}
    for t in range(n):
        by_win.setdefault((int(level[t]), int(win[t])), []).append(t)
    win_start, win_len, csr = [], [], []
    for key in sorted(by_win):
        toks = by_win[key]
        assert [int(rank[t]) for t in toks] == list(range(len(toks)))
        win_start.append(len(csr))
        win_len.append(len(toks))
        csr.extend(toks)
    i64 = lambda a: np.asarray(a, dtype=np.int64).reshape(-1)                     # noqa: E731
    return {"tok_win": win, "tok_level": level, "tok_slot": part["slot"].numpy(),
            "tok_pos": (in_win[:, 1] * wx + in_win[:, 2]).astype(np.int64) if n else np.zeros(0, np.int64),
            "csr_tok": i64(csr), "win_start": i64(win_start), "win_len": i64(win_len),
            "n_win": [int(part["num_win"].get(l, 0)) for l in range(nlev)] + [0] * (3 - nlev),
            "n_tok": [int((level == l).sum()) for l in range(nlev)] + [0] * (3 - nlev),
            "keep": part["keep"].numpy(), "pop": i64(win_len)}


def _decoder(stages, sources, B, H, W):
    """Active 8 x 8 tiles of the (B, H, W) map for the given source stages and the per-source site rulebooks."""
    cover = np.zeros((B, H, W), dtype=bool)
    for si in sources:
        st = stages[si]
        occ = (st["map"] >= 0).reshape(B, st["Y"], st["X"])
        cover |= np.repeat(np.repeat(occ, st["up_s"], axis=1), st["up_s"], axis=2)
    TH, TW = (H + 7) // 8, (W + 7) // 8
    tile_slot = -np.ones(B * TH * TW, dtype=np.int64)
    tile_list = []
    for b in range(B):
        for ty in range(TH):
            for tx in range(TW):
                y0, y1, x0, x1 = max(ty * 8 - 1, 0), min(ty * 8 + 9, H), max(tx * 8 - 1, 0), min(tx * 8 + 9, W)
                if cover[b, y0:y1, x0:x1].any():
                    t = (b * TH + ty) * TW + tx
                    tile_slot[t] = len(tile_list)
                    tile_list.append(t)
    nbrs = []
    for si in sources:
        st = stages[si]
        sites = st["tok_cell"] if st["up_s"] == 1 else st["up_sites"].reshape(-1)
        byx = _cells_to_byx(sites, H, W)
        nbr = -np.ones((len(sites), 9), dtype=np.int64)
        for k in range(9):
            uy, ux = byx[:, 1] - (k // 3 - 1), byx[:, 2] - (k % 3 - 1)
            ok = (uy >= 0) & (uy < H) & (ux >= 0) & (ux < W)
            sl = tile_slot[(byx[:, 0] * TH + np.clip(uy, 0, H - 1) // 8) * TW + np.clip(ux, 0, W - 1) // 8]
            nbr[:, k] = np.where(ok & (sl >= 0), sl * 64 + (uy % 8) * 8 + (ux % 8), -1)
        nbrs.append(nbr)
    return {"sources": tuple(sources), "B": B, "H": H, "W": W, "n_act": len(tile_list), "tile_slot": tile_slot,
            "tile_list": np.asarray(tile_list, dtype=np.int64), "nbr": nbrs}


def reference_plan(points, point_cloud_range, voxel_size, grid_size, batch_size, strides, window_shapes, drop_infos,
                   keep_frac=None, noise=None, dec_sources=None):
    """points (N0, 1 + F) fp32 [b, x, y, z, ...]; noise: at least one fp32 value per pillar (needed when keep_frac is set).
    -> dict of NumPy int64 arrays (``mask`` fp32), see the module docstring."""
    points = torch.as_tensor(points, dtype=torch.float32)
    gx, gy, gz = (int(g) for g in grid_size)
    assert gz == 1
    B = int(batch_size)
    keep, coords = orc.point_coords(points, point_cloud_range, voxel_size, grid_size)
    vc, inverse, rank, counts = orc.unique_pillars(coords, grid_size)
    M = int(vc.shape[0])
    out = {"N": int(keep.sum()), "M": M, "voxel_coords": vc.numpy()}
    if keep_frac is not None:
        noise = torch.as_tensor(noise, dtype=torch.float32)[:M]
        assert noise.numel() == M
        ratio = 1.0 - float(keep_frac)
        for b in range(B):      # the builders evaluate int(L * keep_frac), the oracle int(L * (1 - ratio)): the same number here
            L = int((vc[:, 0] == b).sum())
            assert int(L * (1 - ratio)) == int(L * float(keep_frac))
        mask = orc.mae_mask(vc, B, ratio, noise).numpy().astype(np.float32)
        vis = np.flatnonzero(mask == 0)
        out["mask"] = mask
    else:
        vis = np.arange(M)
        out["mask"] = None
    out["tok_pillar"] = vis.astype(np.int64)
    idx = vc.numpy()[vis][:, [0, 2, 3]].astype(np.int64).reshape(-1, 3)     # (b, y, x), ascending linear key
    Y, X = gy, gx
    stages = []
    prev = None
    for si, stride in enumerate(int(s) for s in strides):
        nbr_down = nbr_down_t = None
        if stride > 1:
            assert stride == 2
            n_in, Yi, Xi, map_in = len(idx), Y, X, (prev["map"] if prev is not None else None)
            if map_in is None:                      # a strided first stage: its input set is the visible pillars
                map_in = -np.ones(B * Yi * Xi, dtype=np.int64)
                map_in[(idx[:, 0] * Yi + idx[:, 1]) * Xi + idx[:, 2]] = np.arange(n_in)
            _, oidx, oshape = tp.sparse_conv2d(torch.ones(n_in, 1), torch.from_numpy(idx).int(), [Yi, Xi], B,
                                               torch.ones(1, 3, 3, 1), 2, 1)
            idx = oidx.numpy().astype(np.int64).reshape(-1, 3)
            Y, X = int(oshape[0]), int(oshape[1])
            assert (Y, X) == ((Yi - 1) // 2 + 1, (Xi - 1) // 2 + 1)
            nbr_down = -np.ones((len(idx), 9), dtype=np.int64)
            for k in range(9):                                       # in = 2 * o - 1 + k
                nbr_down[:, k] = _lookup(map_in, B, Yi, Xi, idx[:, 0], 2 * idx[:, 1] - 1 + k // 3, 2 * idx[:, 2] - 1 + k % 3)
            nbr_down_t = -np.ones((n_in, 9), dtype=np.int64)           # the exact inverse relation
            o, k = np.nonzero(nbr_down >= 0)
            nbr_down_t[nbr_down[o, k], k] = o
        n = len(idx)
        cell = (idx[:, 0] * Y + idx[:, 1]) * X + idx[:, 2]
        assert np.all(np.diff(cell) > 0)
        cmap = -np.ones(B * Y * X, dtype=np.int64)
        cmap[cell] = np.arange(n)
        nbr_subm = -np.ones((n, 9), dtype=np.int64)
        for k in range(9):
            nbr_subm[:, k] = _lookup(cmap, B, Y, X, idx[:, 0], idx[:, 1] + k // 3 - 1, idx[:, 2] + k % 3 - 1)
        us = gy // Y
        up_s = us if (us >= 1 and us * Y == gy and us * X == gx) else 0
        drop = _drop(drop_infos[si])
        st = {"B": B, "Y": Y, "X": X, "n_tok": n, "tok_cell": cell, "map": cmap, "nbr_subm": nbr_subm,
              "nbr_subm_t": nbr_subm[:, ::-1].copy(), "nbr_down": nbr_down, "nbr_down_t": nbr_down_t, "up_s": up_s,
              "up_sites": upsample_cells(cell, Y, X, up_s) if up_s > 1 else None,
              "windows": [_windows(idx, Y, X, window_shapes[si], sh, drop) for sh in (0, 1)]}
        stages.append(st)
        prev = st
    out["stages"] = stages
    out["dec"] = None
    if dec_sources is not None:
        srcs = [int(i) for i in dec_sources]
        if all(stages[i]["up_s"] in (1, 2, 4, 8) for i in srcs):
            out["dec"] = _decoder(stages, srcs, B, gy, gx)
    return out
