"""Crafted occupancy grids for the geometry-plan tests (tests/test_plan_reference_cpu.py, tests/test_geometry_plan_edges.py).

A scene lists the occupied cells of a (B, Y, X) pillar grid; ``build`` places one point at the centre of every listed cell (and
a few more inside some of them where ``extra`` asks for pillars with several points), so the occupancy map is exactly what the
scene says.  Every scene uses the shipped three-stage block list (strides 1, 2, 2), 8 x 8 windows, the shipped drop ranges
[0, 16), [16, 32), [32, 100000) and a seeded noise vector with one value per CELL (>= the pillar capacity of either builder).

The scenes are the smallest that still reach each seam of the plan kernels:
  scan seams   cell counts 4095 / 4096 / 4097 (one look-back tile +- 1) and 65535 / 65536 / 65537 (single-launch limit of the
               three-launch scan +- 1; fully occupied, so the PILLAR count straddles it too); pillar counts 4095 / 4096 / 4097;
               window-grid sizes 4095 / 4096 / 4097.  First and last cell occupied.
  extents      odd in both directions, X < 8, Y = 1, exactly one window
  occupancy    full grid, four corners, isolated odd sites (every token activates four strided outputs: the down-sampled
               capacity min(4 * cap, B * Y * X) is reached exactly), windows of 1, 15, 16, 17, 31, 32, 33, 63, 64 tokens in
               each shift (the drop-range borders)
  batch        B = 3 with the middle / the last sample empty, a sample whose keep count truncates to zero
  masking      keep_frac None, 1.0, 0.25 and 0.5 with coarse noise (ties that straddle the keep boundary)
  empty        every point outside the range
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

VS = 0.5                      # pillar size: cell centres are exact in fp32
POPULATIONS = (1, 15, 16, 17, 31, 32, 33, 63, 64)


@dataclass
class Scene:
    name: str
    B: int
    Y: int
    X: int
    cells: np.ndarray                       # (n, 3) int64 (b, y, x), distinct
    keep_frac: Optional[float] = None
    coarse_noise: bool = False
    extra: int = 0                          # additional points placed into already occupied cells
    outside: int = 0                        # additional points outside the range
    seed: int = 0
    expect: dict = field(default_factory=dict)


def _rand_cells(seed, B, Y, X, n, ends=True):
    """n distinct cells, the first and the last cell of the grid among them."""
    rng = np.random.default_rng(seed)
    total = B * Y * X
    lin = rng.choice(total, size=n, replace=False)
    if ends:
        lin = np.unique(np.r_[lin, 0, total - 1])
        drop = [i for i in rng.permutation(len(lin)) if lin[i] not in (0, total - 1)][:len(lin) - n]
        lin = np.delete(lin, drop)
    lin = np.sort(lin)
    assert len(lin) == n
    return np.stack([lin // (Y * X), (lin // X) % Y, lin % X], axis=-1).astype(np.int64)


def _full(B, Y, X, samples=None):
    b, y, x = np.meshgrid(np.arange(B) if samples is None else np.asarray(samples), np.arange(Y), np.arange(X), indexing="ij")
    return np.stack([b.ravel(), y.ravel(), x.ravel()], axis=-1).astype(np.int64)


def _population_cells():
    """Windows of exactly POPULATIONS tokens: aligned 8 x 8 blocks for the un-shifted pass (window origin at multiples of 8) and
    blocks at offset 4 for the shifted pass (origin at 8 k - 4); blocks are 16 apart so that none shares a window with another."""
    out = []
    for i, p in enumerate(POPULATIONS):
        for y0, x0 in ((0, 16 * i), (20, 16 * i + 4)):
            out += [(0, y0 + q // 8, x0 + q % 8) for q in range(p)]
    return np.asarray(out, dtype=np.int64)


def _scenes():
    S = []
    # ---- scan seams over the cells (look-back tile = 4096)
    S.append(Scene("cells_4095", 1, 63, 65, _rand_cells(1, 1, 63, 65, 700), keep_frac=0.25, seed=1))
    S.append(Scene("cells_4096", 1, 64, 64, _rand_cells(2, 1, 64, 64, 700), keep_frac=None, seed=2, extra=300))
    S.append(Scene("cells_4097", 1, 17, 241, _rand_cells(3, 1, 17, 241, 700), keep_frac=0.5, coarse_noise=True, seed=3))
    # ---- ... and around 65536, fully occupied: cells, pillars and stage-1 tokens all sit on the seam
    S.append(Scene("cells_65535_full", 1, 255, 257, _full(1, 255, 257), keep_frac=None, seed=4))
    S.append(Scene("cells_65536_full", 1, 256, 256, _full(1, 256, 256), keep_frac=0.25, seed=5))
    S.append(Scene("cells_65537_full", 1, 1, 65537, _full(1, 1, 65537), keep_frac=None, seed=6))
    S.append(Scene("cells_65537_sparse", 1, 1, 65537, _rand_cells(7, 1, 1, 65537, 5000), keep_frac=0.25, seed=7))
    # ---- pillar counts around one scan tile
    S.append(Scene("pillars_4095", 1, 96, 96, _rand_cells(8, 1, 96, 96, 4095), keep_frac=None, seed=8))
    S.append(Scene("pillars_4096", 1, 96, 96, _rand_cells(9, 1, 96, 96, 4096), keep_frac=1.0, seed=9))
    S.append(Scene("pillars_4097", 1, 96, 96, _rand_cells(10, 1, 96, 96, 4097), keep_frac=0.5, coarse_noise=True, seed=10))
    # ---- window-grid sizes B * (ceil(X / 8) + 1) * (ceil(Y / 8) + 1) around one scan tile
    S.append(Scene("windows_4095", 3, 16, 3632, _rand_cells(11, 3, 16, 3632, 3000), keep_frac=None, seed=11,
                   expect={"n_win_grid": 4095}))
    S.append(Scene("windows_4096", 1, 8, 16376, _rand_cells(12, 1, 8, 16376, 3000), keep_frac=1.0, seed=12,
                   expect={"n_win_grid": 4096}))
    S.append(Scene("windows_4097", 1, 128, 1920, _rand_cells(13, 1, 128, 1920, 3000), keep_frac=0.25, seed=13,
                   expect={"n_win_grid": 4097}))
    # ---- extents
    S.append(Scene("odd_37x51", 2, 37, 51, _rand_cells(14, 2, 37, 51, 900), keep_frac=0.25, seed=14, extra=200))
    S.append(Scene("narrow_x5", 2, 19, 5, _rand_cells(15, 2, 19, 5, 60), keep_frac=None, seed=15))
    S.append(Scene("single_row", 1, 1, 29, _rand_cells(16, 1, 1, 29, 17), keep_frac=1.0, seed=16))
    S.append(Scene("one_window", 1, 8, 8, _rand_cells(17, 1, 8, 8, 23), keep_frac=None, seed=17))
    # ---- occupancy
    S.append(Scene("full_24x24", 2, 24, 24, _full(2, 24, 24), keep_frac=None, seed=18))
    S.append(Scene("corners", 1, 24, 40, np.asarray([(0, 0, 0), (0, 0, 39), (0, 23, 0), (0, 23, 39)], dtype=np.int64), keep_frac=None,
                   seed=19))
    odd = np.asarray([(b, y, x) for b in range(2) for y in range(1, 32, 4) for x in range(1, 32, 4)], dtype=np.int64)
    S.append(Scene("isolated_odd", 2, 32, 32, odd, keep_frac=None, seed=20, expect={"four_outputs": True}))
    S.append(Scene("populations", 1, 32, 144, _population_cells(), keep_frac=None, seed=21, expect={"populations": True}))
    # ---- batch
    c = _rand_cells(22, 1, 24, 24, 150)
    S.append(Scene("middle_sample_empty", 3, 24, 24, np.concatenate([c, c[::2] + np.asarray([2, 0, 0])]), keep_frac=0.25, seed=22))
    S.append(Scene("last_sample_empty", 3, 24, 24, np.concatenate([c[1::2], c + np.asarray([1, 0, 0])]), keep_frac=0.5,
                   coarse_noise=True, seed=23))
    S.append(Scene("keep_count_zero", 2, 16, 16, np.concatenate([_rand_cells(24, 1, 16, 16, 40), np.asarray([(1, 7, 9)])]),
                   keep_frac=0.25, seed=24, expect={"sample1_tokens": 0}))
    # ---- nothing inside the range
    S.append(Scene("no_pillars", 2, 16, 24, np.zeros((0, 3), dtype=np.int64), keep_frac=0.25, seed=25, outside=37))
    S.append(Scene("no_pillars_unmasked", 1, 12, 20, np.zeros((0, 3), dtype=np.int64), keep_frac=None, seed=26, outside=5))
    return S


SCENES = {s.name: s for s in _scenes()}
NAMES = list(SCENES)
DEC_SOURCES = (0, 1, 2)          # the shipped FEATURES_SOURCE: x_conv1, x_conv2, x_conv3


def plan_args():
    """(strides, window shapes, drop infos) of the shipped block list, through stage_plan_args like the product."""
    from gdmae_hip import configs
    from pcdet.models.backbones_3d.spt_backbone import stage_plan_args
    bb = configs.gdmae_ssl_model_cfg().BACKBONE_3D
    assert tuple(int(s[-1]) - 1 for s in bb.FEATURES_SOURCE) == DEC_SOURCES
    return stage_plan_args(bb.SST_BLOCK_LIST)


def geometry(scene):
    """(point_cloud_range, voxel_size, grid_size) of a scene."""
    return [0.0, 0.0, -1.0, scene.X * VS, scene.Y * VS, 1.0], [VS, VS, 2.0], [scene.X, scene.Y, 1]


def points_of(scene):
    """(N0, 5) fp32 rows [b, x, y, z, intensity], grouped by sample, shuffled inside a sample."""
    rng = np.random.default_rng(1000 + scene.seed)
    c = scene.cells.reshape(-1, 3)
    assert len(np.unique((c[:, 0] * scene.Y + c[:, 1]) * scene.X + c[:, 2])) == len(c), "scene cells must be distinct"
    assert len(c) == 0 or (c.min(0) >= 0).all() and (c.max(0) < [scene.B, scene.Y, scene.X]).all()
    xyz = np.stack([c[:, 0], (c[:, 2] + 0.5) * VS, (c[:, 1] + 0.5) * VS, np.zeros(len(c))], axis=-1)
    if scene.extra:
        pick = c[rng.integers(0, len(c), scene.extra)]
        off = rng.uniform(-0.2, 0.2, (scene.extra, 2))
        xyz = np.concatenate([xyz, np.stack([pick[:, 0], (pick[:, 2] + 0.5 + off[:, 0]) * VS, (pick[:, 1] + 0.5 + off[:, 1]) * VS,
                                             rng.uniform(-0.5, 0.5, scene.extra)], axis=-1)])
    if scene.outside:
        far = np.stack([rng.integers(0, scene.B, scene.outside), scene.X * VS + rng.uniform(2, 9, scene.outside),
                        -rng.uniform(2, 9, scene.outside), np.zeros(scene.outside)], axis=-1)
        xyz = np.concatenate([xyz, far])
    pts = np.concatenate([xyz, rng.uniform(0, 1, (len(xyz), 1))], axis=-1).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    return pts[np.argsort(pts[:, 0], kind="stable")]


def noise_of(scene):
    """One seeded fp32 value per CELL: covers the pillar capacity of both builders (the exact count / min(points, cells))."""
    rng = np.random.default_rng(2000 + scene.seed)
    n = scene.B * scene.Y * scene.X
    if scene.coarse_noise:
        return (rng.integers(0, 50, n) / 50).astype(np.float32)
    return rng.random(n, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def build(name):
    """-> (scene, points, noise, reference plan).  Computed once per process and shared by every test: treat as read-only.
    Asserts on the CPU what the scene promises (occupancy, token drop = identity, the seam it is meant to reach)."""
    from plan_reference import reference_plan
    sc = SCENES[name]
    pts, noise = points_of(sc), noise_of(sc)
    pcr, vs, grid = geometry(sc)
    strides, wins, drops = plan_args()
    assert all(list(w) == [8, 8, 1] for w in wins) and list(strides) == [1, 2, 2]
    ref = reference_plan(pts, pcr, vs, grid, sc.B, strides, wins, drops, sc.keep_frac, noise, DEC_SOURCES)
    c = sc.cells.reshape(-1, 3)
    assert ref["M"] == len(c) and np.array_equal(ref["voxel_coords"][:, [0, 2, 3]], c[np.lexsort((c[:, 2], c[:, 1], c[:, 0]))])
    for st in ref["stages"]:
        for w in st["windows"]:
            assert w["keep"].all(), "token drop must be the identity"
    e = sc.expect
    if "n_win_grid" in e:
        assert sc.B * ((sc.X + 7) // 8 + 1) * ((sc.Y + 7) // 8 + 1) == e["n_win_grid"]
    if e.get("four_outputs"):
        assert ref["stages"][1]["n_tok"] == min(4 * ref["stages"][0]["n_tok"], sc.B * ref["stages"][1]["Y"] * ref["stages"][1]["X"])
        assert ref["stages"][1]["n_tok"] == 4 * ref["stages"][0]["n_tok"] == sc.B * ref["stages"][1]["Y"] * ref["stages"][1]["X"]
    if e.get("populations"):
        for sh, w in enumerate(ref["stages"][0]["windows"]):
            missing = set(POPULATIONS) - set(w["pop"].tolist())
            assert not missing, f"shift {sh}: no window with {sorted(missing)} tokens"
    if "sample1_tokens" in e:
        assert int((ref["stages"][0]["tok_cell"] >= sc.Y * sc.X).sum()) == e["sample1_tokens"] and ref["stages"][0]["n_tok"] > 0
    return sc, pts, noise, ref
