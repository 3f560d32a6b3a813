"""GPU: both builders of the geometry plan - the per-operator path (plan.voxelize + plan.encoder_plan: csrc/partition.hip entry
points, three-launch scans) and the one-call path (PlanPrefetch -> gdmae_geometry_plan: csrc/plan.hip, look-back scans, merged
launches, capacity-bucketed arena) - on the crafted grids of tests/plan_scenes.py against the plain CPU reference of
tests/plan_reference.py (validated against the goldens by tests/test_plan_reference_cpu.py).

Every field is compared exhaustively and exactly (all quantities are integers; the mask holds 0.0 / 1.0): each path with the
reference, the two paths with each other, and two builds of the one-call plan with each other.  Capacity-sized buffers are
compared on their counted prefix, the cell maps in full."""
import numpy as np
import pytest
import torch

import plan_scenes as PS

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _a(t):
    return t.detach().cpu().numpy().astype(np.int64)


def _reference_fields(sc, ref):
    vc = ref["voxel_coords"]
    B, M = sc.B, ref["M"]
    c2p = -np.ones(B * sc.Y * sc.X, dtype=np.int64)
    c2p[(vc[:, 0] * sc.Y + vc[:, 2]) * sc.X + vc[:, 3]] = np.arange(M)
    f = {"N": ref["N"], "M": M, "voxel_coords": vc, "sample_off": np.searchsorted(vc[:, 0], np.arange(B + 1)).astype(np.int64),
         "cell2pillar": c2p, "mask": ref["mask"], "tok_pillar": ref["tok_pillar"]}
    for i, st in enumerate(ref["stages"]):
        p = f"s{i}."
        f[p + "geometry"] = (st["B"], st["Y"], st["X"], st["n_tok"])
        for k in ("tok_cell", "map", "nbr_subm", "nbr_subm_t", "nbr_down", "nbr_down_t"):
            f[p + k] = st[k]
        f[p + "up_sites"] = None if st["up_sites"] is None else (st["up_s"], st["up_sites"].reshape(-1))
        for s, w in enumerate(st["windows"]):
            for k in ("tok_win", "tok_level", "tok_slot", "tok_pos", "csr_tok", "win_start", "win_len", "n_win", "n_tok"):
                f[f"{p}w{s}.{k}"] = w[k]
    d = ref["dec"]
    f["dec"] = None if d is None else (d["sources"], d["B"], d["H"], d["W"], d["n_act"])
    if d is not None:
        f["dec.tile_slot"], f["dec.tile_list"] = d["tile_slot"], d["tile_list"]
        for g, nbr in enumerate(d["nbr"]):
            f[f"dec.nbr{g}"] = nbr
    return f


def _plan_fields(vox, ep, dec_nbr):
    """The same dictionary from a GPU plan (the builders hand out the counted prefixes; ``map`` / ``tile_slot`` are full-size)."""
    f = {"N": vox.N, "M": vox.M, "voxel_coords": _a(vox.voxel_coords), "sample_off": _a(vox.sample_off), "cell2pillar": _a(vox.cell2pillar),
         "mask": None if ep.mask is None else ep.mask.cpu().numpy(), "tok_pillar": _a(ep.tok_pillar)}
    for i, st in enumerate(ep.stages):
        p = f"s{i}."
        f[p + "geometry"] = (st.B, st.Y, st.X, st.n_tok)
        f[p + "tok_cell"], f[p + "map"], f[p + "nbr_subm"], f[p + "nbr_subm_t"] = _a(st.tok_cell), _a(st.map), _a(st.nbr_subm), _a(st._nbr_subm_t)
        f[p + "nbr_down"] = None if st.nbr_down is None else _a(st.nbr_down)
        f[p + "nbr_down_t"] = None if st.nbr_down_t is None else _a(st.nbr_down_t)
        f[p + "up_sites"] = None if st._up_sites is None else (int(st._up_sites[0]), _a(st._up_sites[1]))
        for s, w in enumerate(st.windows):
            for k in ("tok_win", "tok_level", "tok_slot", "tok_pos", "csr_tok", "win_start", "win_len"):
                f[f"{p}w{s}.{k}"] = _a(getattr(w, k))
            f[f"{p}w{s}.n_win"], f[f"{p}w{s}.n_tok"] = list(w.n_win), list(w.n_tok)
    d = ep.dec_tiles
    f["dec"] = None if d is None else (tuple(d.sources), d.B, d.H, d.W, d.n_act)
    if d is not None:
        f["dec.tile_slot"], f["dec.tile_list"] = _a(d.tile_slot), _a(d.tile_list)
        for g, nbr in enumerate(dec_nbr):
            f[f"dec.nbr{g}"] = _a(nbr)
    return f


def _same(a, b, what):
    assert sorted(a) == sorted(b), (what, sorted(set(a) ^ set(b)))
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, tuple) and len(x) == 2 and isinstance(x[1], np.ndarray):        # (up_s, sites)
            assert isinstance(y, tuple) and x[0] == y[0], (what, k)
            x, y = x[1], y[1]
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            assert x is not None and y is not None, (what, k)
            assert x.shape == y.shape, (what, k, x.shape, y.shape)
            if not np.array_equal(x, y):
                bad = np.argwhere(x != y)
                raise AssertionError(f"{what}: {k} differs at {len(bad)} of {x.size} entries, first {bad[0].tolist()}: "
                                     f"{x[tuple(bad[0])]} vs {y[tuple(bad[0])]}")
        else:
            assert x == y, (what, k, x, y)


def _per_operator(sc, pts, noise, ref):
    from gdmae_hip import plan
    pcr, vs, grid = PS.geometry(sc)
    vox = plan.voxelize(pts, pcr, vs, grid, sc.B)
    # one noise value per pillar; a cloud without pillars has none to pass (the builder then draws its own capacity-1 vector)
    nz = None if (sc.keep_frac is None or vox.M == 0) else noise[:vox.M].contiguous()
    ep = plan.encoder_plan(vox, *PS.plan_args(), keep_frac=sc.keep_frac, noise=nz, dec_sources=PS.DEC_SOURCES)
    nbr = None
    if ep.dec_tiles is not None:
        st = [ep.stages[i] for i in PS.DEC_SOURCES]
        ups = [sc.Y // s.Y for s in st]
        nbr = plan.decoder_site_rulebooks(ep.dec_tiles, [s.tok_cell if u == 1 else s._up_sites[1] for s, u in zip(st, ups)], ups)
    return _plan_fields(vox, ep, nbr)


def _one_call(sc, pts, noise):
    from gdmae_hip import plan
    pcr, vs, grid = PS.geometry(sc)
    # capacity-sized noise: the one-call path is handed min(point capacity, cells) values (one per CELL covers it)
    pf = plan.PlanPrefetch(pts, pcr, vs, grid, sc.B, *PS.plan_args(), keep_frac=sc.keep_frac,
                           noise=None if sc.keep_frac is None else noise, dec_sources=PS.DEC_SOURCES)
    vox, ep = pf.finish()
    return _plan_fields(vox, ep, None if ep.dec_tiles is None else ep.dec_tiles.nbr)


@pytest.mark.parametrize("name", PS.NAMES)
def test_both_plan_builders_match_the_cpu_reference(name):
    sc, pts_np, noise_np, ref = PS.build(name)
    want = _reference_fields(sc, ref)
    pts, noise = torch.from_numpy(pts_np).to(_dev()), torch.from_numpy(noise_np).to(_dev())
    print(f"{name}: cells={sc.B * sc.Y * sc.X} points={len(pts_np)} pillars={ref['M']} tokens={[st['n_tok'] for st in ref['stages']]} "
          f"windows={[[sum(w['n_win']) for w in st['windows']] for st in ref['stages']]} "
          f"tiles={None if ref['dec'] is None else ref['dec']['n_act']}")
    a = _per_operator(sc, pts, noise, ref)
    b = _one_call(sc, pts, noise)
    b2 = _one_call(sc, pts, noise)
    torch.cuda.synchronize()
    errors = []
    for x, y, what in ((want, a, "reference vs per-operator path"), (want, b, "reference vs one-call path"),
                       (a, b, "per-operator vs one-call path"), (b, b2, "one-call path built twice")):
        try:
            _same(x, y, f"{name}: {what}")
        except AssertionError as e:         # report every comparison: which path is wrong is half of the finding
            errors.append(str(e))
    assert not errors, "\n".join(errors)
