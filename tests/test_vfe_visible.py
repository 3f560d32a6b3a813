"""DynVFE's second layer for the visible pillars only (gdmae_vfe_max_layer_vis_fwd / _bwd[_f16], the plan's "vfe.*" arrays and the
module switch DynVFE.visible_only) against the full path of the same library.

The reference is the existing code: gdmae_vfe_max_layer_fwd / _bwd[_f16] on every pillar with the gradient zero-filled at the masked
pillars (what GatherUnique's backward hands it), held to fp64 by tests/test_vfe_backward_one_pass.py.  Everything is compared with
torch.equal - no tolerance: the visible path re-associates no sum.

  kernels  the four size lists of test_vfe_backward_one_pass.py x both row types x the masks below; row_tok / vis_rows / vis_tok are
           built on the CPU from the mask.  out / arg of the tokens, statistics, ab, batch moments, running statistics, dy1, dW2, dgamma2,
           dbeta2 and two consecutive calls of the new path are bit-equal.
  plan     row_tok, vis_rows, vis_tok, tok_row_off and Nv of PlanPrefetch on two crafted clouds (one frame; three frames, the middle one
           with a single visible pillar) against the same quantities from vox.row_pillar, ep.tok_pillar and ep.mask on the CPU.
  module   one config-A training step with a prefetched plan, switch on against switch off: loss and every gradient bit-equal."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = {
    "crowded": [1, 700, 3, 1, 2600, 17, 2, 2, 1, 90, 31, 33, 1],      # a crowded pillar; N = 3 482 is not a multiple of 32
    "tiny": [1] * 300,                                                # 32 pillars per tile
    "one_tile": [5, 1, 9, 2],                                         # N = 17: less than one tile
    # 1 313 tiles, N % 32 = 24: 329 workgroups of four tiles, below the 1 024-row caps of csrc/vfe_layer2.hip (v2_grid) - a layer-2 kernel
    # makes a second pass here only where the occupancy query keeps one workgroup per CU resident (256 workgroups)
    "many_tiles": [40] * 600 + [9000, 1, 7, 9000],
}
MASKS = ["all", "first", "last", "largest", "crowded_masked", "every_second", "random_quarter"]


def _visible(sizes, kind):
    """(M,) bool: which pillars are visible"""
    M, s = len(sizes), np.asarray(sizes)
    v = np.zeros(M, dtype=bool)
    if kind == "all":
        v[:] = True
    elif kind == "first":
        v[0] = True
    elif kind == "last":
        v[-1] = True
    elif kind == "largest":                      # one visible pillar that spans many worker ranges (where the case has one)
        v[int(np.argmax(s))] = True
    elif kind == "crowded_masked":               # only the crowded pillars masked (the largest one where none is crowded)
        v[:] = s < 600
        if v.all():
            v[int(np.argmax(s))] = False
    elif kind == "every_second":
        v[::2] = True
    elif kind == "random_quarter":
        rng = np.random.default_rng(M)
        v[rng.permutation(M)[:max(1, M // 4)]] = True
    return v


def _index_arrays(sizes, vis):
    """tok_pillar, row_tok, vis_rows, vis_tok (int32, CPU) from the mask"""
    rowpil = np.repeat(np.arange(len(sizes)), sizes)
    tok_pillar = np.flatnonzero(vis)
    pil_tok = np.where(vis, np.cumsum(vis) - 1, -1)
    row_tok = pil_tok[rowpil]
    vis_rows = np.flatnonzero(row_tok >= 0)
    return tuple(torch.from_numpy(a.astype(np.int32)) for a in (tok_pillar, row_tok, vis_rows, row_tok[vis_rows]))


def test_the_masks_reach_the_small_and_ragged_row_counts():
    nv = {(c, m): int(np.asarray(CASES[c])[_visible(CASES[c], m)].sum()) for c in CASES for m in MASKS}
    assert any(v % 32 != 0 for v in nv.values()) and any(0 < v < 16 for v in nv.values())
    assert nv[("many_tiles", "largest")] == 9000 and nv[("crowded", "largest")] == 2600
    assert all(v > 0 for v in nv.values())


def _bn_buffers(d):
    return torch.zeros(128, device=d), torch.ones(128, device=d), torch.zeros((), dtype=torch.int64, device=d)


@functools.lru_cache(maxsize=None)
def _full(case, f16):
    """Inputs and the full path's forward for one (sizes, row type): computed once, read-only"""
    from gdmae_hip import lib as L
    sizes = CASES[case]
    d = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(len(sizes) * 13 + sizes[0] + int(f16))
    N, M = sum(sizes), len(sizes)
    off = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int32)
    rowpil = torch.repeat_interleave(torch.arange(M, dtype=torch.int32), torch.tensor(sizes))
    y = torch.relu(torch.randn(N, 64, generator=gen))
    for p in range(1, M, 2):                     # every second pillar is made of identical rows: the arg-max is decided by the tie rule
        y[off[p]:off[p + 1]] = y[off[p]].clone()
    y1 = y.to(torch.float16 if f16 else torch.bfloat16).to(d).contiguous()
    W2 = torch.randn(128, 64, generator=gen) * 0.2
    W2d = (W2 if f16 else W2.bfloat16()).to(d).contiguous()
    g2, b2 = (torch.rand(128, generator=gen) + 0.5).to(d), (torch.randn(128, generator=gen) * 0.3).to(d)
    up = torch.randn(M, 128, generator=gen).to(d)
    offd, rpd = off.to(d), rowpil.to(d)
    out = torch.full((M, 128), float("nan"), device=d)
    arg = torch.full((M, 128), -7, dtype=torch.int32, device=d)
    st, ab, mv = torch.empty(256, dtype=torch.float64, device=d), torch.empty(256, device=d), torch.empty(256, device=d)
    rm, rv, nb = _bn_buffers(d)
    ws = torch.empty(L.load().gdmae_vfe_max_layer_workspace_bytes(), dtype=torch.uint8, device=d)
    L.call("gdmae_vfe_max_layer_fwd" + ("_f16" if f16 else ""), L.ptr(y1), N, L.ptr(W2d), L.ptr(offd), L.ptr(rpd), M, L.ptr(g2), L.ptr(b2),
           1e-3, 0.01, L.ptr(rm), L.ptr(rv), L.ptr(nb), L.ptr(st), L.ptr(ab), L.ptr(mv), L.ptr(out), L.ptr(arg), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    return dict(N=N, M=M, y1=y1, W=W2d, gamma=g2, beta=b2, up=up, rowpil=rpd, out=out, arg=arg, stats=st, ab=ab, mv=mv, rm=rm, rv=rv, nb=nb)


def _bwd_outputs(N, rows, d):
    return dict(gm=torch.full((rows, 128), float("nan"), device=d), dy1=torch.full((N, 64), float("nan"), dtype=torch.bfloat16, device=d),
                dg=torch.empty(128, device=d), db=torch.empty(128, device=d), dW=torch.empty(128, 64, device=d))


@pytest.mark.parametrize("f16", [False, True], ids=["bf16_rows", "fp16_rows"])
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("case", list(CASES))
def test_visible_path_is_the_full_path_bit_for_bit(case, mask, f16):
    from gdmae_hip import lib as L
    F = _full(case, f16)
    d, N, M, sfx = F["y1"].device, F["N"], F["M"], "_f16" if f16 else ""
    vis = _visible(CASES[case], mask)
    tok_pillar, row_tok, vis_rows, vis_tok = (t.to(d) for t in _index_arrays(CASES[case], vis))
    n_tok, Nv = tok_pillar.numel(), vis_rows.numel()
    ws = torch.empty(L.load().gdmae_vfe_max_layer_workspace_bytes(), dtype=torch.uint8, device=d)
    # the full path's backward with the gradient zero-filled at the masked pillars
    visd = torch.from_numpy(vis).to(d)
    g_full = torch.where(visd[:, None], F["up"], torch.zeros_like(F["up"])).contiguous()
    want = _bwd_outputs(N, M, d)
    L.call("gdmae_vfe_max_layer_bwd" + sfx, L.ptr(F["y1"]), N, L.ptr(F["W"]), L.ptr(F["rowpil"]), M, L.ptr(F["gamma"]), L.ptr(F["stats"]),
           L.ptr(F["ab"]), L.ptr(F["out"]), L.ptr(F["arg"]), L.ptr(g_full), L.ptr(want["gm"]), L.ptr(want["dy1"]), L.ptr(want["dg"]),
           L.ptr(want["db"]), L.ptr(want["dW"]), 0, L.ptr(ws), L.stream())
    # the visible path, twice
    g_tok = F["up"][tok_pillar.long()].contiguous()
    runs = []
    for _ in range(2):
        out = torch.full((n_tok, 128), float("nan"), device=d)
        arg = torch.full((n_tok, 128), -7, dtype=torch.int32, device=d)
        st, ab, mv = torch.empty(256, dtype=torch.float64, device=d), torch.empty(256, device=d), torch.empty(256, device=d)
        rm, rv, nb = _bn_buffers(d)
        L.call("gdmae_vfe_max_layer_vis_fwd" + sfx, L.ptr(F["y1"]), N, L.ptr(F["W"]), L.ptr(vis_rows), L.ptr(vis_tok), Nv, n_tok,
               L.ptr(F["gamma"]), L.ptr(F["beta"]), 1e-3, 0.01, L.ptr(rm), L.ptr(rv), L.ptr(nb), L.ptr(st), L.ptr(ab), L.ptr(mv), L.ptr(out),
               L.ptr(arg), L.ptr(ws), L.stream())
        got = _bwd_outputs(N, n_tok, d)
        L.call("gdmae_vfe_max_layer_vis_bwd" + sfx, L.ptr(F["y1"]), N, L.ptr(F["W"]), L.ptr(row_tok), L.ptr(tok_pillar), n_tok, M,
               L.ptr(F["gamma"]), L.ptr(st), L.ptr(ab), L.ptr(out), L.ptr(arg), L.ptr(g_tok), L.ptr(got["gm"]), L.ptr(got["dy1"]),
               L.ptr(got["dg"]), L.ptr(got["db"]), L.ptr(got["dW"]), 0, L.ptr(ws), L.stream())
        got.update(out=out, arg=arg, stats=st, ab=ab, mv=mv, rm=rm, rv=rv, nb=nb)
        runs.append(got)
    torch.cuda.synchronize()
    a, b = runs
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k} differs between two calls of the visible path"
    tp = tok_pillar.long()
    assert torch.equal(a["out"], F["out"][tp]), "out"
    assert torch.equal(a["arg"], F["arg"][tp]), "arg"
    for k in ("stats", "ab", "mv", "rm", "rv", "nb"):
        assert torch.equal(a[k], F[k]), k
    assert torch.equal(a["gm"], want["gm"][tp]), "gm"
    for k in ("dy1", "dW", "dg", "db"):
        assert bool(torch.isfinite(a[k].float()).all()), f"{k}: an element was not written"
        assert torch.equal(a[k], want[k]), k


def _cloud(name, B, Y, X, cells, extra, seed):
    import plan_scenes as PS
    sc = PS.Scene(name, B, Y, X, np.asarray(cells, dtype=np.int64), keep_frac=0.25, extra=extra, seed=seed)
    return sc, PS.points_of(sc), PS.noise_of(sc)


def _clouds():
    import plan_scenes as PS
    one = _cloud("vis_one_frame", 1, 24, 40, PS._rand_cells(31, 1, 24, 40, 90), 400, 31)
    # three frames: 60 pillars, 5 pillars (int(5 * 0.25) = 1 visible), 33 pillars
    c = np.concatenate([PS._rand_cells(32, 1, 16, 24, 60, ends=False), PS._rand_cells(33, 1, 16, 24, 5, ends=False) + [1, 0, 0],
                        PS._rand_cells(34, 1, 16, 24, 33, ends=False) + [2, 0, 0]])
    return [one, _cloud("vis_three_frames", 3, 16, 24, c, 250, 32)]


@pytest.mark.parametrize("which", [0, 1], ids=["one_frame", "three_frames"])
def test_plan_arrays_against_the_cpu(which):
    import plan_scenes as PS
    from gdmae_hip import plan
    sc, pts, noise = _clouds()[which]
    d = torch.device("cuda:0")
    pcr, vs, grid = PS.geometry(sc)
    vox, ep = plan.PlanPrefetch(torch.from_numpy(pts).to(d), pcr, vs, grid, sc.B, *PS.plan_args(), keep_frac=sc.keep_frac,
                                noise=torch.from_numpy(noise).to(d), dec_sources=PS.DEC_SOURCES).finish()
    v = ep.vfe_vis
    assert v is not None and v.n_pillars == vox.M and v.tok_pillar is ep.tok_pillar
    rowpil, mask, tokp = vox.row_pillar.cpu().numpy(), ep.mask.cpu().numpy(), ep.tok_pillar.cpu().numpy()
    visible = mask == 0
    assert np.array_equal(tokp, np.flatnonzero(visible))
    if which == 1:
        frame = vox.voxel_coords[:, 0].cpu().numpy()
        assert int(visible[frame == 1].sum()) == 1, "the middle frame must keep exactly one pillar"
    pil_tok = np.where(visible, np.cumsum(visible) - 1, -1)
    row_tok = pil_tok[rowpil]
    vis_rows = np.flatnonzero(row_tok >= 0)
    assert vox.N > vox.M, "the cloud must have pillars of several points"
    assert v.n_rows == len(vis_rows) and 0 < v.n_rows < vox.N
    assert np.array_equal(v.row_tok.cpu().numpy(), row_tok)
    assert np.array_equal(v.vis_rows.cpu().numpy(), vis_rows)
    assert np.array_equal(v.vis_tok.cpu().numpy(), row_tok[vis_rows])
    assert np.array_equal(v.tok_row_off.cpu().numpy(), np.searchsorted(row_tok[vis_rows], np.arange(len(tokp) + 1)))
    # an unmasked plan has none
    _, ep0 = plan.PlanPrefetch(torch.from_numpy(pts).to(d), pcr, vs, grid, sc.B, *PS.plan_args(), keep_frac=None).finish()
    assert ep0.vfe_vis is None


def test_training_step_switch_on_equals_switch_off():
    import logging
    from gdmae_hip import configs, optim, synth
    from oracle import gdmae_oracle as orc
    from pcdet.models import build_network
    d = torch.device("cuda:0")
    cfg, ds, _ = configs.named_config("A")
    B = 2
    pts = torch.from_numpy(synth.synth_batch(7, B, ds.point_cloud_range, beams=16, azimuths=200, extra=300, features=4)).to(d)
    sd = orc.seeded_state_dict(orc.param_shapes(cfg, 4), seed=7)
    noise = torch.rand(1 << 16, generator=torch.Generator().manual_seed(3)).to(d)
    got = {}
    for on in (True, False):
        net = build_network(cfg, 3, ds, logging.getLogger("test")).to(d).train()
        net.load_state_dict(sd, strict=False)
        net.vfe.visible_only = on
        opt = optim.FlatAdamOneCycle(net, configs.optimization_cfg(), total_steps=10)
        opt.zero_grad()
        vox, ep = net.backbone_3d.prefetch_plan(pts, B, noise=noise).finish()
        assert ep.vfe_vis is not None and 0 < ep.vfe_vis.n_rows < vox.N
        bd = {"points": pts, "batch_size": B, "_gdmae_vox": vox, "_gdmae_plan": ep}
        with torch.autocast("cuda", dtype=torch.bfloat16):
            net.vfe(bd)
            assert (bd["voxel_features"] is None) == on and ("_gdmae_tok_features" in bd) == on
            bd = {"points": pts, "batch_size": B, "_gdmae_vox": vox, "_gdmae_plan": ep}
            ret, _, _ = net(bd)
        ret["loss"].backward()
        torch.cuda.synchronize()
        got[on] = (ret["loss"].detach().clone(), opt.flat_grad.clone(), {k: v.clone() for k, v in net.state_dict().items()})
    assert torch.equal(got[True][0], got[False][0]), (float(got[True][0]), float(got[False][0]))
    assert torch.equal(got[True][1], got[False][1]), int((got[True][1] != got[False][1]).sum())
    assert bool(got[True][1].abs().sum() > 0)
    for k in got[True][2]:                       # running statistics of every BatchNorm
        assert torch.equal(got[True][2][k], got[False][2][k]), k
