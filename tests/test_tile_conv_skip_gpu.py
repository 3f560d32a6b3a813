"""GPU: the leading-phase skip of the decoder's tile convolution (csrc/conv_tiles.hip).

* tile classes and the class-sorted pairing order of BOTH builders - the one-shot entry gdmae_decoder_tiles_classes and the geometry
  plan's (PlanPrefetch -> gdmae_geometry_plan, "dec.tile_class" / "dec.tile_order") - exactly against tests/tile_classes_reference.py
  (itself checked by tests/test_tile_classes_reference_cpu.py);
* gdmae_conv3x3_tiles_fwd_skip with the classes / order / pre-accumulators against the SAME call without them (= gdmae_conv3x3_tiles_fwd,
  which the existing tests hold to its fp64 bound): Yc, the per-tile statistics partials, stats, ab, mv and the running statistics
  bit for bit, twice;
* the pre-accumulators against an fp64 sum of the same fp16 operands, to a small multiple of the round-off that sum shows when it is
  accumulated in fp32.

Every case first asserts, from the reference, that the classes it claims to cover are there."""
import numpy as np
import pytest
import torch

import tile_classes_reference as R

pytestmark = pytest.mark.gpu

SCENES = {
    "center_class2": lambda: R.scene_center(2),
    "center_class1": lambda: R.scene_center(1),
    "center_class0": lambda: R.scene_center(0),
    "mixed": R.scene_mixed,
    "all_class0": R.scene_all_class0,
    "k2": R.scene_k2,
}


def _dev():
    return torch.device("cuda:0")


def _i(t):
    return t.detach().cpu().numpy().astype(np.int64)


def _leads(r):
    c = r["tile_class"][r["tile_order"]]
    return [int(c[i:i + 2].min()) for i in range(0, len(c), 2)], [len(set(c[i:i + 2].tolist())) > 1 for i in range(0, len(c), 2)]


def _assert_covers(name, r):
    """what each scene is there for, from the reference"""
    cls = set(r["tile_class"].tolist())
    ld, mixed = _leads(r)
    TWc = 3
    if name.startswith("center"):
        want = int(name[-1])
        assert int(r["tile_class"][r["tile_slot"][1 * TWc + 1]]) == want and cls == {0, want}
    elif name == "mixed":
        assert cls == {0, 1, 2} and r["n_act"] % 2 == 1 and {0, 1, 2} <= set(ld) and any(mixed)
    elif name == "all_class0":
        assert cls == {0} and r["n_act"] > 2 and np.array_equal(r["tile_order"], np.arange(r["n_act"]))
    elif name == "k2":
        assert cls == {0, 1} and 1 in ld


def _tiles_one_shot(maps, strides, B, H, W):
    from gdmae_hip import lib as L
    lib, d = L.load(), _dev()
    nt = B * ((H + 7) // 8) * ((W + 7) // 8)
    mapsd = [torch.from_numpy(m.reshape(-1).astype(np.int32)).to(d) for m in maps]
    out = {k: torch.full((nt,), -7, dtype=torch.int32, device=d) for k in ("tile_slot", "tile_list", "tile_class", "tile_order")}
    nact = torch.zeros(1, dtype=torch.int32, device=d)
    ws = torch.empty(lib.gdmae_decoder_tiles_workspace_bytes(B, H, W), dtype=torch.uint8, device=d)
    L.call("gdmae_decoder_tiles_classes", L.host_ptrs(mapsd), L.host_i32(list(strides)), len(maps), B, H, W, L.ptr(out["tile_slot"]),
           L.ptr(out["tile_list"]), L.ptr(out["tile_class"]), L.ptr(out["tile_order"]), L.ptr(nact), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    return mapsd, out, int(nact.item())


def _assert_tiles(got, n_act, r, what):
    assert n_act == r["n_act"], what
    assert np.array_equal(_i(got["tile_slot"]), r["tile_slot"]), what
    for k in ("tile_list", "tile_class", "tile_order"):
        assert np.array_equal(_i(got[k])[:n_act], r[k]), (what, k, _i(got[k])[:n_act], r[k])


@pytest.mark.parametrize("name", list(SCENES))
def test_skip_is_bit_equal_to_the_full_chain(name):
    from gdmae_hip import lib as L
    lib, d = L.load(), _dev()
    maps, strides, B, H, W = SCENES[name]()
    k = len(maps)
    r = R.tile_classes(maps, strides, B, H, W)
    _assert_covers(name, r)
    # ---- the one-shot builder, exactly (before anything is indexed through its order)
    mapsd, T, n_act = _tiles_one_shot(maps, strides, B, H, W)
    _assert_tiles(T, n_act, r, name)
    # the old entry still hands out the same slots
    slot0, list0 = torch.empty_like(T["tile_slot"]), torch.empty_like(T["tile_list"])
    nact0 = torch.zeros(1, dtype=torch.int32, device=d)
    ws = torch.empty(lib.gdmae_decoder_tiles_workspace_bytes(B, H, W), dtype=torch.uint8, device=d)
    L.call("gdmae_decoder_tiles", L.host_ptrs(mapsd), L.host_i32(list(strides)), k, B, H, W, L.ptr(slot0), L.ptr(list0), L.ptr(nact0), L.ptr(ws),
           L.stream())
    assert int(nact0.item()) == n_act and torch.equal(slot0, T["tile_slot"]) and torch.equal(list0[:n_act], T["tile_list"][:n_act])
    # ---- operands: deconvolution rows, folded BatchNorm scale / shift with negative shifts (background 0), weights of both signs
    g = torch.Generator().manual_seed(100 + len(name))
    Ps, a_l, b_l = [], [], []
    for m, s in zip(maps, strides):
        n_tok = int((m >= 0).sum())
        Ps.append((torch.randn(max(n_tok, 1) * s * s, 128, generator=g) * 1.5).bfloat16().to(d))
        a_l.append((torch.rand(128, generator=g) + 0.5).to(d))
        b = torch.randn(128, generator=g) * 0.5
        assert int((b < 0).sum()) > 16 and int((b > 0).sum()) > 16
        b_l.append(b.to(d))
    w = (torch.randn(128, 128 * k, 3, 3, generator=g) * 0.05).to(d).contiguous()
    gamma, beta = (torch.rand(128, generator=g) + 0.5).to(d), torch.randn(128, generator=g).to(d)
    Wp = torch.empty(lib.gdmae_conv3x3_tiles_packed_bytes(k), dtype=torch.uint8, device=d)
    bgz = torch.empty(128 * k, dtype=torch.bfloat16, device=d)
    ybg = torch.empty(9, 128, dtype=torch.bfloat16, device=d)
    pre = torch.full((max(k - 1, 1), 128), float("nan"), dtype=torch.float32, device=d)
    L.call("gdmae_conv3x3_tiles_pack_pre", L.ptr(w), 128, 128 * k, L.host_ptrs(b_l), k, L.ptr(Wp), L.ptr(bgz), L.ptr(ybg), L.ptr(pre), L.stream())
    # the plain pack leaves the same weight image and constants
    Wp0, bgz0, ybg0 = torch.empty_like(Wp), torch.empty_like(bgz), torch.empty_like(ybg)
    L.call("gdmae_conv3x3_tiles_pack", L.ptr(w), 128, 128 * k, L.host_ptrs(b_l), k, L.ptr(Wp0), L.ptr(bgz0), L.ptr(ybg0), L.stream())
    assert torch.equal(Wp0, Wp) and torch.equal(bgz0.view(torch.int16), bgz.view(torch.int16)) and torch.equal(ybg0.view(torch.int16), ybg.view(torch.int16))

    def run(skip):
        Yc = torch.full((max(n_act, 1) * 64, 128), float("nan"), dtype=torch.bfloat16, device=d)
        stats = torch.empty(256, dtype=torch.float64, device=d)
        ab, mv = torch.empty(256, dtype=torch.float32, device=d), torch.empty(256, dtype=torch.float32, device=d)
        rm, rv, nb = torch.zeros(128, device=d), torch.ones(128, device=d), torch.zeros(1, dtype=torch.int64, device=d)
        ws2 = torch.full((lib.gdmae_conv3x3_tiles_workspace_bytes(n_act),), 0xFF, dtype=torch.uint8, device=d)
        extra = (L.ptr(T["tile_class"]), L.ptr(T["tile_order"]), L.ptr(pre)) if skip else (None, None, None)
        L.call("gdmae_conv3x3_tiles_fwd_skip", L.host_ptrs(Ps), L.host_ptrs(mapsd), L.host_ptrs(a_l), L.host_ptrs(b_l), L.host_i32(list(strides)), k,
               L.ptr(Wp), L.ptr(ybg), L.ptr(T["tile_list"]), n_act, B, H, W, L.ptr(Yc), L.ptr(gamma), L.ptr(beta), 1e-3, 0.01, L.ptr(rm),
               L.ptr(rv), L.ptr(nb), L.ptr(stats), L.ptr(ab), L.ptr(mv), *extra, L.ptr(ws2), L.stream())
        torch.cuda.synchronize()
        part = ws2[:n_act * 256 * 4].view(torch.int32)                 # the per-tile statistics partials lead the workspace
        return dict(Yc=Yc.view(torch.int16), part=part, stats=stats.view(torch.int64), ab=ab.view(torch.int32), mv=mv.view(torch.int32),
                    rm=rm.view(torch.int32), rv=rv.view(torch.int32))

    off, on, on2 = run(False), run(True), run(True)
    assert not torch.isnan(off["Yc"].view(torch.bfloat16).float()).any()
    for key in off:
        assert torch.equal(off[key], on[key]), (name, key, int((off[key] != on[key]).sum()))
        assert torch.equal(on[key], on2[key]), (name, key, "two runs differ")
    # the old entry point is the call without the three pointers
    Yc = torch.full((max(n_act, 1) * 64, 128), float("nan"), dtype=torch.bfloat16, device=d)
    stats = torch.empty(256, dtype=torch.float64, device=d)
    ab, mv = torch.empty(256, dtype=torch.float32, device=d), torch.empty(256, dtype=torch.float32, device=d)
    ws2 = torch.empty(lib.gdmae_conv3x3_tiles_workspace_bytes(n_act), dtype=torch.uint8, device=d)
    L.call("gdmae_conv3x3_tiles_fwd", L.host_ptrs(Ps), L.host_ptrs(mapsd), L.host_ptrs(a_l), L.host_ptrs(b_l), L.host_i32(list(strides)), k,
           L.ptr(Wp), L.ptr(ybg), L.ptr(T["tile_list"]), n_act, B, H, W, L.ptr(Yc), L.ptr(gamma), L.ptr(beta), 1e-3, 0.01, None, None, None,
           L.ptr(stats), L.ptr(ab), L.ptr(mv), L.ptr(ws2), L.stream())
    torch.cuda.synchronize()
    assert torch.equal(Yc.view(torch.int16), off["Yc"]) and torch.equal(mv.view(torch.int32), off["mv"])


def test_pre_accumulators_against_fp64():
    """pre[j][c] = sum over the stages g <= j, the 9 taps and the 128 channels of f16(W[c][g, ci][tap]) * f16(relu(b_g[ci])).  The products
    of two fp16 values are exact in fp32, so the only error is the accumulation's.  Bound: 4 x the largest error the same sum shows when it
    is accumulated term by term in fp32 (the matrix cores add 16 products at a time to the fp32 accumulator, so the kernel's own error is
    expected below that of 2304 single additions; the factor covers a channel whose running sum happens to round well in the emulation)."""
    from gdmae_hip import lib as L
    lib, d = L.load(), _dev()
    k = 3
    g = torch.Generator().manual_seed(5)
    w = torch.randn(128, 128 * k, 3, 3, generator=g) * 0.05
    b_l = [torch.randn(128, generator=g) * 0.5 for _ in range(k)]
    Wp = torch.empty(lib.gdmae_conv3x3_tiles_packed_bytes(k), dtype=torch.uint8, device=d)
    bgz, ybg = torch.empty(128 * k, dtype=torch.bfloat16, device=d), torch.empty(9, 128, dtype=torch.bfloat16, device=d)
    bd = [b.to(d) for b in b_l]
    pre = torch.full((k - 1, 128), float("nan"), dtype=torch.float32, device=d)
    L.call("gdmae_conv3x3_tiles_pack_pre", L.ptr(w.to(d).contiguous()), 128, 128 * k, L.host_ptrs(bd), k, L.ptr(Wp), L.ptr(bgz), L.ptr(ybg),
           L.ptr(pre), L.stream())
    torch.cuda.synchronize()
    got = pre.cpu().double().numpy()
    wh = w.half().double().numpy()                                     # (128, 384, 3, 3)
    ref = np.zeros((k - 1, 128))
    emu = np.zeros((k - 1, 128), dtype=np.float32)
    acc64, acc32 = np.zeros(128), np.zeros(128, dtype=np.float32)
    for j in range(k - 1):
        bg = torch.relu(b_l[j]).half().double().numpy()
        for tap in range(9):                                           # the kernel's order: tap, then channel
            for ci in range(128):
                p = wh[:, j * 128 + ci, tap // 3, tap % 3] * bg[ci]
                acc64 = acc64 + p
                acc32 = (acc32 + p.astype(np.float32)).astype(np.float32)
        ref[j], emu[j] = acc64, acc32
    err_kernel = float(np.abs(got - ref).max())
    err_emulated = float(np.abs(emu.astype(np.float64) - ref).max())
    print(f"pre-accumulators: max |kernel - fp64| {err_kernel:.3e}, max |fp32 emulation - fp64| {err_emulated:.3e}, max |ref| {np.abs(ref).max():.3e}")
    assert err_emulated > 0.0
    assert err_kernel <= 4.0 * err_emulated, (err_kernel, err_emulated)


def _plan_scene(name):
    import plan_scenes as PS
    if name == "populations":
        return PS.SCENES[name]
    # isolated pillars well inside a 64 x 64 map: the stage-1 / stage-2 token sets (k3 s2 p1 down-sampling) reach one / two rings further
    # than the pillars, so the tiles around a pillar's own are class 1 and class 2
    cells = np.asarray([(0, 30, 30), (1, 20, 43), (1, 44, 18)], dtype=np.int64)
    return PS.Scene("isolated_64", 2, 64, 64, cells, keep_frac=None, seed=31)


@pytest.mark.parametrize("name,want", [("isolated_64", {0, 1, 2}), ("populations", {0, 2})])
def test_plan_builder_classes_and_order(name, want):
    """The geometry plan's builder (gd_decoder_tiles_lb + the order launch) against the reference evaluated on the plan's OWN stage maps."""
    import plan_scenes as PS
    from gdmae_hip import plan
    sc = _plan_scene(name)
    pts, noise = torch.from_numpy(PS.points_of(sc)).to(_dev()), torch.from_numpy(PS.noise_of(sc)).to(_dev())
    pcr, vs, grid = PS.geometry(sc)
    pf = plan.PlanPrefetch(pts, pcr, vs, grid, sc.B, *PS.plan_args(), keep_frac=sc.keep_frac, noise=None, dec_sources=PS.DEC_SOURCES)
    vox, ep = pf.finish()
    torch.cuda.synchronize()
    dt = ep.dec_tiles
    assert dt is not None and dt.tile_class is not None and dt.tile_order is not None
    st = [ep.stages[i] for i in PS.DEC_SOURCES]
    maps = [_i(s.map).reshape(s.B, s.Y, s.X) for s in st]
    strides = [sc.Y // s.Y for s in st]
    r = R.tile_classes(maps, strides, sc.B, sc.Y, sc.X)
    assert set(r["tile_class"].tolist()) == want, np.bincount(r["tile_class"], minlength=3)
    got = dict(tile_slot=dt.tile_slot, tile_list=dt.tile_list, tile_class=dt.tile_class, tile_order=dt.tile_order)
    _assert_tiles(got, dt.n_act, r, name)
    # the per-operator builder of the same plan (plan.encoder_plan -> the one-shot entry) agrees
    ep2 = plan.encoder_plan(plan.voxelize(pts, pcr, vs, grid, sc.B), *PS.plan_args(), keep_frac=None, noise=None, dec_sources=PS.DEC_SOURCES)
    d2 = ep2.dec_tiles
    _assert_tiles(dict(tile_slot=d2.tile_slot, tile_list=d2.tile_list, tile_class=d2.tile_class, tile_order=d2.tile_order), d2.n_act, r, name)
