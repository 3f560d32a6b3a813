"""The sparse-conv block (csrc/conv_block.hip: gdmae_conv_block_fwd / _bwd) and the kernels under it against the float64 reference of
tests/conv_block_reference.py, at the tile edges.  tests/test_conv_block_reference_cpu.py validates that reference against autograd and
shows that one dropped (row, tap) pair in any case below lands far outside the bounds used here.

Which argument or row count reaches which route (everything is reached through arguments, in one process):

(a) raw kernels, operands for which fp32 accumulation is exact in any order - every difference is a bug
  k_spconv<cin, cout, fp32 rows>          all four channel pairs x bf16 / fp32 rows; forward images on nbr, transposed images on nbr_t, of a
                                          submanifold and a strided scene; n = 1, ROWS - 1, ROWS, ROWS + 1, 2 ROWS + 1 (ROWS = rows per workgroup
                                          = gdmae_spconv_stat_rows): a lone row, a full tile, a tile + 1, more than one workgroup
    missing taps / rows past n            they load source row 0 (NaN here) and are masked; Y's guard rows stay NaN
    statistics epilogue                   gdmae_spconv_stats: the partial rows, summed in float64, are the exact column sums of Y and Y^2
  k_dw_grouped<1> + k_tap_dw_reduce       gdmae_tap_dw, 128 x 128: n = 1, 63, 65 (slices without a valid row), 513 (two chunks per slice),
                                          1025 (three: the odd count ends with an all-zero phase), 4096 (S = 16), 8192 (S = 32); 256 x 128 and
                                          128 x 256 at n = 513 (tile index -> (tm, tn)); G rows in [n, n_pad) and the workspace hold NaN; one
                                          rulebook row names the same source nine times; `out` starts non-zero (the call accumulates)

(b) the block, ten cases (conv_block_reference.CASES)
  case  shape                       reaches
  1     subm 128->128 bf16 x 129    k_spconv 128-row tile + 1; weight-gradient slices 3..7 without a valid row; k_dw_grouped<1>
  2     subm 128->128 fp32 x 65     64-row tile + 1; k_dw_grouped<2> (fp32 rows rounded on load); running statistics NULL; out_f32; g_f32
  3     down 128->256 fp32 x 1400   n_out 934: two chunks per slice; transposed launch 256 -> 128 over nbr_t with n_in != n_out
  4     down 256->256 bf16 x 1200   n_out 1259: three chunks per slice (odd); out_f32; running statistics NULL
  5     subm 256->256 fp32 x 33     32-row tile + 1
  6     subm 256->256 bf16 x 4200   S = 16, five chunks per slice (n_pad 5120)
  7     subm 128->128 bf16 x 8200   S = 32, five chunks per slice (n_pad 10240)
  8     subm 256->256 fp32 x 32769  1025 statistics blocks of 32 rows: the fused epilogue is off, gdmae_bn_fold reads y (nblk > 1024); S = 16, 33 chunks
  9s/9d subm / down 128->128, bf16 = 0: the library route (im2col gather, hipBLASLt GEMMs, split-K weight gradient, permuted weights)
  flags: out_f32, g_f32, running statistics present / NULL are spread over cases 1-8 (each value at least twice); every case but 8 repeats
  the backward with dx == NULL: the weight gradient's reduce then runs as its own launch (k_spconv_dw_reduce) instead of riding on the
  input-gradient launch, and must give the same bits.  dW / dgamma / dbeta start non-zero (accumulation); the scratch starts as 0xFF bytes, so
  rows >= n_out of the padded dy are NaN; y / out / dx carry NaN guard rows.

Staged checks: each stage is judged from the kernel's own saved buffers against float64, by the rounding of that stage alone (formulas at
_check_block).  End to end (dW, dx) the reference chain starts from the kernel's y / out and the bounds are 2 x the values measured on an MI355X
(BOUNDS; the factor 2 covers another legitimate summation order and the rare bf16 boundary flips of dy), under caps that are conditions, not
measurements: dW relative L2 <= 1e-4 and dx worst row <= 2^-7 on the implicit route.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import conv_block_reference as R
from gdmae_hip import lib as L

gpu = pytest.mark.gpu

U24 = 2.0 ** -24
CAP_DW_REL_L2 = 1e-4
CAP_DX_WORST_ROW = 2.0 ** -7
# 2 x the largest value measured on an MI355X over the cases of the route (the measured value and its case in the comment); the kernels
# are bit-repeatable and the inputs seeded, so a rerun prints the same figures (the MEASURE lines of _check_block)
BOUNDS = {
    "implicit_bf16x": {                 # cases 1, 4, 6, 7
        "dW_rel_l2": 5.6e-5,            # 2.760e-05 (case 4)
        "dW_max": 6.9e-4,               # 3.435e-04 (case 4)
        "dx_rel_l2": 1.4e-4,            # 6.934e-05 (case 4)
        "dx_worst_row": 4.4e-3,         # 2.172e-03 (case 7)
    },
    "implicit_f32x": {                  # cases 2, 3, 5, 8
        "dW_rel_l2": 4.3e-5,            # 2.150e-05 (case 3)
        "dW_max": 6.0e-4,               # 2.955e-04 (case 3)
        "dx_rel_l2": 1.5e-4,            # 7.326e-05 (case 3)
        "dx_worst_row": 4.1e-3,         # 2.038e-03 (case 8)
    },
    "library": {                        # cases 9s, 9d (fp32 throughout: no bf16 rounding of dy, so no boundary flips)
        "dW_rel_l2": 3.3e-7,            # 1.619e-07 (case 9s)
        "dW_max": 5.3e-7,               # 2.645e-07 (case 9s)
        "dx_rel_l2": 8.9e-7,            # 4.406e-07 (case 9s)
        "dx_worst_row": 1.4e-6,         # 6.576e-07 (case 9s)
    },
}
# library route (fp32 GEMM of the library): |y - y_ref| <= Y_LIB_COEF * S_abs, 2 x the largest ratio measured against the float64 reference
Y_LIB_COEF = 4.8e-7                     # 2.354e-07 (case 9s; 9d: 1.884e-07)
RAW_SCENES = {"raw_subm": ("subm", 420, 21), "raw_down": ("down", 700, 22), "tap_dw": ("down", 12000, 23, 4)}


def y_bound(route, y_ref, S_abs):
    """one bf16 rounding + fp32 accumulation order (the bound of test_spconv_bias_relu_matches_fp64_formula_at_tile_edges); the fp32
    library GEMM: its measured share of S_abs"""
    if route == "library":
        return Y_LIB_COEF * S_abs
    return 2.0 ** -8 * y_ref.abs() + 2.0 ** -16 * S_abs


def _dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


# ------------------------------------------------------------------------------------------------------------------------------
# (a) raw kernels, bit-exact
# ------------------------------------------------------------------------------------------------------------------------------
_scene_cache = {}


def _raw_scene(name):
    if name not in _scene_cache:
        _scene_cache[name] = R.scene_full(*RAW_SCENES[name])
    return _scene_cache[name]


def _int_weight(cout, cin, gen):
    """W in {-1, 0, 1}, at most 85 non-zeros per output channel over its 9 cin entries AND per input channel over its 9 cout entries (the
    transposed launch sums over those): with |x| <= 3 every partial sum is an integer of magnitude <= 255, exact in fp32 and in bf16"""
    q = 40 if cout <= cin else 20
    W = torch.zeros(cout, 9 * cin)
    for o in range(cout):
        pos = torch.randperm(9 * cin, generator=gen)[:q]
        W[o, pos] = torch.randint(0, 2, (q,), generator=gen).float() * 2 - 1
    W = W.view(cout, 3, 3, cin)
    assert int((W != 0).sum((1, 2, 3)).max()) <= 85 and int((W != 0).sum((0, 1, 2)).max()) <= 85
    return W.contiguous()


@gpu
@pytest.mark.parametrize("src_f32", [0, 1])
@pytest.mark.parametrize("cin,cout", [(128, 128), (128, 256), (256, 128), (256, 256)])
def test_spconv_and_statistics_epilogue_are_exact_on_integer_operands(cin, cout, src_f32):
    from gdmae_hip import packing
    dev = _dev()
    lib = L.load()
    gen = torch.Generator().manual_seed(7 * cin + cout + src_f32)
    W = _int_weight(cout, cin, gen)
    Wdev = W.to(dev)
    packed_fwd, packed_bwd = packing.conv_pack_now(Wdev)
    Wk = W.double().reshape(cout, 9, cin)
    launches = 0
    for sname in ("raw_subm", "raw_down"):
        s = _raw_scene(sname)
        # (launch cin, launch cout, rulebook, source rows, packed images, per-tap matrices (launch cout, launch cin))
        dirs = (("fwd", cin, cout, s["nbr"], s["n_in"], packed_fwd, [Wk[:, k] for k in range(9)]),
                ("transposed", cout, cin, s["nbr_t"], s["n_out"], packed_bwd, [Wk[:, k].t() for k in range(9)]))
        for dname, ci, co, nbr, n_src, packed, mats in dirs:
            rows = lib.gdmae_spconv_stat_rows(ci, co, src_f32)
            assert rows in (32, 64, 128)
            n_max = 2 * rows + 1
            assert len(nbr) >= n_max
            X = torch.randint(-3, 4, (n_src, ci), generator=gen).double()
            Xs = torch.cat([torch.full((1, ci), float("nan"), dtype=torch.float64), X])     # row 0: referenced by no index, loaded by missing taps
            Xd = Xs.to(dev, torch.float32 if src_f32 else torch.bfloat16)
            nb = torch.from_numpy(nbr[:n_max])
            want = torch.zeros(n_max, co, dtype=torch.float64)
            for k in range(9):
                want += (X[nb[:, k].clamp_min(0)] * (nb[:, k] >= 0)[:, None]) @ mats[k].t()
            assert float(want.abs().max()) <= 255
            nbd_all = torch.where(nb >= 0, nb + 1, nb).int().to(dev)
            for n in (1, rows - 1, rows, rows + 1, 2 * rows + 1):
                nbd = nbd_all[:n].contiguous()
                nblk = (n + rows - 1) // rows
                for stats in (0, 1):
                    Y = torch.full((n + 8, co), float("nan"), dtype=torch.bfloat16, device=dev)
                    part = torch.full((nblk + 1, 2, co), float("nan"), device=dev)
                    if stats:
                        L.call("gdmae_spconv_stats", L.ptr(Xd), src_f32, L.ptr(nbd), L.ptr(packed), n, ci, co, L.ptr(Y), L.ptr(part), L.stream())
                    else:
                        L.call("gdmae_spconv", L.ptr(Xd), src_f32, L.ptr(nbd), L.ptr(packed), n, ci, co, L.ptr(Y), 0, L.stream())
                    torch.cuda.synchronize()
                    launches += 1
                    what = f"{sname} {dname} {ci}->{co} f32={src_f32} n={n} stats={stats}"
                    assert torch.equal(Y[:n].double().cpu(), want[:n]), what
                    assert torch.isnan(Y[n:].float()).all(), what + ": guard rows written"
                    if stats:
                        p = part[:nblk].double().sum(0).cpu()
                        assert torch.equal(p[0], want[:n].sum(0)) and torch.equal(p[1], (want[:n] ** 2).sum(0)), what + ": statistics partials"
                        assert torch.isnan(part[nblk:]).all(), what + ": partial rows past the last workgroup written"
                    else:
                        assert torch.isnan(part).all()
    assert launches == 2 * 2 * 5 * 2


TAP_DW_CASES = [(128, 128, 1, 8, 1), (128, 128, 63, 8, 1), (128, 128, 65, 8, 1), (128, 128, 513, 8, 2), (128, 128, 1025, 8, 3),
                (128, 128, 4096, 16, 4), (128, 128, 8192, 32, 4), (256, 128, 513, 8, 2), (128, 256, 513, 8, 2)]


@gpu
@pytest.mark.parametrize("M,N,n,S_want,chunks_want", TAP_DW_CASES)
def test_tap_dw_gathered_weight_gradient_is_exact_on_integer_operands(M, N, n, S_want, chunks_want):
    dev = _dev()
    lib = L.load()
    s = _raw_scene("tap_dw")
    assert s["n_out"] >= 8192
    # the slice grid the test believes it hits (gd_dw_pick: S doubles from 8 while tiles x 2 S <= 640 workgroups and a slice keeps >= 4 chunks)
    n_pad = lib.gdmae_tap_dw_rows(n, M, N)
    ws_bytes = lib.gdmae_tap_dw_workspace_bytes(n, M, N)
    S = ws_bytes // (9 * M * N * 4)
    assert S == S_want and n_pad % (S * 64) == 0 and n_pad // (S * 64) == chunks_want and n_pad >= n
    if n < 8 * 64:
        assert (S - 1) * (n_pad // S) >= n                                  # the last slice holds no valid row
    gen = torch.Generator().manual_seed(M + 3 * N + n)
    n_src = s["n_in"]
    nbr = s["nbr"][:n].copy()
    r = n // 2
    nbr[r, :] = nbr[r][nbr[r] >= 0][0]                                    # one row whose nine taps name the same source
    nb = torch.from_numpy(nbr)
    G = torch.randint(-2, 3, (n, M), generator=gen).double()
    X = torch.randint(-2, 3, (n_src, N), generator=gen).double()
    out0 = torch.randint(-3, 4, (9, N, M), generator=gen).double()
    want = out0.clone()
    for k in range(9):
        want[k] += (X[nb[:, k].clamp_min(0)] * (nb[:, k] >= 0)[:, None]).t() @ G
    assert float(want.abs().max()) < 2 ** 24
    Gd = torch.full((n_pad, M), float("nan"), dtype=torch.bfloat16, device=dev)
    Gd[:n] = G.to(dev, torch.bfloat16)
    Xd = torch.cat([torch.full((1, N), float("nan"), dtype=torch.float64), X]).to(dev, torch.bfloat16)
    nbd = torch.where(nb >= 0, nb + 1, nb).int().to(dev)
    out = out0.float().to(dev)
    ws = torch.full((ws_bytes // 4,), float("nan"), device=dev)
    L.call("gdmae_tap_dw", L.ptr(Gd), n, n_pad, M, L.ptr(Xd), L.ptr(nbd), N, L.ptr(out), M, 0, L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    assert torch.equal(out.double().cpu(), want)


# ------------------------------------------------------------------------------------------------------------------------------
# (b) the block
# ------------------------------------------------------------------------------------------------------------------------------
def _run_block(I, dev, with_dx):
    """One forward + backward through the C entry points on fresh buffers; -> dict of the buffers the block wrote."""
    from gdmae_hip import packing
    c, s = I["case"], I["scene"]
    lib = L.load()
    n_in, n_out, cin, cout = s["n_in"], s["n_out"], c["cin"], c["cout"]
    cdt = torch.bfloat16 if c["bf16"] else torch.float32
    nan = float("nan")
    x = I["x"].to(dev, torch.float32 if (c["x_f32"] or not c["bf16"]) else torch.bfloat16).contiguous()
    Wdev = I["W"].to(dev).contiguous()
    wc = Wdev.to(cdt).contiguous()
    nbr = torch.from_numpy(s["nbr"]).int().to(dev).contiguous()
    nbr_t = torch.from_numpy(s["nbr_t"]).int().to(dev).contiguous()
    gamma, beta = I["gamma"].to(dev), I["beta"].to(dev)
    g = I["g"].to(dev, torch.float32 if (c["g_f32"] or not c["bf16"]) else torch.bfloat16).contiguous()
    out_fp32 = bool(c["out_f32"]) or not c["bf16"]
    B = {"y": torch.full((n_out + 8, cout), nan, dtype=cdt, device=dev),
         "out": torch.full((n_out + 8, cout), nan, dtype=torch.float32 if out_fp32 else cdt, device=dev),
         "dx": torch.full((n_in + 8, cin), nan, dtype=cdt, device=dev) if with_dx else None,
         "stats": torch.full((2 * cout,), nan, dtype=torch.float64, device=dev),
         "abmv": torch.full((4 * cout,), nan, device=dev),
         "dW": I["dW0"].to(dev).contiguous(), "dgamma": I["dgamma0"].to(dev), "dbeta": I["dbeta0"].to(dev),
         "rm": I["rm0"].to(dev), "rv": I["rv0"].to(dev), "nb": torch.full((1,), 7, dtype=torch.int64, device=dev)}
    a = L.ConvBlockArgs()
    a.n_in, a.n_out, a.cin, a.cout = n_in, n_out, cin, cout
    a.bf16, a.x_f32, a.g_f32, a.out_f32 = c["bf16"], c["x_f32"], c["g_f32"], c["out_f32"]
    a.eps, a.momentum = R.EPS, R.MOMENTUM
    a.x, a.nbr, a.nbr_t, a.W, a.gamma, a.beta = L.ptr(x), L.ptr(nbr), L.ptr(nbr_t), L.ptr(wc), L.ptr(gamma), L.ptr(beta)
    if c["running"]:
        a.running_mean, a.running_var, a.num_batches = L.ptr(B["rm"]), L.ptr(B["rv"]), L.ptr(B["nb"])
    keep = [x, Wdev, wc, nbr, nbr_t, gamma, beta, g]
    if c["bf16"]:
        packed = packing.conv_pack_now(Wdev)
        a.packed_fwd, a.packed_bwd = L.ptr(packed[0]), L.ptr(packed[1])
        keep.append(packed)
    else:
        cols = torch.full((n_out, 9 * cin), nan, dtype=cdt, device=dev)
        a.cols = L.ptr(cols)
        keep.append(cols)
    nbytes = lib.gdmae_conv_block_scratch_bytes(n_in, n_out, cin, cout, c["bf16"])
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    a.y, a.out, a.stats, a.ab, a.mv = L.ptr(B["y"]), L.ptr(B["out"]), L.ptr(B["stats"]), L.ptr(B["abmv"]), L.ptr(B["abmv"][2 * cout:])
    a.scratch = L.ptr(scratch)
    L.call("gdmae_conv_block_fwd", C.byref(a), L.stream())
    torch.cuda.synchronize()
    scratch.fill_(0xFF)
    a.g, a.dx = L.ptr(g), (L.ptr(B["dx"]) if with_dx else None)
    a.dW, a.dgamma, a.dbeta = L.ptr(B["dW"]), L.ptr(B["dgamma"]), L.ptr(B["dbeta"])
    L.call("gdmae_conv_block_bwd", C.byref(a), L.stream())
    torch.cuda.synchronize()
    del keep
    return B


# (row slices, 64-row chunks per slice) of the weight-gradient launch per implicit case
DW_GRID = {"1": (8, 1), "2": (8, 1), "3": (8, 2), "4": (8, 3), "5": (8, 1), "6": (16, 5), "7": (32, 5), "8": (16, 33)}


def _stat_rows(c, n, lib):
    """largest row count one fp32 statistics partial covers, and whether the fused epilogue produced it"""
    if c["bf16"]:
        rows = lib.gdmae_spconv_stat_rows(c["cin"], c["cout"], c["x_f32"])
        if (n + rows - 1) // rows <= 1024:
            return rows, True
    nblk = min(512, max(1, n // 64))                # gdmae_bn_fold (csrc/segment.hip), n < 2^20
    return (n + nblk - 1) // nblk, False


def _check_block(name):
    """Stages, each from the kernel's own buffers (u = 2^-24, n = n_out):
      y        |y - y_ref| <= 2^-8 |y_ref| + 2^-16 S_abs                       (library route: Y_LIB_COEF S_abs)
      stats    mean within R u mean|y|, E[y^2] within R u E[y^2] of the float64 statistics of the kernel's y, both carried to rstd
      ab, mv   one fp32 rounding of gamma rstd, beta - a mean, mean, var from the kernel's stats
      running  torch's update r (1 - m) + m v (unbiased variance), 4 u relative; num_batches + 1
      out      |out - relu(a y + b)| <= 2^-8 |ref| + 2^-22 (|a y| + |b|)       (fp32 out: the second term)
      dgamma, dbeta   R_b u sum|term| per column + one fp32 rounding (+ the rounding of the accumulation)
    then dW and dx against the reference chain started from the kernel's y / out (BOUNDS)."""
    dev = _dev()
    lib = L.load()
    I = R.make_inputs(name)
    c, s = I["case"], I["scene"]
    n_in, n_out, cin, cout = s["n_in"], s["n_out"], c["cin"], c["cout"]
    route = R.route(c)
    fails = []
    if c["bf16"]:
        # the slice grid of the weight-gradient launch this case claims (conv_block.hip picks it with the rule gdmae_tap_dw reports)
        S = lib.gdmae_tap_dw_workspace_bytes(n_out, cout, cin) // (9 * cout * cin * 4)
        chunks = lib.gdmae_tap_dw_rows(n_out, cout, cin) // (S * 64)
        assert (S, chunks) == DW_GRID[name], (name, n_out, S, chunks)

    def check(ok, msg):
        if not bool(ok):
            fails.append(msg)

    K = _run_block(I, dev, True)
    K2 = _run_block(I, dev, True)
    for k, v in K.items():
        check(torch.equal(_bits(v), _bits(K2[k])), f"{k}: two identical runs differ")
    del K2
    if name != "8":
        K3 = _run_block(I, dev, False)
        for k in ("dW", "dgamma", "dbeta", "y", "out"):
            check(torch.equal(_bits(K[k]), _bits(K3[k])), f"{k}: dx == NULL changes it (own reduce launch vs rider)")
        del K3
    # guard rows, finiteness
    for k, n in (("y", n_out), ("out", n_out), ("dx", n_in)):
        check(torch.isnan(K[k][n:].float()).all(), f"{k}: guard rows written")
        check(torch.isfinite(K[k][:n].float()).all(), f"{k}: not finite")
    for k in ("stats", "abmv", "dW", "dgamma", "dbeta", "rm", "rv"):
        check(torch.isfinite(K[k]).all(), f"{k}: not finite")

    rdev = dev if n_out >= 4000 else torch.device("cpu")          # the float64 reference of the large cases runs as plain torch on the device
    to = lambda t: t.to(rdev)                                       # noqa: E731
    yk, outk = to(K["y"][:n_out]).double(), to(K["out"][:n_out]).double()
    r = R.reference(to(I["x"]), to(I["W"]), to(I["gamma"]), to(I["beta"]), R.EPS, s["nbr"], to(I["g"]), y=yk, out=outk,
                    out_f32=bool(c["out_f32"]), rounding=bool(c["bf16"]))
    fig = {}
    # ---- y
    dev_abs = (yk - r["y_exact"]).abs()
    ratio = float((dev_abs / (y_bound(route, r["y_exact"], r["S_abs"]) + 1e-300)).max())
    fig["y_ratio"] = ratio
    fig["y_over_S_abs"] = float((dev_abs / (r["S_abs"] + 1e-300)).max())
    check(ratio <= 1.0, f"y: {ratio:.3f} x its bound")
    # ---- statistics of the kernel's y
    Rs, fused = _stat_rows(c, n_out, lib)
    assert fused == (name not in ("8", "9s", "9d"))
    mean64, e2 = yk.mean(0), (yk * yk).mean(0)
    dmean, de2 = Rs * U24 * yk.abs().mean(0) + 1e-14 * mean64.abs(), Rs * U24 * e2 * (1 + 1e-9)
    var64 = (e2 - mean64 * mean64).clamp_min(0)
    dvar = de2 + 2 * mean64.abs() * dmean + dmean * dmean
    rstd64 = (var64 + R.EPS) ** -0.5
    drstd = ((var64 - dvar).clamp_min(0) + R.EPS) ** -0.5 - rstd64 + 1e-14 * rstd64
    st = to(K["stats"])
    mean_k, rstd_k = st[:cout], st[cout:]
    fig["mean_ratio"] = float(((mean_k - mean64).abs() / dmean).max())
    fig["rstd_ratio"] = float(((rstd_k - rstd64).abs() / drstd).max())
    check(fig["mean_ratio"] <= 1.0, f"mean: {fig['mean_ratio']:.3f} x its bound (R = {Rs})")
    check(fig["rstd_ratio"] <= 1.0, f"rstd: {fig['rstd_ratio']:.3f} x its bound (R = {Rs})")
    # ---- ab, mv: one fp32 rounding of the float64 values from the kernel's stats
    gam, bet = to(I["gamma"]).double(), to(I["beta"]).double()
    abmv = to(K["abmv"]).double()
    a64 = gam * rstd_k
    b64 = bet - a64 * mean_k
    var_s = rstd_k ** -2 - R.EPS
    check(((abmv[:cout] - a64).abs() <= U24 * a64.abs()).all(), "ab: a")
    check(((abmv[cout:2 * cout] - b64).abs() <= U24 * b64.abs() + 2.0 ** -50 * (bet.abs() + (a64 * mean_k).abs())).all(), "ab: b")
    check(((abmv[2 * cout:3 * cout] - mean_k).abs() <= U24 * mean_k.abs()).all(), "mv: mean")
    check(((abmv[3 * cout:] - var_s).abs() <= U24 * var_s.abs() + 2.0 ** -48 * (var_s + R.EPS)).all(), "mv: var")
    # ---- running statistics
    if c["running"]:
        m = float(np.float32(R.MOMENTUM))
        rm_ref = to(I["rm0"]).double() * (1 - m) + m * mean_k
        rv_ref = to(I["rv0"]).double() * (1 - m) + m * var_s * (n_out / max(n_out - 1.0, 1.0))
        check(((to(K["rm"]).double() - rm_ref).abs() <= 4 * U24 * rm_ref.abs()).all(), "running_mean")
        check(((to(K["rv"]).double() - rv_ref).abs() <= 4 * U24 * rv_ref.abs()).all(), "running_var")
        check(int(K["nb"]) == 8, "num_batches")
    else:
        check(torch.equal(K["rm"].cpu(), I["rm0"]) and torch.equal(K["rv"].cpu(), I["rv0"]) and int(K["nb"]) == 7, "running statistics touched")
    # ---- out from the kernel's y and ab
    ak, bk = abmv[:cout], abmv[cout:2 * cout]
    ref_out = torch.relu(ak * yk + bk)
    out_fp32 = bool(c["out_f32"]) or not c["bf16"]
    ob = (0.0 if out_fp32 else 2.0 ** -8) * ref_out + 2.0 ** -22 * ((ak * yk).abs() + bk.abs())
    fig["out_ratio"] = float(((outk - ref_out).abs() / ob).max())
    check(fig["out_ratio"] <= 1.0, f"out: {fig['out_ratio']:.3f} x its bound")
    # ---- dgamma, dbeta from the kernel's y, stats, out and g
    gk = to(I["g"]).double()
    dh = gk * (outk > 0)
    s0, s1 = dh.sum(0), (dh * yk).sum(0)
    Rb = math.ceil(n_out / lib.gdmae_rows_bwd_stats_rows(n_out))
    e0, e1 = Rb * U24 * dh.abs().sum(0), Rb * U24 * (dh * yk).abs().sum(0)
    dg_ref = (s1 - s0 * mean_k) * rstd_k
    db_tot, dg_tot = to(I["dbeta0"]).double() + s0, to(I["dgamma0"]).double() + dg_ref
    db_b = e0 + U24 * s0.abs() + U24 * db_tot.abs()
    dg_b = rstd_k * (e1 + mean_k.abs() * e0) + U24 * dg_ref.abs() + U24 * dg_tot.abs()
    fig["dbeta_ratio"] = float(((to(K["dbeta"]).double() - db_tot).abs() / db_b).max())
    fig["dgamma_ratio"] = float(((to(K["dgamma"]).double() - dg_tot).abs() / dg_b).max())
    check(fig["dbeta_ratio"] <= 1.0, f"dbeta: {fig['dbeta_ratio']:.3f} x its bound (R_b = {Rb})")
    check(fig["dgamma_ratio"] <= 1.0, f"dgamma: {fig['dgamma_ratio']:.3f} x its bound (R_b = {Rb})")
    # ---- end to end from the kernel's y / out
    bound = BOUNDS[route]
    dW_err = to(K["dW"]).double() - to(I["dW0"]).double() - r["dW"]
    fig["dW_rel_l2"] = float(dW_err.norm() / r["dW"].norm())
    fig["dW_max"] = float(dW_err.abs().max() / r["dW"].abs().max())
    fig["dx_rel_l2"], fig["dx_worst_row"] = R.row_errors(to(K["dx"][:n_in]).double(), r["dx"])
    print(f"MEASURE case {name} route {route} n_in {n_in} n_out {n_out} fused_stats {int(fused)} " + " ".join(f"{k} {v:.3e}" for k, v in fig.items()))
    for k in ("dW_rel_l2", "dW_max", "dx_rel_l2", "dx_worst_row"):
        check(fig[k] <= bound[k], f"{k}: {fig[k]:.3e} > {bound[k]:.3e}")
    assert not fails, f"case {name}: " + "; ".join(fails)


@gpu
@pytest.mark.parametrize("name", list(R.CASES))
def test_conv_block_stages_and_gradients_match_fp64_reference(name):
    _check_block(name)
