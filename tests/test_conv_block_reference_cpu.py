"""The conv-block reference (tests/conv_block_reference.py) is itself checked here, without a GPU, before tests/test_conv_block_gpu.py
judges a kernel by it:

* with the roundings switched off it equals float64 autograd through the oracle's convolutions + F.batch_norm(training) + relu, output
  and all four gradients, to 1e-12; the strided scene's output order is the oracle's;
* every crafted scene holds the features its docstring lists (read off the rulebook);
* the GPU test has the power it claims: dropping ONE (row, tap) pair from the rulebook of any block case moves dW, the dx worst row and
  the affected y row far past the bounds the GPU test applies (>= 10 x the caps), computed as the rank-one updates they are on an fp32
  emulation of the block's rounding chain;
* the caps on the measured bounds hold.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_block_reference as R
import test_conv_block_gpu as G
from oracle import thirdparty as tp


@pytest.mark.parametrize("kind,n,seed", [("subm", 129, 1), ("down", 150, 2), ("subm", 500, 3)])
def test_reference_without_rounding_equals_float64_autograd(kind, n, seed):
    s = R.scene_full(kind, n, seed)
    cin, cout, eps = 5, 7, 1e-3
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(s["n_in"], cin, generator=gen, dtype=torch.float64).requires_grad_()
    W = (0.3 * torch.randn(cout, 3, 3, cin, generator=gen, dtype=torch.float64)).requires_grad_()
    gamma = (0.5 + torch.rand(cout, generator=gen, dtype=torch.float64)).requires_grad_()
    beta = (0.3 * torch.randn(cout, generator=gen, dtype=torch.float64)).requires_grad_()
    g = torch.randn(s["n_out"], cout, generator=gen, dtype=torch.float64)
    ind = torch.from_numpy(s["idx_in"]).int()
    if kind == "subm":
        y = tp.subm_conv2d(x, ind, [s["Y"], s["X"]], R.B, W)
    else:
        y, oidx, _ = tp.sparse_conv2d(x, ind, [s["Y"], s["X"]], R.B, W, 2, 1)
        assert np.array_equal(oidx.numpy().astype(np.int64), s["idx_out"]), "output order differs from the oracle's"
    out = torch.relu(F.batch_norm(y, None, None, gamma, beta, True, 0.0, eps))
    out.backward(g)
    r = R.reference(x.detach(), W.detach(), gamma.detach(), beta.detach(), eps, s["nbr"], g, rounding=False)
    for name, got, want in (("y", r["y"], y.detach()), ("out", r["out"], out.detach()), ("dx", r["dx"], x.grad), ("dW", r["dW"], W.grad),
                            ("dgamma", r["dgamma"], gamma.grad), ("dbeta", r["dbeta"], beta.grad)):
        rel = float((got - want).abs().max() / want.abs().max())
        assert rel <= 1e-12, f"{kind} n={n} {name}: {rel:.2e}"


def _all_scenes():
    for name, c in R.CASES.items():
        yield name, R.scene_full(c["kind"], c["n"], 1000 + sorted(R.CASES).index(name), c.get("m"))
    for name, args in G.RAW_SCENES.items():
        yield name, R.scene_full(*args)


def test_scene_seams_are_reached():
    for name, s in _all_scenes():
        rep = R.scene_feature_report(s)
        want = R.FEATURES_ALL if s["n_in"] >= 110 else R.FEATURES_SMALL       # under 110 rows the border lines do not fit (module docstring)
        assert s["features"] == want, (name, s["features"])
        for f in want:
            assert rep[f], f"scene {name}: feature {f} is not in the rulebook"
        # missing taps exist, and the strided scenes have outputs fed by one input only and inputs feeding several outputs
        assert (s["nbr"] < 0).any() and (s["nbr_t"] < 0).any()
        if s["kind"] == "down":
            assert ((s["nbr_t"] >= 0).sum(1) > 1).any() and ((s["nbr"] >= 0).sum(1) == 1).any() and s["n_out"] != s["n_in"]


def test_block_cases_reach_the_row_counts_they_name():
    n_out = {name: R.scene_full(c["kind"], c["n"], 1000 + sorted(R.CASES).index(name), c.get("m"))["n_out"] for name, c in R.CASES.items()}
    assert 513 <= n_out["3"] <= 1024            # two 64-row chunks per slice (S = 8)
    assert 1025 <= n_out["4"] <= 1536           # three
    for flag in ("out_f32", "g_f32", "running", "x_f32"):
        for v in (0, 1):
            assert sum(1 for c in R.CASES.values() if c["bf16"] and c[flag] == v) >= 2, (flag, v)


def test_caps_on_the_measured_bounds():
    for route, b in G.BOUNDS.items():
        if route.startswith("implicit"):
            assert b["dW_rel_l2"] <= G.CAP_DW_REL_L2 and b["dx_worst_row"] <= G.CAP_DX_WORST_ROW, route


@pytest.mark.parametrize("name", ["1", "2", "3", "5"])
def test_fp32_emulation_of_the_chain_stays_under_the_caps(name):
    """The caps leave room for a correct kernel: an fp32 emulation with the block's bf16 roundings, judged exactly as the GPU test judges
    the kernels (float64 chain started from the emulation's y / out), stays under them."""
    I = R.make_inputs(name)
    c, s = I["case"], I["scene"]
    args = (I["x"], I["W"], I["gamma"], I["beta"], R.EPS, s["nbr"], I["g"])
    e = R.reference(*args, out_f32=bool(c["out_f32"]), dtype=torch.float32)
    r = R.reference(*args, y=e["y"].double(), out=e["out"].double(), out_f32=bool(c["out_f32"]))
    dw = float((e["dW"].double() - r["dW"]).norm() / r["dW"].norm())
    dx_l2, dx_worst = R.row_errors(e["dx"].double(), r["dx"])
    flips = float((e["dy"].double() != r["dy"]).double().mean())
    print(f"case {name}: emulation dW rel L2 {dw:.2e}, dx rel L2 {dx_l2:.2e}, worst row {dx_worst:.2e}, dy flips {flips:.1e}")
    assert dw <= G.CAP_DW_REL_L2 and dx_worst <= G.CAP_DX_WORST_ROW


@pytest.mark.parametrize("name", list(R.CASES))
def test_one_dropped_pair_is_far_outside_the_gpu_bounds(name):
    """A pair from the middle of the rulebook's pair list and the last pair of the last row.  Measured with this test (fp32 emulation):
    the dW change is 1.1e-1 at n = 33, 4.5e-2 at n = 129, 7e-3 at n = 4200 / 8200 and 2.4e-3 at n = 32769 (it falls as 1 / sqrt(9 n);
    threshold 1e-3); the dx row moves by 0.38 - 1.0 of its norm (threshold 0.078); >= 98 % of the y row's elements leave their bound."""
    I = R.make_inputs(name)
    c, s = I["case"], I["scene"]
    rounding = bool(c["bf16"])
    r = R.reference(I["x"], I["W"], I["gamma"], I["beta"], R.EPS, s["nbr"], I["g"], out_f32=bool(c["out_f32"]), rounding=rounding,
                    dtype=torch.float32)
    nbr = s["nbr"]
    o_all, k_all = np.nonzero(nbr >= 0)
    mid = len(o_all) // 2
    last_k = int(np.flatnonzero(nbr[-1] >= 0)[-1])
    bound = G.BOUNDS[R.route(c)]
    thr_dw = 10 * max(G.CAP_DW_REL_L2, bound["dW_rel_l2"])
    thr_dx = 10 * max(G.CAP_DX_WORST_ROW, bound["dx_worst_row"])
    nrm = r["dx"].norm(dim=1)
    rms = float((nrm ** 2).mean().sqrt())
    for (o, k) in ((int(o_all[mid]), int(k_all[mid])), (len(nbr) - 1, last_k)):
        dy_abs, dw_change, dx_change, i = R.drop_pair_effect(r, nbr, o, k)
        dw_rel = dw_change / float(r["dW"].norm())
        dx_rel = dx_change / max(float(nrm[i]), 0.05 * rms)
        yb = G.y_bound(R.route(c), r["y_exact"][o].double(), r["S_abs"][o].double())
        frac = float((dy_abs.double() > yb).double().mean())
        print(f"case {name} pair ({o}, {k}): dW moves {dw_rel:.2e} (>= {thr_dw:.1e}), dx row {dx_rel:.3f} (>= {thr_dx:.3f}), "
              f"{frac:.2f} of the y row beyond its bound")
        assert dw_rel >= thr_dw and dx_rel >= thr_dx
        assert frac >= 0.5
