"""Every kernel route of the windowed cosine attention against one float64 reference (tests/window_attention_reference.py), on
crafted window lists: the shipped boundary lengths where the planner puts them (16 tokens in a T = 32 window, 32 in a T = 64 window),
single-token windows in every level, empty levels, levels passed out of capacity order, rows that no window names.

route  rows  impl  entry
  A    fp32   0    all-levels (exact-fp32 MFMA for T >= 32, lane-per-query VALU for T = 16)
  B    fp32   1    all-levels (VALU)
  C    bf16   1    all-levels (VALU, bf16 I/O)
  D    bf16   2    all-levels (fp32 MFMA with bf16 I/O, VALU T = 16)
  E    bf16   0    per-level entries (attention_t16 alone, cooperative forward per level, fp32-MFMA backward)
  F    bf16   0    all-levels with lse and the forward's out (one launch per direction; k_attn_lo_bwd without T = 64 windows)
  G    bf16   0    all-levels, lse = None (cooperative forward, per-level backward)
  H32 / Hbf  0     ops.WindowCosineAttention.apply on fp32 / bf16 rows; Hbf-impl1 / Hbf-impl2: bf16 rows under impl 1 / 2

For the bf16 routes the reference reads the bf16-rounded qk, v and dout: what is left is kernel error.  dtau of the raw entries is
the project's gated sum (gdmae_sum_partials_gated, the clamp's gate) over the partial buffer the backward filled.

Bounds.  y(t) = max |float32 CPU evaluation of the reference - float64 reference| / max |reference| of tensor t, computed here
for every (list, shape, tau): about 2e-7 at tau = 0.2 and 5e-6 at tau_min.
  fp32 rows (A, B, H32):      out max error <= 2e-5 max|ref|; dqk, dv max error <= F32_FACTOR y(t) max|ref|;
                              |dtau - ref| <= 2e-3 |ref| + 1e-6
  fp32 arithmetic, one bf16 store (C, D, Hbf-impl1/2):
                              elementwise |got - ref| <= 2^-8 |ref| + F32_FACTOR y(t) max|ref|; dtau 2e-2 |ref| + 1e-4
  matrix-core (E, F, G, Hbf): relative L2 <= MC_L2, max error <= MC_MAX max|ref|, dtau 2e-2 |ref| + 1e-4
The table under the bounds holds, for every bound, the largest value an MI355X gave over all lists and shapes."""
import json

import numpy as np
import pytest
import torch

import window_attention_reference as war

pytestmark = pytest.mark.gpu

ROUTES = {
    "A": dict(bf16=False, impl=0, entry="levels", bound="fp32"),
    "B": dict(bf16=False, impl=1, entry="levels", bound="fp32"),
    "C": dict(bf16=True, impl=1, entry="levels", bound="bf16io"),
    "D": dict(bf16=True, impl=2, entry="levels", bound="bf16io"),
    "E": dict(bf16=True, impl=0, entry="per-level", bound="mc"),
    "F": dict(bf16=True, impl=0, entry="levels-lse", bound="mc-lse"),
    "G": dict(bf16=True, impl=0, entry="levels", bound="mc"),
    "H32": dict(bf16=False, impl=0, entry="op", bound="fp32"),
    "Hbf": dict(bf16=True, impl=0, entry="op", bound="mc-lse"),
    "Hbf-impl1": dict(bf16=True, impl=1, entry="op", bound="bf16io"),
    "Hbf-impl2": dict(bf16=True, impl=2, entry="op", bound="bf16io"),
}
BASE_ROUTES = ("A", "B", "C", "D", "E", "F", "G", "H32", "Hbf")

# dqk / dv of the fp32 routes and the fp32 part of the bf16-I/O routes: multiples of the yardstick
F32_FACTOR = 32.0
OUT_F32 = 2e-5                       # the bound test_window_attention_fwd_bwd_matches_oracle holds the fp32 kernels to
DTAU_F32 = (2e-3, 1e-6)
DTAU_BF16 = (2e-2, 1e-4)
# matrix-core routes: (relative L2, max error / max |ref|), the bounds of test_packed_window_attention_edge_cases
MC_L2, MC_MAX = 6e-3, 0.06
# ... which hold at tau_min as well, with one exception: dqk of the backward that takes the forward's out and lse (routes F, Hbf).
# Its D = dO . O reads O as the forward stored it, rounded to bf16; dS = P (dP - D) then carries P (D_exact - D), and at tau_min P is
# close to one-hot, dP - D close to zero on the key that counts, so the residue is no longer small next to it.  The float64 reference
# with only that rounding injected (O to bf16 inside D, results to bf16) gives dqk relative L2 6.66e-3 / 6.47e-3 / 6.33e-3 on only32
# d128 / only32 d256 / only64 d128 where the kernel gives 6.91e-3 / 6.57e-3 / 6.69e-3, and 1.70e-3 without it.  Bound = 2 x the largest
# measured value (6.91e-3, only32-F-d128h8-taumin).
MC_LSE_DQK_L2_TAU_MIN = 0.014


# Largest measured values on an MI355X, over all window lists and the three shapes (741 runs), next to the bound they are held to.
#
# fp32 rows: error / (y max|ref|) of dqk and dv - the bound is F32_FACTOR = 32 -, out error / max|ref| (bound 2e-5), |dtau - ref|
#   route     tau      dqk/y   dv/y    out        dtau abs   (|ref| is 10 to 1e3 at tau 0.2 / 0.37, about 1e3 at tau_min)
#   A, H32    0.2      1.88    2.09    4.1e-7     1.9e-4
#   A, H32    0.37     2.19    1.94    3.4e-7     4.5e-5
#   A, H32    tau_min  1.53    1.65    4.2e-6     2.9e-1
#   B         0.2      1.89    1.67    6.2e-7     1.9e-4
#   B         0.37     2.19    1.94    3.6e-7     5.8e-5
#   B         tau_min  1.83    1.94    4.1e-6     1.9e-1
#   zero-norm slices (tau 0.2), error / (y of the slice x its max):  A, H32 2.83   B 3.55
# The ratios do not grow with 1 / tau and the error is spread over the rows: the factor stays at 32.
#
# fp32 arithmetic with one bf16 store: (|got - ref| - 2^-8 |ref|) / (y max|ref|), bound F32_FACTOR = 32
#   route        tau      out     dqk     dv
#   C            0.2      0.18    0.29    0.36
#   C            0.37     0.11    0.20    0.22
#   C            tau_min  0.96    0.15    0.40
#   D            0.2      0.46    0.14    0.24
#   D            0.37     0.11    0.15    0.22
#   D            tau_min  0.96    0.13    0.40
#   Hbf-impl1/2  all      0.52    0.29    0.36
#
# matrix-core: relative L2 (bound 6e-3; dqk of F / Hbf at tau_min 1.4e-2) and max error / max|ref| (bound 0.06), |dtau - ref|
#   route     tau      out.l2   out.max  dqk.l2   dqk.max  dv.l2    dv.max   dtau abs
#   E, G      0.2      2.2e-3   3.0e-3   2.4e-3   4.4e-3   2.2e-3   3.7e-3   1.5e-4
#   E, G      0.37     2.3e-3   3.4e-3   2.4e-3   5.1e-3   2.2e-3   3.7e-3   3.1e-5
#   E, G      tau_min  1.4e-3   3.6e-3   2.5e-3   5.6e-3   1.9e-3   3.4e-3   1.5e-1
#   F, Hbf    0.2      2.2e-3   3.0e-3   2.5e-3   4.4e-3   2.3e-3   3.8e-3   1.7e-4
#   F, Hbf    0.37     2.3e-3   3.4e-3   2.4e-3   5.1e-3   2.4e-3   3.7e-3   5.0e-5
#   F, Hbf    tau_min  1.4e-3   3.6e-3   6.9e-3   7.2e-3   2.0e-3   3.6e-3   4.9e-2
#   zero-norm slices (tau 0.2), all four routes: slice L2 3.3e-3, slice max 5.6e-3, the uniform query's output 5.3e-4 max|ref|
# dtau of F / Hbf before the row-mean correction in coop_bwd (attention_coop.hip): 8.8e-1 at tau 0.2 (bound broken on edges d256h8 and
# on the zero-norm run), 1.5e-1 at 0.37, 1.4e+3 at tau_min, where |ref| is about 1e3 - the same rounding of O inside D, multiplied by the
# row's mean logit.
def _mc_limits(bound, tau_class, nm):
    if bound == "mc-lse" and tau_class == "tau_min" and nm == "dqk":
        return MC_LSE_DQK_L2_TAU_MIN, MC_MAX
    return MC_L2, MC_MAX


_LIST_SHAPES = [(name, d, H) for name in war.WINDOW_LISTS for d, H in war.SHAPES[:2]] + [("edges",) + war.SHAPES[2]]
RUNS = [(name, d, H, r, ti) for name, d, H in _LIST_SHAPES
        for r in BASE_ROUTES + (("Hbf-impl1", "Hbf-impl2") if name == "edges" else ()) for ti in range(len(war.TAUS))]


def _id(run):
    name, d, H, r, ti = run
    return f"{name}-{r}-d{d}h{H}-{war.TAU_IDS[ti]}"


# sentinels, as raw bits: a NaN with a payload for out, a finite odd value for the gradients
_SENT = {(torch.float32, "out"): 0x7FC0BEEF, (torch.float32, "grad"): 0x4640E6B7,      # NaN, 12345.679
         (torch.bfloat16, "out"): 0x7FC1, (torch.bfloat16, "grad"): 0x4641}            # NaN, 12352
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def _filled(shape, dtype, kind, dev):
    return torch.full(shape, _SENT[(dtype, kind)], dtype=_INT[dtype], device=dev).view(dtype)


def _bits(t):
    return t.contiguous().view(_INT[t.dtype])


def _run_raw(route, w, qk, v, dout, tau, d, H, dev):
    """One forward + backward through the C entries.  Returns dict(out, dqk, dv, part, dtau, lse)."""
    from gdmae_hip import lib as L
    dt = torch.bfloat16 if route["bf16"] else torch.float32
    bf = int(route["bf16"])
    n = w["n"]
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32).to(dev)   # noqa: E731
    csr, ws, wl = i32(w["csr"]), i32(w["win_start"]), i32(w["win_len"])
    qk_d, v_d, go = qk.to(dev, dt), v.to(dev, dt), dout.to(dev, dt)
    out = _filled((n, d), dt, "out", dev)
    dqk = _filled((n, 2 * d), dt, "grad", dev)
    dv = _filled((n, d), dt, "grad", dev)
    n_win, mt = w["n_win"], w["max_tokens"]
    part = torch.full((sum(n_win) * H,), 123.0, device=dev)                # every slot must be written
    tau_d = torch.full((1,), tau, dtype=torch.float32, device=dev)
    nl, nw_h, T_h = len(n_win), L.host_i32(n_win), L.host_i32(mt)
    lse = None
    if route["entry"] == "per-level":
        base = pb = 0
        for nw, T in zip(n_win, mt):
            L.call("gdmae_window_attention_fwd", L.ptr(qk_d), L.ptr(v_d), L.ptr(out), bf, L.ptr(csr), L.ptr(ws[base:]), L.ptr(wl[base:]), nw, T,
                   d, H, L.ptr(tau_d), war.TAU_MIN, L.stream())
            L.call("gdmae_window_attention_bwd", L.ptr(qk_d), L.ptr(v_d), L.ptr(go), L.ptr(dqk), L.ptr(dv), bf, L.ptr(part[pb:]), L.ptr(csr),
                   L.ptr(ws[base:]), L.ptr(wl[base:]), nw, T, d, H, L.ptr(tau_d), war.TAU_MIN, L.stream())
            base += nw
            pb += nw * H
    else:
        if route["entry"] == "levels-lse":
            assert L.load().gdmae_window_attention_levels_writes_lse(bf, nl, T_h, d, H) == 1
            lse = torch.full((n, H), float("nan"), device=dev)
        L.call("gdmae_window_attention_levels_fwd", L.ptr(qk_d), L.ptr(v_d), L.ptr(out), bf, L.ptr(csr), L.ptr(ws), L.ptr(wl), nl, nw_h, T_h, d, H,
               L.ptr(tau_d), war.TAU_MIN, L.ptr(lse), L.stream())
        lse_fwd = lse.clone() if lse is not None else None
        L.call("gdmae_window_attention_levels_bwd", L.ptr(qk_d), L.ptr(v_d), L.ptr(go), L.ptr(dqk), L.ptr(dv), bf, L.ptr(part), L.ptr(csr),
               L.ptr(ws), L.ptr(wl), nl, nw_h, T_h, d, H, L.ptr(tau_d), war.TAU_MIN, L.ptr(out if lse is not None else None), L.ptr(lse),
               L.stream())
        lse = lse_fwd
    dtau = torch.full((1,), 7.0, device=dev)
    L.call("gdmae_sum_partials_gated", L.ptr(part), part.numel(), 1.0, L.ptr(dtau), L.ptr(tau_d), war.TAU_MIN, L.stream())
    torch.cuda.synchronize(dev)
    return dict(out=out, dqk=dqk, dv=dv, part=part, dtau=dtau, lse=lse)


def _run_op(route, w, qk, v, dout, tau, d, H, dev):
    """ops.WindowCosineAttention.apply with a WindowPlan, tau a (1, 1, 1) leaf, a non-contiguous dout."""
    from gdmae_hip import ops
    from gdmae_hip.plan import WindowPlan
    dt = torch.bfloat16 if route["bf16"] else torch.float32
    p = war.plan_fields(w)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32).to(dev)   # noqa: E731
    plan = WindowPlan(i32(p["tok_win"]), i32(p["tok_level"]), i32(p["tok_slot"]), torch.zeros(w["n"], dtype=torch.int32, device=dev),
                      i32(w["csr"]), i32(w["win_start"]), i32(w["win_len"]), list(w["n_win"]), list(p["n_tok"]), list(w["max_tokens"]))
    qk_d = qk.to(dev, dt).requires_grad_(True)
    v_d = v.to(dev, dt).requires_grad_(True)
    tau_d = torch.full((1, 1, 1), tau, dtype=torch.float32, device=dev).requires_grad_(True)
    out = ops.WindowCosineAttention.apply(qk_d, v_d, tau_d, plan, H, war.TAU_MIN)
    assert out.dtype == dt
    wide = torch.zeros(w["n"], 2 * d, dtype=dt, device=dev)
    go = wide[:, ::2]
    go.copy_(dout.to(dev, dt))
    assert not go.is_contiguous()
    out.backward(go)
    torch.cuda.synchronize(dev)
    assert tau_d.grad.shape == (1, 1, 1)
    return dict(out=out.detach(), dqk=qk_d.grad, dv=v_d.grad, part=None, dtau=tau_d.grad.reshape(1), lse=None)


def _run(rname, w, qk, v, dout, tau, d, H, dev):
    from gdmae_hip import lib as L
    route = ROUTES[rname]
    try:
        L.call("gdmae_set_attention_impl", route["impl"])
        return (_run_op if route["entry"] == "op" else _run_raw)(route, w, qk, v, dout, tau, d, H, dev)
    finally:
        L.call("gdmae_set_attention_impl", 0)


def _structure_checks(rname, w, r1, r2, H):
    """What holds whatever the numbers are: sentinels on unreferenced rows, every partial slot written, lse rows, two identical calls."""
    route = ROUTES[rname]
    unref = torch.from_numpy(w["unref"])
    ref_rows = torch.from_numpy(np.setdiff1d(np.arange(w["n"]), w["unref"]))
    if route["entry"] != "op":
        for nm, kind in (("out", "out"), ("dqk", "grad"), ("dv", "grad")):
            t = r1[nm]
            assert bool((_bits(t).cpu()[unref] == torch.tensor(_SENT[(t.dtype, kind)], dtype=_INT[t.dtype])).all()), \
                f"{nm}: a row that no window names was written"
            assert torch.equal(_bits(t), _bits(r2[nm])), f"{nm}: two identical calls differ"
        assert bool((r1["part"] != 123.0).all()), "a dtau partial slot was not written"
        assert torch.equal(r1["part"], r2["part"]), "dtau partials: two identical calls differ"
        if r1["lse"] is not None:
            dense = [int(t) for i, (s, k) in enumerate(zip(w["win_start"], w["win_len"])) if w["max_tokens"][w["level_of_win"][i]] >= 32
                     for t in w["csr"][s:s + k]]
            if dense:
                assert bool(torch.isfinite(r1["lse"].cpu()[torch.tensor(dense)]).all()), "lse of a T = 32 / 64 row is not finite"
    else:
        # the op allocates its results itself (torch.empty): nothing to pre-fill, unreferenced rows are not looked at
        for nm in ("out", "dqk", "dv"):
            assert torch.equal(_bits(r1[nm]).cpu()[ref_rows], _bits(r2[nm]).cpu()[ref_rows]), f"{nm}: two identical calls differ"
    assert torch.equal(r1["dtau"], r2["dtau"]), "dtau: two identical calls differ"
    for nm in ("out", "dqk", "dv"):
        assert bool(torch.isfinite(r1[nm].float().cpu()[ref_rows]).all()), f"{nm} is not finite on a referenced row"
    return ref_rows


def _figures(bound, got, ref, y, tau_class):
    """[(name, measured, limit)] of one tensor triple + dtau against the reference, by bound class."""
    figs = []
    for i, nm in enumerate(("out", "dqk", "dv")):
        g, r = got[i], ref[i]
        err = (g - r).abs()
        mx = float(r.abs().max())
        if bound == "fp32":
            lim = OUT_F32 if nm == "out" else F32_FACTOR * y[i]
            figs.append((f"{nm}.max", float(err.max()) / mx if mx > 0 else float(err.max()), lim))
            if nm != "out":
                figs.append((f"{nm}.max/y", float(err.max()) / (mx * y[i]) if mx * y[i] > 0 else float(err.max()), F32_FACTOR))
        elif bound == "bf16io":
            slack = err - (2.0 ** -8 * r.abs() + F32_FACTOR * y[i] * mx)
            figs.append((f"{nm}.excess", float(slack.max()), 0.0))
            # the same check as a multiple of y: (|got - ref| - 2^-8 |ref|) / (y max|ref|)
            figs.append((f"{nm}.max/y", float((err - 2.0 ** -8 * r.abs()).max()) / (mx * y[i]) if mx * y[i] > 0 else float(err.max()),
                         F32_FACTOR))
        else:
            l2, mxb = _mc_limits(bound, tau_class, nm)
            rn = float(r.norm())
            figs.append((f"{nm}.l2", float(err.norm()) / rn if rn > 0 else float(err.norm()), l2))
            figs.append((f"{nm}.max", float(err.max()) / mx if mx > 0 else float(err.max()), mxb))
    rel, ab = DTAU_F32 if bound == "fp32" else DTAU_BF16
    figs.append(("dtau", abs(float(got[3]) - float(ref[3])), rel * abs(float(ref[3])) + ab))
    return figs


def _assert_figures(tag, figs):
    print("MEASURE " + json.dumps({"id": tag, "fig": {k: v for k, v, _ in figs}, "lim": {k: b for k, _, b in figs}}))
    bad = [f"{k} = {v:.3e} > {b:.3e}" for k, v, b in figs if not v <= b]
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("run", RUNS, ids=[_id(r) for r in RUNS])
def test_route_matches_fp64_reference(run):
    """One route on one window list, shape and tau: forward and backward with a random dout against the float64 reference within
    the route's bounds; sentinels intact on the rows no window names; every dtau partial slot written; a second call bit-identical;
    at tau_min a non-zero dtau, below it dtau = 0 and everything else bit-identical to the run at tau_min."""
    name, d, H, rname, ti = run
    tau = war.TAUS[ti]
    route = ROUTES[rname]
    dev = torch.device("cuda:0")
    w, qk, v, dout, ref, y, _, _ = war.cached_reference(name, d, H, tau, route["bf16"])
    r1 = _run(rname, w, qk, v, dout, tau, d, H, dev)
    r2 = _run(rname, w, qk, v, dout, tau, d, H, dev)
    rows = _structure_checks(rname, w, r1, r2, H)
    got = [r1[nm].double().cpu()[rows] for nm in ("out", "dqk", "dv")] + [r1["dtau"].double().cpu()[0]]
    refr = [t[rows] for t in ref[:3]] + [ref[3]]
    if r1["part"] is not None and tau >= war.TAU_MIN:
        # the gated sum is the plain sum of the partial slots (at most 240 here: 240 x 2^-24 of sum |partial| covers any fp32 order)
        ps = r1["part"].double()
        assert abs(float(ps.sum()) - float(r1["dtau"][0])) <= 2e-5 * float(ps.abs().sum()), "dtau is not the sum of its partials"
    if tau < war.TAU_MIN:
        # below the clamp: no gradient to tau, and everything else is the same route's run at tau_min, bit for bit
        assert float(r1["dtau"][0]) == 0.0 and float(ref[3]) == 0.0, "dtau must be exactly 0 below tau_min"
        at = _run(rname, w, qk, v, dout, war.TAU_MIN, d, H, dev)
        for nm in ("out", "dqk", "dv"):
            assert torch.equal(_bits(r1[nm]).cpu()[rows], _bits(at[nm]).cpu()[rows]), f"{nm}: tau = 0.004 differs from tau = tau_min"
    elif tau == war.TAU_MIN and float(ref[3]) != 0.0:
        assert float(r1["dtau"][0]) != 0.0, "tau == tau_min: the clamp's gradient must pass"
    _assert_figures(_id(run), _figures(route["bound"], got, refr, y, "tau_min" if tau <= war.TAU_MIN else "tau"))


ZN_RUNS = [(d, H, r) for d, H in war.SHAPES for r in ROUTES]


@pytest.mark.parametrize("run", ZN_RUNS, ids=[f"{r}-d{d}h{H}" for d, H, r in ZN_RUNS])
def test_zero_norm_head_slices(run):
    """``edges`` list, tau = 0.2; in one window of each level one token's q slice of head 0 and another token's k slice of head 3 are
    zero (the eps branch of the normalisation).  The query's head-0 output is the plain mean of the window's v slices; everything is
    finite; outside the six edited gradient slices (about 1e12 by the eps rule) the normal bounds hold; the edited slices are
    compared relative to their own largest reference element, with a yardstick taken on the slice."""
    d, H, rname = run
    dh = d // H
    tau = war.TAUS[0]
    route = ROUTES[rname]
    bound = route["bound"]
    dev = torch.device("cuda:0")
    w, qk, v, dout, ref, _, f32, edits = war.cached_reference("edges", d, H, tau, route["bf16"], zero_norm=True)
    r1 = _run(rname, w, qk, v, dout, tau, d, H, dev)
    r2 = _run(rname, w, qk, v, dout, tau, d, H, dev)
    rows = _structure_checks(rname, w, r1, r2, H)
    got = [r1[nm].double().cpu() for nm in ("out", "dqk", "dv")]
    slices = [(rq, slice(war.ZERO_Q_HEAD * dh, (war.ZERO_Q_HEAD + 1) * dh)) for _, rq, _ in edits] + \
             [(rk, slice(d + war.ZERO_K_HEAD * dh, d + (war.ZERO_K_HEAD + 1) * dh)) for _, _, rk in edits]
    figs = []
    # the six edited slices of dqk, each on its own scale
    for i, (row, sl) in enumerate(slices):
        g, r, f = got[1][row, sl], ref[1][row, sl], f32[1][row, sl].double()
        mx = float(r.abs().max())
        assert mx > 1e9
        ys = float((f - r).abs().max()) / mx
        err = (g - r).abs()
        if bound == "fp32":
            figs.append((f"edit{i}.max/y", float(err.max()) / (mx * ys), F32_FACTOR))
        elif bound == "bf16io":
            figs.append((f"edit{i}.max/y", float((err - 2.0 ** -8 * r.abs()).max()) / (mx * ys), F32_FACTOR))
        else:
            figs.append((f"edit{i}.l2", float(err.norm() / r.norm()), MC_L2))
            figs.append((f"edit{i}.max", float(err.max()) / mx, MC_MAX))
    # everything else: the edited slices taken out of dqk on both sides and out of the yardstick
    refm, f32m = [t.clone() for t in ref[:3]], [t.double().clone() for t in f32[:3]]
    for row, sl in slices:
        for t in (got[1], refm[1], f32m[1]):
            t[row, sl] = 0
    y = tuple(float((a[rows] - b[rows]).abs().max() / b[rows].abs().max()) for a, b in zip(f32m, refm))
    figs += _figures(bound, [t[rows] for t in got] + [r1["dtau"].double().cpu()[0]], [t[rows] for t in refm] + [ref[3]], y, "tau")
    # the zero query attends uniformly
    for wi, rq, _ in edits:
        s, k = int(w["win_start"][wi]), int(w["win_len"][wi])
        mean = v[torch.from_numpy(w["csr"][s:s + k]), :dh].double().mean(0)
        err = (got[0][rq, :dh] - mean).abs()
        mx = float(refm[0][rows].abs().max())
        if bound == "fp32":
            figs.append((f"mean{wi}.max", float(err.max()) / mx, OUT_F32))
        elif bound == "bf16io":
            figs.append((f"mean{wi}.excess", float((err - (2.0 ** -8 * mean.abs() + F32_FACTOR * y[0] * mx)).max()), 0.0))
        else:
            figs.append((f"mean{wi}.max", float(err.max()) / mx, MC_MAX))
    _assert_figures(f"zeronorm-{rname}-d{d}h{H}", figs)
