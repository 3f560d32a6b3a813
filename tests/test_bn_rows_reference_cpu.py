"""tests/bn_rows_reference.py validated without a GPU: its fold / forward / backward against torch.nn.functional.batch_norm + relu
under autograd in float64 (plain rows, a column slice of a wider matrix, the implicit-dense case count > R with `tot`), its max tail
against a per-segment reduction of torch.relu(bn(x)), its tie rule, its row movers, and the rounding-model bounds of the GPU tests:
an fp32 emulation of the kernels' summation shape stays inside them with at least a factor 4 to spare."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_rows_reference as R

TOL = 1e-12


def _close(a, b, tol=TOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.max(np.abs(a - b)) <= tol * max(1.0, np.max(np.abs(b))), np.max(np.abs(a - b))


def _autograd_bn_relu(xfull, gamma, beta, eps, mom, rm, rv, gout):
    x = torch.tensor(xfull, dtype=torch.float64, requires_grad=True)
    g = torch.tensor(gamma, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    rm, rv = torch.tensor(rm, dtype=torch.float64), torch.tensor(rv, dtype=torch.float64)
    y = torch.relu(F.batch_norm(x, rm, rv, g, b, True, mom, eps))
    y.backward(torch.tensor(gout, dtype=torch.float64))
    return y.detach().numpy(), x.grad.numpy(), g.grad.numpy(), b.grad.numpy(), rm.numpy(), rv.numpy()


@pytest.mark.parametrize("layout", ["plain", "slice", "implicit_dense"])
def test_fold_forward_backward_match_autograd(layout):
    rng = np.random.default_rng(3)
    n, C, eps, mom = 97, 12, 1e-3, 0.1
    x = rng.standard_normal((n, C)) * rng.uniform(0.2, 3, C) + rng.uniform(-2, 2, C)
    gamma, beta = rng.uniform(-1.5, 1.5, C), rng.uniform(-0.5, 0.5, C)
    gamma[3] = 0.0
    rm, rv = rng.standard_normal(C), rng.uniform(0.5, 2, C)
    total = n if layout != "implicit_dense" else n + 55           # 55 background sites hold x = 0
    site = rng.permutation(total)[:n] if layout == "implicit_dense" else None
    xfull = x if site is None else np.zeros((total, C))
    if site is not None:
        xfull[site] = x
    zrow, col0 = (C, 0) if layout != "slice" else (C + 20, 8)
    gfull = rng.standard_normal((total, zrow))
    y_t, dx_t, dg_t, db_t, rm_t, rv_t = _autograd_bn_relu(xfull, gamma, beta, eps, mom, rm, rv, gfull[:, col0:col0 + C])

    s1, s2 = R.colsums(x)
    f = R.fold(s1, s2, total, gamma, beta, eps, mom, rm, rv, 7)
    _close(f["running_mean"], rm_t)
    _close(f["running_var"], rv_t)
    assert f["num_batches_tracked"] == 8
    Z0 = np.full((total, zrow), np.nan)
    Z = R.rows_forward(x, f["a"], f["b"], site, Z0, zrow, col0)
    rows = np.arange(n) if site is None else site
    _close(Z[rows, col0:col0 + C], y_t[rows])
    mask = np.ones_like(Z, bool)
    mask[rows, col0:col0 + C] = False
    assert np.isnan(Z[mask]).all()
    if site is not None:                                          # every background site holds the constant relu(b)
        bg = np.setdiff1d(np.arange(total), site)
        _close(np.broadcast_to(np.maximum(f["b"], 0), (len(bg), C)), y_t[bg])
    G = gfull[rows, col0:col0 + C]
    tot = gfull[:, col0:col0 + C].sum(0) if site is not None else None
    k = R.rows_backward(x, f["a"], f["b"], G, f["mean"], f["rstd"], total, tot)
    _close(k["dP"], dx_t[rows])
    _close(k["dgamma"], dg_t)
    _close(k["dbeta"], db_t)
    if site is not None:
        assert (f["b"] > 0).any() and (f["b"] <= 0).any()        # the gate on `tot` is exercised on both sides


def test_sub_add_round_the_relu_first():
    rng = np.random.default_rng(4)
    P = rng.standard_normal((9, 8))
    a, b, v = rng.uniform(0.5, 2, 8), rng.uniform(-1, 1, 8), rng.standard_normal(8)
    y = np.maximum(a * P + b, 0)
    _close(R.rows_forward(P, a, b, sub=v), y - v)
    _close(R.rows_forward(P, a, b, sub=v, z_bf16=True), R.bf16_round(y) - v)
    add = rng.standard_normal((9, 8))
    _close(R.rows_forward(P, a, b, add=add, z_bf16=True), R.bf16_round(y) + add)
    # bf16_round is round-to-nearest-even on the 8-bit mantissa
    assert R.bf16_round(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20])).tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7]


def test_max_tail_matches_autograd_with_first_maximum():
    rng = np.random.default_rng(5)
    C, eps = 8, 1e-3
    sizes = [1, 3, 4, 5, 9, 40]
    pt_off, csr, inv = R.make_pillars(sizes, 1)
    N, M = len(inv), len(sizes)
    x = np.round(rng.standard_normal((N, C)) * 4) / 4            # quarter steps: plenty of exact ties
    gamma, beta = rng.uniform(-1.5, 1.5, C), rng.uniform(-0.5, 0.5, C)
    gamma[1] = -0.7
    dout = rng.standard_normal((M, C))
    s1, s2 = R.colsums(x)
    f = R.fold(s1, s2, N, gamma, beta, eps)
    out, arg = R.segment_max_affine(x, f["a"], f["b"], pt_off, csr)

    xt = torch.tensor(x, requires_grad=True)
    gt, bt = torch.tensor(gamma, requires_grad=True), torch.tensor(beta, requires_grad=True)
    h = torch.relu(F.batch_norm(xt, None, None, gt, bt, True, 0.1, eps))
    sel = torch.zeros(M, C, dtype=torch.int64)
    for p in range(M):
        ids = np.sort(csr[pt_off[p]:pt_off[p + 1]])
        hp = h[ids].detach().numpy()
        sel[p] = torch.tensor(ids[np.argmax(hp, axis=0)])          # first maximum in ascending point id
    o_t = torch.gather(h, 0, sel)
    o_t.backward(torch.tensor(dout))
    _close(out, o_t.detach().numpy())
    assert np.array_equal(arg, sel.numpy())
    sums, _ = R.segmax_affine_sums(x, out, arg, dout)
    k = R.bn_coeffs(sums, f["mean"], f["rstd"], f["a"], f["b"], N)
    dx = f["a"] * R.segmax_affine_dh(out, arg, dout, inv, N) + k["c0"] + k["c1"] * x
    _close(dx, xt.grad.numpy())
    _close(k["dgamma"], gt.grad.numpy())
    _close(k["dbeta"], bt.grad.numpy())
    # the plain maximum and its backward
    o2, a2 = R.segment_max(x, pt_off, csr)
    for p in range(M):
        ids = np.sort(csr[pt_off[p]:pt_off[p + 1]])
        assert np.array_equal(o2[p], x[ids].max(0))
    d2 = R.segment_max_bwd(dout, a2, inv, N)
    assert np.allclose(np.add.reduceat(d2[csr], pt_off[:-1], axis=0), dout, atol=1e-15)
    assert (np.count_nonzero(d2, axis=0) <= M).all()


def test_tie_rule_lowest_point_id_in_any_csr_order():
    C = 4
    pt_off = np.array([0, 5, 6, 11])
    csr = np.array([9, 2, 7, 4, 10, 0, 8, 3, 6, 1, 5])           # neither segment-major nor ascending inside a segment
    x = np.zeros((11, C))
    x[[9, 2, 7, 4, 10]] = 1.5                                     # identical rows
    x[[8, 3, 6, 1, 5]] = -2.0
    out, arg = R.segment_max(x, pt_off, csr)
    assert (arg[0] == 2).all() and (arg[1] == 0).all() and (arg[2] == 1).all()
    out, arg = R.segment_max_affine(x, np.ones(C), np.zeros(C), pt_off, csr)
    assert (out[2] == 0).all() and (arg[2] == 1).all()            # all-zero relu: the lowest id, and no gradient
    inv = np.empty(11, np.int64)
    for p in range(3):
        inv[csr[pt_off[p]:pt_off[p + 1]]] = p
    assert (R.segmax_affine_dh(out, arg, np.ones((3, C)), inv, 11)[[8, 3, 6, 1, 5]] == 0).all()
    # a leading -inf is replaced by any larger value, a leading NaN stays (first point taken, then strictly-greater only)
    y = np.array([[-np.inf, np.nan], [1.0, 1.0], [1.0, 2.0]])
    o, a = R.segment_max(y, np.array([0, 3]), np.array([2, 0, 1]))
    assert o[0, 0] == 1.0 and a[0, 0] == 1 and np.isnan(o[0, 1]) and a[0, 1] == 0


def test_row_movers():
    rng = np.random.default_rng(6)
    tab = rng.integers(0, 255, (7, 12)).astype(np.uint8)
    idx = np.array([3, -1, 0, 6])
    g = R.gather_rows(tab, idx, 4, 4)
    assert np.array_equal(g[0], tab[3, 4:8]) and (g[1] == 0).all() and np.array_equal(g[3], tab[6, 4:8])
    src = rng.integers(0, 255, (4, 4)).astype(np.uint8)
    s = R.scatter_rows(src, idx, tab, 8)
    assert np.array_equal(s[3, 8:], src[0]) and np.array_equal(s[:, :8], tab[:, :8]) and np.array_equal(s[1], tab[1])
    assert np.array_equal(R.fill_rows(np.arange(3), 2), [[0, 1, 2], [0, 1, 2]])


def test_geometry_of_the_partial_sums():
    assert [R.colstats_rows(r) for r in (1, 63, 64, 65, 1000, 32833, (1 << 20) - 1, (1 << 20) + 3)] == [1, 1, 1, 1, 15, 512, 512, 1024]
    assert [R.bwd_stats_rows(n) for n in (1, 31, 32, 33, 1000, 16385)] == [1, 1, 1, 1, 31, 512]
    assert -(-16385 // 512) * 497 > 16385                        # n = 16 385: the last workgroups start beyond the last row
    assert R.sum_depth(32833, 512, 1) == 66 and R.sum_depth(1000, 31, 32) == 34


# ---- the bounds of the GPU tests: an fp32 emulation of the summation shape uses at most a quarter of them -------------------------
@pytest.mark.parametrize("R_,C,bf16", [(1, 4, False), (65, 100, False), (1000, 384, False), (32833, 8, True), (1000, 48, True),
                                      (4099, 128, True)])
def test_colstats_emulation_inside_bounds(R_, C, bf16):
    X, fam = R.stats_matrix(R_, C, 11, bf16)
    nblk, rpi = R.colstats_rows(R_), R.colstats_rpi(C, bf16)
    X64 = X.astype(np.float64)
    s1, s2 = R.colsums(X64)
    e1, _ = R.emulate_sum(X, nblk, rpi)
    e2, _ = R.emulate_sum((X64 * X64).astype(np.float32), nblk, rpi)     # the fma's product is exact; its sum rounds once like an add
    b1 = R.sum_bound(np.abs(X64).sum(0), R_, nblk, rpi)
    b2 = R.sum_bound((X64 * X64).sum(0), R_, nblk, rpi)
    assert (4 * np.abs(e1 - s1) <= b1).all() and (4 * np.abs(e2 - s2) <= b2).all()
    # ... and through the fold: the emulated sums give statistics inside a quarter of the propagated bounds
    gamma, beta = np.linspace(0.5, 1.5, C), np.linspace(-0.3, 0.3, C)
    ref, emu = R.fold(s1, s2, R_, gamma, beta, 1e-3), R.fold(e1, e2, R_, gamma, beta, 1e-3)
    fb = R.fold_bounds(None, None, b1, b2, s1, s2, R_, gamma, beta, 1e-3)
    for k in ("mean", "var", "rstd", "a", "b"):
        assert (4 * np.abs(emu[k] - ref[k]) <= fb[k] + 1e-300).all(), k
    # the constant column: variance >= 0 and rstd finite; the reference's own value is 1 / sqrt(eps) exactly
    assert (ref["var"][fam == 4] == 0).all() and np.allclose(ref["rstd"][fam >= 4], 1 / np.sqrt(1e-3), rtol=1e-15)


@pytest.mark.parametrize("n,C,v8", [(1, 8, True), (33, 100, False), (1000, 48, False), (1000, 64, True), (16385, 128, True)])
def test_bwd_stats_emulation_inside_bounds(n, C, v8):
    rng = np.random.default_rng(12)
    P = rng.standard_normal((n, C)).astype(np.float32)
    G = rng.standard_normal((n, C)).astype(np.float32)
    a, b = rng.uniform(-1.5, 1.5, C).astype(np.float32), rng.uniform(-0.5, 0.5, C).astype(np.float32)
    sums, dh = R.rows_backward_sums(P, a, b, G)
    nblk, rpi = R.bwd_stats_rows(n), R.bwd_stats_rpi(C, v8)
    terms = [dh, dh * P.astype(np.float64), G.astype(np.float64)]
    for k in range(3):
        e, part = R.emulate_sum(terms[k].astype(np.float32), nblk, rpi)
        assert part.shape[0] == nblk
        assert (4 * np.abs(e - sums[k]) <= R.sum_bound(np.abs(terms[k]).sum(0), n, nblk, rpi) + 1e-300).all(), k
