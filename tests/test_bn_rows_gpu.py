"""The BatchNorm(train)+ReLU row kernels of csrc/segment.hip and csrc/decoder.hip through the C ABI, and the autograd wrappers of
gdmae_hip/vfe.py on top of them, against the float64 reference and the rounding-model bounds of tests/bn_rows_reference.py
(validated without a GPU by tests/test_bn_rows_reference_cpu.py).

Every reference works from the values the device consumed: bf16 inputs upcast exactly, and for the elementwise kernels the device's
own fp32 a|b and c0|c1 vectors, so each kernel is judged on its own arithmetic.  Output buffers start as NaN (ints / bytes: a
sentinel) and everything outside the addressed rows and columns must still hold it; gradient maps hold NaN wherever the kernel has
no business reading.  Shapes are the smallest at which the dispatch or the loop structure changes: the scalar twins (C % 8, an odd
row pitch or first column, C = 48 / 96 / 100 for the statistics kernels), every (P, Z, dP) dtype combination, n below / at / above
one chunk of the partial sums, the empty trailing workgroups at n = 16 385, the 1024-partial switch at 2^20 rows, the grid-stride
loops behind the 8 192- and 16 384-workgroup caps, every width of the segmented maximum at pillar sizes around its lane-group
count, ties, -inf / NaN, dead pillars, and BatchNorm scales from 1 down to 0 in the max layer's backward.

Each check prints measured error / bound; the worst per entry point is collected and written to the file named by the environment
variable BN_ROWS_RECORD when set (profiles/bn_rows_reference.txt is that file from an MI355X run).

Measured (MI355X, worst error / bound): column sums 0.11, folded statistics <= 0.11 (running statistics 0.45, mostly their fp32
arithmetic), elementwise fp32 results <= 0.5 and bf16 results up to 0.99 (2^-8 is bf16's unit roundoff, reached just above a power of
two), backward column sums <= 0.03, coefficients <= 0.6, segmented maximum and row movers exact.  The variance's relative error
per mean/std family: 3e-7 (0), 1e-6 (1), 7e-4 (30), 7e-2 (300), each at 0.07 - 0.11 of its bound, which grows with mean^2 / var.
One defect was found and fixed: gdmae_segmax_bwd_stats (a, b given) took x as (out - b) / a for every |a| >= 1e-30; with
BatchNorm scales of 1e-6 and 1e-9 at b ~ 0.5 sum dh x missed its bound 750- and 56 000-fold (dgamma, c0, c1 and dx with it).  The
kernel now reconstructs x only where (|b| + |out|) / |a| <= 4 |x| and reads it through arg elsewhere: every scale sits at <= 0.01
of the bound (dx 0.28), the same as the kernel that always reads x.
"""
import functools
import os

import numpy as np
import pytest
import torch

import bn_rows_reference as R
from gdmae_hip import bn as gbn
from gdmae_hip import lib as L
from gdmae_hip import vfe as gvfe

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-3, 0.1
NAN = float("nan")
_REC, _VAR, _SMALL = {}, {}, {}


def _dev():
    return torch.device("cuda:0")


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(_dev())


def _mk(x, bf):
    """fp32 array -> device tensor of the kernel's dtype and the float64 values it holds."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    t = t.bfloat16() if bf else t
    return t.to(_dev()), t.float().numpy().astype(np.float64)


def _f64(t):
    return t.detach().to(torch.float64).cpu().numpy()


def _nan(shape, bf=False, dtype=None):
    return torch.full(shape, NAN, dtype=dtype or (torch.bfloat16 if bf else torch.float32), device=_dev())


def _ws(nbytes):
    return torch.empty(int(nbytes), dtype=torch.uint8, device=_dev())


def _hold(name, got, ref, bound):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = np.abs(got - ref)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    worst = float(np.nanmax(ratio)) if ratio.size else 0.0
    _REC[name] = max(_REC.get(name, 0.0), worst)
    print(f"{name}: worst error / bound {worst:.3f} (largest error {float(np.nanmax(err)) if err.size else 0:.3e})")
    assert not np.isnan(got).any(), f"{name}: NaN in the result"
    assert (err <= bound).all(), f"{name}: error / bound {worst:.3f}"


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    lines = ["worst measured error / bound per entry point and case family"]
    lines += [f"  {k:<58s} {v:.3f}" for k, v in sorted(_REC.items())]
    lines += ["variance: largest |var - ref| / ref (and as a share of its bound) per mean/std family, over all shapes"]
    lines += [f"  {k:<58s} {v[0]:.3e}  ({v[1]:.3f} of the bound)" for k, v in sorted(_VAR.items())]
    lines += ["max layer backward, BatchNorm scale gamma x s at b ~ 0.5: worst error / bound of sum dh x, dgamma, c0, c1, dx"]
    lines += [f"  {k:<58s} " + "  ".join(f"{x:.3f}" for x in v) for k, v in sorted(_SMALL.items())]
    print("\n".join(lines))
    path = os.environ.get("BN_ROWS_RECORD")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(autouse=True)
def _stop_on_device_error():
    """a device error is sticky: nothing more is started on the GPU after one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, stopping: {e}", returncode=3)


# ====================================================================================================== statistics
ROWS = (1, 63, 64, 65, 1000, 32833)
STAT_CASES = [(r, c, False) for c in (4, 100, 384, 1024) for r in ROWS] + [(r, c, True) for c in (8, 48, 128, 384, 2048) for r in ROWS] \
    + [((1 << 20) + 3, 4, False), ((1 << 20) + 3, 8, True)]


@functools.lru_cache(None)
def _stats_base(bf):
    return R.stats_matrix(32833, 2048, 21, bf)


@functools.lru_cache(None)
def _affine(C, seed=31):
    rng = np.random.default_rng(seed)
    gamma = (rng.uniform(0.5, 1.5, C) * np.where(rng.random(C) < 0.3, -1, 1)).astype(np.float32)
    gamma[C // 2] = 0.0
    return gamma, rng.uniform(-0.5, 0.5, C).astype(np.float32)


def _colstats(x, R_, C, bf):
    out = _nan((2 * C,), dtype=torch.float64)
    ws = _ws(L.load().gdmae_colstats_workspace_bytes(C))
    L.call("gdmae_colstats", L.ptr(x), R_, C, int(bf), L.ptr(out), L.ptr(ws), L.stream())
    return out


def _fold(x, R_, C, bf, count, gamma, beta, rm=None, rv=None, nb=None, part=None):
    stats, ab, mv = _nan((2 * C,), dtype=torch.float64), _nan((2 * C,)), _nan((2 * C,))
    tail = (L.ptr(gamma), L.ptr(beta), EPS, MOM, L.ptr(rm), L.ptr(rv), L.ptr(nb), L.ptr(stats), L.ptr(ab), L.ptr(mv))
    if part is not None:
        L.call("gdmae_bn_fold_partials", L.ptr(part), part.shape[0], C, float(count), *tail, L.stream())
    else:
        ws = _ws(L.load().gdmae_colstats_workspace_bytes(C))
        L.call("gdmae_bn_fold", L.ptr(x), R_, C, int(bf), float(count), *tail, L.ptr(ws), L.stream())
    return stats, ab, mv


def _check_fold(tag, C, count, s1, s2, b1, b2, gamma, beta, run, fam=None):
    """run(rm, rv, nb) -> (stats, ab, mv) on the device; checked against R.fold under R.fold_bounds, running statistics twice."""
    g64, be64 = gamma.astype(np.float64), beta.astype(np.float64)
    rng = np.random.default_rng(5)
    rm0, rv0 = rng.standard_normal(C).astype(np.float32), rng.uniform(0.5, 2, C).astype(np.float32)
    rm, rv, nb = _t(rm0), _t(rv0), _t(np.array([5], np.int64))
    stats, ab, mv = run(rm, rv, nb)
    ref = R.fold(s1, s2, count, g64, be64, EPS, MOM, rm0, rv0, 5)
    fb = R.fold_bounds(None, None, b1, b2, s1, s2, count, g64, be64, EPS)
    st, abh, mvh = _f64(stats), _f64(ab), _f64(mv)
    _hold(f"{tag} mean", st[:C], ref["mean"], fb["mean"])
    _hold(f"{tag} rstd", st[C:], ref["rstd"], fb["rstd"])
    _hold(f"{tag} a", abh[:C], ref["a"], fb["a"])
    _hold(f"{tag} b", abh[C:], ref["b"], fb["b"])
    _hold(f"{tag} mv mean", mvh[:C], ref["mean"], fb["mean32"])
    _hold(f"{tag} mv var", mvh[C:], ref["var"], fb["var32"])
    assert (mvh[C:] >= 0).all()
    unbf = count / (count - 1.0) if count > 1 else 1.0
    b_rm = MOM * fb["mean32"] + 4 * R.U * (np.abs(rm0) + MOM * np.abs(ref["mean"]))
    b_rv = MOM * unbf * fb["var32"] + 4 * R.U * (np.abs(rv0) + MOM * unbf * ref["var"])
    _hold(f"{tag} running_mean", _f64(rm), ref["running_mean"], b_rm)
    _hold(f"{tag} running_var", _f64(rv), ref["running_var"], b_rv)
    assert int(nb.item()) == 6
    stats2, ab2, mv2 = run(rm, rv, nb)            # a second batch on the same module buffers: momentum twice, counter + 2
    ref2 = R.fold(s1, s2, count, g64, be64, EPS, MOM, ref["running_mean"], ref["running_var"], 6)
    _hold(f"{tag} running_mean, 2nd call", _f64(rm), ref2["running_mean"], 2 * b_rm + 4 * R.U * np.abs(ref["running_mean"]))
    _hold(f"{tag} running_var, 2nd call", _f64(rv), ref2["running_var"], 2 * b_rv + 4 * R.U * np.abs(ref["running_var"]))
    assert int(nb.item()) == 7 and ref2["num_batches_tracked"] == 7
    assert torch.equal(stats, stats2) and torch.equal(ab, ab2) and torch.equal(mv, mv2)      # two calls bit-equal
    nb5 = _t(np.array([5], np.int64))             # null running pointers: same statistics, nothing else written
    stats3, ab3, _ = run(None, None, nb5)
    assert torch.equal(stats, stats3) and torch.equal(ab, ab3) and int(nb5.item()) == 5
    if fam is not None:
        flat = fam[:C] >= 4                        # constant column and all-zero column: var >= 0, rstd = 1 / sqrt(eps) to 1e-6
        assert np.isfinite(st[C:]).all()
        assert (np.abs(st[C:][flat] * np.sqrt(EPS) - 1.0) <= 1e-6).all(), st[C:][flat]
        for k in range(4):
            m = (fam[:C] == k) & (ref["var"] > 0)
            if m.any():
                e = np.abs(mvh[C:][m] - ref["var"][m])
                key = f"mean/std = {R.FAMILIES[k]:g}"
                old = _VAR.get(key, (0.0, 0.0))
                _VAR[key] = (max(old[0], float(np.max(e / ref["var"][m]))), max(old[1], float(np.max(e / fb["var32"][m]))))
    return stats, ab, mv


@pytest.mark.parametrize("R_,C,bf", STAT_CASES)
def test_colstats_and_bn_fold(R_, C, bf):
    if R_ <= 32833:
        base, fam = _stats_base(bf)
        X = np.ascontiguousarray(base[:R_, :C])
    else:
        X, fam = R.stats_matrix(R_, C, 22, bf)
    x, X64 = _mk(X, bf)
    s1, s2 = R.colsums(X64)
    nblk, rpi = R.colstats_rows(R_), R.colstats_rpi(C, bf)
    b1, b2 = R.sum_bound(np.abs(X64).sum(0), R_, nblk, rpi), R.sum_bound(s2, R_, nblk, rpi)
    tag = "colstats bf16" if bf else "colstats fp32"
    out = _colstats(x, R_, C, bf)
    _hold(f"{tag} sum", _f64(out)[:C], s1, b1)
    _hold(f"{tag} sum of squares", _f64(out)[C:], s2, b2)
    assert torch.equal(out, _colstats(x, R_, C, bf))
    gamma, beta = _affine(C)
    g, b = _t(gamma), _t(beta)
    tag = "bn_fold bf16" if bf else "bn_fold fp32"
    _check_fold(tag, C, R_, s1, s2, b1, b2, gamma, beta, lambda rm, rv, nb: _fold(x, R_, C, bf, R_, g, b, rm, rv, nb), fam)
    _check_fold(tag + ", count > R", C, R_ + 37, s1, s2, b1, b2, gamma, beta,
                lambda rm, rv, nb: _fold(x, R_, C, bf, R_ + 37, g, b, rm, rv, nb))


@pytest.mark.parametrize("nblk", [1, 15, 16, 17, 129, 300])
@pytest.mark.parametrize("C", [7, 100])
def test_bn_fold_partials_from_hand_made_rows(nblk, C):
    rng = np.random.default_rng(nblk * 1000 + C)
    rows = 40
    X = (rng.standard_normal((nblk, rows, C)) + rng.uniform(-2, 2, C)).astype(np.float32).astype(np.float64)
    part = np.stack([X.sum(1), (X * X).sum(1)], axis=1).astype(np.float32)           # (nblk, 2, C)
    p64 = part.astype(np.float64)
    s1, s2 = p64[:, 0].sum(0), p64[:, 1].sum(0)
    tiny1, tiny2 = 2.0 ** -50 * np.abs(p64[:, 0]).sum(0), 2.0 ** -50 * p64[:, 1].sum(0)    # the combine is float64
    gamma, beta = _affine(C)
    g, b, pd = _t(gamma), _t(beta), _t(part)
    for count in (nblk * rows, nblk * rows + 11):
        _check_fold("bn_fold_partials", C, count, s1, s2, tiny1, tiny2, gamma, beta,
                    lambda rm, rv, nb: _fold(None, 0, C, False, count, g, b, rm, rv, nb, part=pd))


# ====================================================================================================== elementwise rows
WIDTHS = (8, 48, 64, 100, 128, 256)
DT2 = [(False, False), (False, True), (True, False), (True, True)]


def _layouts(C):
    out = [("plain", C, 0)] + [(f"slice{c0}", 384, c0) for c0 in (0, 128, 256) if c0 + C <= 384]
    return out + [("odd", C + 4, 4)]


def _site(kind, n, rng):
    if kind == "null":
        return None, n
    if kind == "perm":
        return rng.permutation(n).astype(np.int32), n
    return rng.choice(2 * n + 3, n, replace=False).astype(np.int32), 2 * n + 3


def _rows_inputs(n, C, pbf, seed):
    """P, a, b with a negative and two zero entries in a, and pre-activations that are exactly 0 (channel 2 on every third row;
    channel 1 everywhere)."""
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((n, C)).astype(np.float32)
    a = (rng.uniform(0.5, 1.5, C) * np.where(rng.random(C) < 0.3, -1, 1)).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, C).astype(np.float32)
    a[0], a[1], b[1], a[2], b[2], a[3], b[3] = -abs(a[0]), 0.0, 0.0, 1.0, -0.75, 0.0, 0.25
    P[::3, 2] = 0.75
    return P, a, b


def _fwd(P, pbf, site, n, C, a, b, Z, zbf, zrow, col0, sub=None, add=None):
    if sub is not None:
        L.call("gdmae_rows_affine_relu_sub", L.ptr(P), int(pbf), L.ptr(site), n, C, L.ptr(a), L.ptr(b), L.ptr(sub), L.ptr(Z), int(zbf),
               zrow, col0, L.stream())
    elif add is not None:
        L.call("gdmae_rows_affine_relu_add", L.ptr(P), int(pbf), n, C, L.ptr(a), L.ptr(b), L.ptr(add), L.ptr(Z), int(zbf), L.stream())
    else:
        L.call("gdmae_rows_affine_relu_scatter", L.ptr(P), int(pbf), L.ptr(site), n, C, L.ptr(a), L.ptr(b), L.ptr(Z), int(zbf), zrow,
               col0, L.stream())


def _check_map(name, Zdev, ref, bound, rows, col0, C):
    """addressed block inside the bound, everything else still NaN."""
    Zh = _f64(Zdev)
    mask = np.zeros(Zh.shape, bool)
    mask[rows, col0:col0 + C] = True
    assert np.isnan(Zh[~mask]).all(), f"{name}: written outside the addressed rows / columns"
    _hold(name, Zh[rows, col0:col0 + C], ref, bound)


def _forward_case(name, n, C, pbf, zbf, zrow, col0, kind, seed):
    rng = np.random.default_rng(seed)
    P, a, b = _rows_inputs(n, C, pbf, seed)
    Pd, P64 = _mk(P, pbf)
    site, zrows = _site(kind, n, rng)
    Z = _nan((zrows, zrow), zbf)
    _fwd(Pd, pbf, None if site is None else _t(site), n, C, _t(a), _t(b), Z, zbf, zrow, col0)
    ref = np.maximum(a.astype(np.float64) * P64 + b, 0.0)
    rows = np.arange(n) if site is None else site
    full = R.rows_forward(P64, a, b, site, np.full((zrows, zrow), np.nan), zrow, col0)
    assert np.array_equal(full[rows, col0:col0 + C], ref)
    _check_map(name, Z, ref, R.elementwise_bound(a, P64, b, ref, zbf), rows, col0, C)
    zero = (a.astype(np.float64) * P64 + b) == 0
    assert zero[:, 1].all() and zero[::3, 2].all() and (_f64(Z)[rows, col0:col0 + C][zero] == 0).all()     # the ReLU boundary


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("pbf,zbf", DT2)
def test_rows_affine_relu_scatter(pbf, zbf, C):
    seed = 100
    for lname, zrow, col0 in _layouts(C):
        for kind in ("null", "perm", "subset"):
            for n in (1, 7, 1000):
                seed += 1
                v8 = C % 8 == 0 and zrow % 8 == 0 and col0 % 8 == 0
                _forward_case(f"rows_affine_relu_scatter {'v8' if v8 else 'scalar'} P {'bf16' if pbf else 'fp32'} Z {'bf16' if zbf else 'fp32'}",
                              n, C, pbf, zbf, zrow, col0, kind, seed)


@pytest.mark.parametrize("n,C,zrow,col0,pbf,zbf", [(66000, 256, 256, 0, True, True), (21001, 100, 104, 4, False, False)])
def test_rows_affine_relu_scatter_grid_stride(n, C, zrow, col0, pbf, zbf):
    assert (n * C // 8 if (C % 8 == 0 and zrow % 8 == 0 and col0 % 8 == 0) else n * C) > 8192 * 256
    _forward_case("rows_affine_relu_scatter grid-stride loop", n, C, pbf, zbf, zrow, col0, "perm", 7)


@pytest.mark.parametrize("C", [8, 48, 64, 128, 256])
@pytest.mark.parametrize("pbf,zbf", DT2)
def test_rows_affine_relu_sub_and_add(pbf, zbf, C):
    seed = 300
    for n in (1, 7, 1000):
        for lname, zrow, col0 in [l for l in _layouts(C) if l[0] != "odd"]:
            seed += 1
            rng = np.random.default_rng(seed)
            P, a, b = _rows_inputs(n, C, pbf, seed)
            Pd, P64 = _mk(P, pbf)
            site, zrows = _site(("null", "perm", "subset")[seed % 3], n, rng)
            subd, sub64 = _mk(rng.standard_normal(C), zbf)
            Z = _nan((zrows, zrow), zbf)
            _fwd(Pd, pbf, None if site is None else _t(site), n, C, _t(a), _t(b), Z, zbf, zrow, col0, sub=subd)
            relu = np.maximum(a.astype(np.float64) * P64 + b, 0.0)
            rows = np.arange(n) if site is None else site
            ref = R.rows_forward(P64, a, b, site, np.full((zrows, zrow), np.nan), zrow, col0, sub=sub64, z_bf16=zbf)[rows, col0:col0 + C]
            _check_map("rows_affine_relu_sub", Z, ref, R.elementwise_bound(a, P64, b, ref, zbf, mid=relu), rows, col0, C)
        addd, add64 = _mk(rng.standard_normal((n, C)), zbf)
        Z = _nan((n, C), zbf)
        _fwd(Pd, pbf, None, n, C, _t(a), _t(b), Z, zbf, C, 0, add=addd)
        ref = R.rows_forward(P64, a, b, add=add64, z_bf16=zbf)
        _check_map("rows_affine_relu_add", Z, ref, R.elementwise_bound(a, P64, b, ref, zbf, mid=relu), np.arange(n), 0, C)


@pytest.mark.parametrize("pbf", [False, True])
def test_sub_add_bf16_two_step_rounding_bit_for_bit(pbf):
    """Operands on a dyadic grid make a P + b exact in fp32, so Z must be round(round(relu) -/+ v) in bits: torch's bf16 ops on the CPU."""
    rng = np.random.default_rng(41)
    n, C = 257, 64
    kmax = 120 if pbf else 4000
    P = (rng.integers(-kmax, kmax + 1, (n, C)) / 64.0).astype(np.float32)
    a = rng.choice([-1.5, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0], C).astype(np.float32)
    b = (rng.integers(-64, 65, C) / 64.0).astype(np.float32)
    Pd, P64 = _mk(P, pbf)
    assert np.array_equal(P64, P.astype(np.float64))
    h = a.astype(np.float64) * P64 + b
    assert np.array_equal(h.astype(np.float32).astype(np.float64), h)                 # exact in fp32
    relu_bf = torch.from_numpy(np.maximum(h, 0).astype(np.float32)).bfloat16()
    assert (relu_bf.float().numpy() != np.maximum(h, 0)).any()                        # the first rounding does something
    v = torch.from_numpy(rng.standard_normal(C).astype(np.float32)).bfloat16()
    addv = torch.from_numpy(rng.standard_normal((n, C)).astype(np.float32)).bfloat16()
    Z = _nan((n, C), True)
    _fwd(Pd, pbf, None, n, C, _t(a), _t(b), Z, True, C, 0, sub=v.to(_dev()))
    assert torch.equal(Z.cpu().view(torch.int16), (relu_bf - v[None, :]).view(torch.int16))
    Z = _nan((n, C), True)
    _fwd(Pd, pbf, None, n, C, _t(a), _t(b), Z, True, C, 0, add=addv.to(_dev()))
    assert torch.equal(Z.cpu().view(torch.int16), (relu_bf + addv).view(torch.int16))


def test_sub_rejects_widths_outside_its_granularity():
    n, C = 5, 100
    Z = _nan((n, C))
    z = torch.zeros(n, C, device=_dev())
    with pytest.raises(L.GdmaeHipError):
        _fwd(z, False, None, n, C, z[0], z[0], Z, False, C, 0, sub=z[0])
    assert torch.isnan(Z).all()


# ------------------------------------------------------------------------------------------------------ backward
def _bwd_stats(Pd, pbf, site, n, C, a, b, dZ, zbf, zrow, col0, with_out):
    ws = _nan((512 * 3 * C,))
    assert ws.numel() * 4 == L.load().gdmae_rows_bwd_stats_workspace_bytes(C)
    out = _nan((3 * C,), dtype=torch.float64) if with_out else None
    L.call("gdmae_rows_bwd_stats", L.ptr(Pd), int(pbf), L.ptr(site), n, C, L.ptr(a), L.ptr(b), L.ptr(dZ), int(zbf), zrow, col0,
           L.ptr(out), L.ptr(ws), L.stream())
    return out, ws.view(512, 3, C)


def _coeffs(route, st, nblk, n_st, stats, ab, gamma, C, count, tot, start, acc):
    dg, db = (_t(start[0]), _t(start[1])) if start is not None else (_nan((C,)), _nan((C,)))
    c01 = _nan((2 * C,))
    if route == "rows":
        L.call("gdmae_bn_bwd_coeffs_rows", L.ptr(st), nblk, n_st, L.ptr(stats), L.ptr(ab), L.ptr(gamma), C, float(count), L.ptr(tot),
               L.ptr(dg), L.ptr(db), acc, L.ptr(c01), L.stream())
    else:
        L.call("gdmae_bn_bwd_coeffs", L.ptr(st), n_st, L.ptr(stats), L.ptr(ab), L.ptr(gamma), C, float(count), L.ptr(tot), L.ptr(dg),
               L.ptr(db), acc, L.ptr(c01), L.stream())
    return dg, db, c01


def _check_coeffs(name, sums, stats64, ab64, gamma, C, count, tot64, dev_out, start, acc):
    """the coefficient kernels are float64 arithmetic on the given sums and one fp32 rounding: 2 u |ref| + 1e-12 of the operands.
    The reference takes a = gamma rstd in float64; the kernels read the fp32 a for the mean's share of c0, which moves each of c0's
    two terms by one more rounding (2 u of their magnitudes)."""
    mean, r, b = stats64[:C], stats64[C:], ab64[C:]
    a = gamma.astype(np.float64) * r
    k = R.bn_coeffs(sums, mean, r, a, b, count, tot64)
    s_dg = (np.abs(sums[1]) + np.abs(mean * k["dbeta"])) * r
    s_c1 = np.abs(a) * r * s_dg / count
    s_c0 = np.abs(a * k["dbeta"]) / count + s_c1 * np.abs(mean)
    dg, db, c01 = (_f64(t) for t in dev_out)
    base = start if (acc and start is not None) else (np.zeros(C), np.zeros(C))
    _hold(f"{name} dgamma", dg, base[0] + k["dgamma"], 2 * R.U * (np.abs(k["dgamma"]) + np.abs(base[0])) + 1e-12 * s_dg)
    _hold(f"{name} dbeta", db, base[1] + k["dbeta"], 2 * R.U * (np.abs(k["dbeta"]) + np.abs(base[1])) + 1e-12 * np.abs(sums[0]))
    _hold(f"{name} c0", c01[:C], k["c0"], 2 * R.U * (np.abs(k["c0"]) + s_c0))
    _hold(f"{name} c1", c01[C:], k["c1"], 2 * R.U * np.abs(k["c1"]) + 1e-12 * s_c1)
    return k


def _backward_case(n, C, pbf, zbf, zrow, col0, kind, seed, full):
    rng = np.random.default_rng(seed)
    P, a, b = _rows_inputs(n, C, pbf, seed)
    Pd, P64 = _mk(P, pbf)
    site, zrows = _site(kind, n, rng)
    rows = np.arange(n) if site is None else site
    G = np.full((zrows, zrow), np.nan, np.float32)               # NaN wherever the kernel must not read
    G[rows, col0:col0 + C] = rng.standard_normal((n, C))
    dZ, G64 = _mk(G, zbf)
    G64 = G64[rows, col0:col0 + C]
    sd = None if site is None else _t(site)
    ad, bd = _t(a), _t(b)
    v8 = C % 8 == 0 and 256 % (C // 8) == 0 and zrow % 8 == 0 and col0 % 8 == 0
    name = f"rows_bwd_stats {'v8' if v8 else 'scalar'} P {'bf16' if pbf else 'fp32'} dZ {'bf16' if zbf else 'fp32'}"
    out, part = _bwd_stats(Pd, pbf, sd, n, C, ad, bd, dZ, zbf, zrow, col0, True)
    sums, dh = R.rows_backward_sums(P64, a, b, G64)
    nblk = R.bwd_stats_rows(n)
    assert nblk == L.load().gdmae_rows_bwd_stats_rows(n)
    ph = part.cpu().numpy()
    assert np.isfinite(ph[:nblk]).all() and np.isnan(ph[nblk:]).all()      # exactly rows_bwd_stats_rows(n) partial rows are written
    terms = (np.abs(dh).sum(0), np.abs(dh * P64).sum(0), np.abs(G64).sum(0))
    bounds = np.stack([np.maximum(R.sum_bound(t, n, nblk, R.bwd_stats_rpi(C, True)) if C % 8 == 0 else 0,
                                  R.sum_bound(t, n, nblk, R.bwd_stats_rpi(C, False))) for t in terms])
    o = _f64(out).reshape(3, C)
    for k, nm in enumerate(("sum dh", "sum dh P", "sum g")):
        _hold(f"{name} {nm}", o[k], sums[k], bounds[k])
    p64 = ph[:nblk].astype(np.float64)                                     # the float64 sums are the sums of those partial rows
    assert (np.abs(p64.sum(0) - o) <= 1e-13 * np.abs(p64).sum(0)).all()
    out2, part2 = _bwd_stats(Pd, pbf, sd, n, C, ad, bd, dZ, zbf, zrow, col0, False)        # out == NULL: partial rows only
    assert torch.equal(part2[:nblk], part[:nblk]) and torch.isnan(part2[nblk:]).all()
    # coefficients: statistics of P from the device's own fold (count > n with `tot`: an implicit dense map)
    gamma, beta = _affine(C)
    gd = _t(gamma)
    extra = 29
    for count, with_tot in ((n, False), (n + extra, True)) if full else ((n + extra, True),):
        stats, ab, _ = _fold(Pd, n, C, pbf, count, gd, _t(beta)) if (C % (8 if pbf else 4) == 0) else _fold_host(P64, C, count, gamma, beta)
        stats64, ab64 = _f64(stats), _f64(ab)
        tot64 = (o[2] + rng.standard_normal(C) * 3) if with_tot else None
        totd = _t(tot64) if with_tot else None
        if with_tot:
            assert (ab64[C:] > 0).any() and (ab64[C:] <= 0).any()           # the gate on `tot` sees both sides
        start = (rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32))
        for n_st in (2, 3):
            for acc in (0, 1):
                tt, t64 = (totd, tot64 if n_st == 3 else None)
                dev = _coeffs("f64", out, 0, n_st, stats, ab, gd, C, count, tt, start if acc else None, acc)
                k = _check_coeffs("bn_bwd_coeffs", o, stats64, ab64, gamma, C, count, t64, dev, start, acc)
                pr = part[:nblk, :n_st].contiguous()
                dev2 = _coeffs("rows", pr, nblk, n_st, stats, ab, gd, C, count, tt, start if acc else None, acc)
                _check_coeffs("bn_bwd_coeffs_rows", p64.sum(0), stats64, ab64, gamma, C, count, t64, dev2, start, acc)
    # dP from the device's own c0 | c1 and the kernel's own a | b
    c01 = dev[2]
    c64 = _f64(c01)
    refP = a.astype(np.float64) * dh + c64[:C] + c64[C:] * P64
    bnd = 2.0 ** -23 * (np.abs(a.astype(np.float64) * dh) + np.abs(c64[C:] * P64) + np.abs(c64[:C]))
    v8e = C % 8 == 0 and zrow % 8 == 0 and col0 % 8 == 0
    for obf in (False, True):
        dP = _nan((n, C), obf)
        L.call("gdmae_rows_bwd", L.ptr(Pd), int(pbf), L.ptr(sd), n, C, L.ptr(ad), L.ptr(bd), L.ptr(c01), c01[C:].data_ptr(), L.ptr(dZ),
               int(zbf), zrow, col0, L.ptr(dP), int(obf), L.stream())
        _hold(f"rows_bwd {'v8' if v8e else 'scalar'} P {'bf16' if pbf else 'fp32'} dZ {'bf16' if zbf else 'fp32'} dP {'bf16' if obf else 'fp32'}",
              _f64(dP), refP, bnd + (R.UB * np.abs(refP) if obf else 0))
    zero = (a.astype(np.float64) * P64 + b) == 0
    assert zero[:, 1].all() and (dh[zero] == 0).all()                      # no gradient at a pre-activation of exactly 0


def _fold_host(P64, C, count, gamma, beta):
    """statistics for widths the fold's 16-byte loads do not take (C = 100 in bf16): the reference's, in the device's formats."""
    f = R.fold(*R.colsums(P64), count, gamma.astype(np.float64), beta.astype(np.float64), EPS)
    return _t(np.concatenate([f["mean"], f["rstd"]])), _t(np.concatenate([f["a"], f["b"]]).astype(np.float32)), None


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("pbf,zbf", DT2)
def test_rows_bwd_stats_coeffs_and_rows_bwd(pbf, zbf, C):
    seed = 500
    lay = _layouts(C)
    for n in (1, 31, 32, 33, 1000):
        for lname, zrow, col0 in lay:
            for kind in ("null", "perm", "subset"):
                seed += 1
                _backward_case(n, C, pbf, zbf, zrow, col0, kind, seed, full=(n == 1000 and kind == "perm"))
    for (lname, zrow, col0), kind in ((lay[0], "null"), (lay[1], "perm"), (lay[-1], "subset")):     # empty trailing workgroups
        seed += 1
        _backward_case(16385, C, pbf, zbf, zrow, col0, kind, seed, full=False)


@pytest.mark.parametrize("n,C,zrow,col0,bf", [(66000, 256, 256, 0, True), (21001, 100, 104, 4, False)])
def test_rows_bwd_grid_stride(n, C, zrow, col0, bf):
    assert (n * C // 8 if (C % 8 == 0 and zrow % 8 == 0 and col0 % 8 == 0) else n * C) > 8192 * 256
    _backward_case(n, C, bf, bf, zrow, col0, "perm", 9, full=False)


def _chain_bounds(a, mean, r, k, B0, B1, count):
    """errors <= B0, B1 of the column sums {dh, dh x} carried through the BatchNorm chain rule (statistics and a are inputs here):
    -> bounds on dgamma, c1, c0.  Each result is one fp32 store (u), the fp32 a the coefficients are formed with differs from
    gamma rstd by one rounding (u on c1 and on each term of c0), hence 3 u of the magnitudes."""
    a = np.abs(np.asarray(a, np.float64))
    d_dg = (B1 + np.abs(mean) * B0) * r + 2 * R.U * np.abs(k["dgamma"])
    d_c1 = a * r * d_dg / count + 3 * R.U * np.abs(k["c1"])
    d_c0 = a * B0 / count + d_c1 * np.abs(mean) + 3 * R.U * (np.abs(k["c0"]) + a * np.abs(k["dbeta"]) / count + np.abs(k["c1"] * mean))
    return d_dg, d_c1, d_c0


# ====================================================================================================== segmented maximum
def _pillars(C, seed, total=0):
    """pillar sizes around the lane-group count G (each twice), four special pillars, then small ones up to ``total`` pillars."""
    sizes = []
    for s in R.pillar_sizes(C):
        sizes += [s, s]                                          # every second pillar: identical rows
    G = 64 // (C // 4)
    sizes += [G + 1, 2 * G + 1, 1, G + 2]                        # -inf first row, NaN first row, a lone -inf row, a dead pillar
    rng = np.random.default_rng(seed)
    sizes += list(rng.integers(1, 6, max(total - len(sizes), 0)))
    return sizes, R.make_pillars(sizes, seed)


def _first(pt_off, csr, p):
    return int(np.min(csr[pt_off[p]:pt_off[p + 1]]))


@pytest.mark.parametrize("C", [16, 32, 64, 128, 256])
def test_segment_max_every_width(C):
    sizes, (pt_off, csr, inv) = _pillars(C, 60 + C)
    M, N = len(sizes), len(inv)
    nreg = 2 * len(R.pillar_sizes(C))
    rng = np.random.default_rng(C)
    x = rng.standard_normal((N, C)).astype(np.float32)
    for p in range(1, nreg, 2):
        x[csr[pt_off[p]:pt_off[p + 1]]] = x[csr[pt_off[p]]]
    x[_first(pt_off, csr, nreg)] = -np.inf
    x[_first(pt_off, csr, nreg + 1), ::2] = np.nan
    x[_first(pt_off, csr, nreg + 2)] = -np.inf
    for p in range(M):                                           # the CSR is ascending inside a pillar and not pillar-major
        ids = csr[pt_off[p]:pt_off[p + 1]]
        assert (np.diff(ids) > 0).all()
    assert not np.array_equal(csr, np.arange(N))
    out, arg = _nan((M + 1, C)), torch.full((M + 1, C), -7, dtype=torch.int32, device=_dev())
    xd, pd, cd, invd = _t(x), _t(pt_off), _t(csr), _t(inv)
    L.call("gdmae_segment_max", L.ptr(xd), L.ptr(pd), L.ptr(cd), M, C, L.ptr(out), L.ptr(arg), L.stream())
    ro, ra = R.segment_max(x, pt_off, csr)
    oh, ah = out.cpu().numpy(), arg.cpu().numpy()
    assert np.array_equal(ah[:M], ra) and (ah[M] == -7).all() and np.isnan(oh[M]).all()
    assert np.array_equal(oh[:M].view(np.uint32), ro.astype(np.float32).view(np.uint32))
    for p in range(1, nreg, 2):
        assert (ah[p] == _first(pt_off, csr, p)).all()           # identical rows: the lowest point id, exactly
    assert (ah[nreg + 1, ::2] == _first(pt_off, csr, nreg + 1)).all() and np.isnan(oh[nreg + 1, ::2]).all()
    assert np.isfinite(oh[nreg]).all() == (sizes[nreg] > 1) and (oh[nreg + 2] == -np.inf).all()
    dout = rng.standard_normal((M, C)).astype(np.float32)
    dx = _nan((N + 1, C))
    dd = _t(dout)
    L.call("gdmae_segment_max_bwd", L.ptr(dd), L.ptr(arg), L.ptr(invd), N, C, L.ptr(dx), L.stream())
    dh = dx.cpu().numpy()
    assert np.array_equal(dh[:N], R.segment_max_bwd(dout, ra, inv, N).astype(np.float32)) and np.isnan(dh[N]).all()
    _REC["segment_max / segment_max_bwd (exact)"] = 0.0


def test_segment_max_grid_cap():
    M, C = 65540, 16                                             # 16 384 workgroups x 4 pillars < M: the grid-stride loop
    pt_off, csr, inv = R.make_pillars([1] * M, 3)
    x = np.random.default_rng(3).standard_normal((M, C)).astype(np.float32)
    out, arg = _nan((M, C)), torch.full((M, C), -7, dtype=torch.int32, device=_dev())
    xd, pd, cd = _t(x), _t(pt_off), _t(csr)
    L.call("gdmae_segment_max", L.ptr(xd), L.ptr(pd), L.ptr(cd), M, C, L.ptr(out), L.ptr(arg), L.stream())
    assert np.array_equal(out.cpu().numpy(), x[csr]) and np.array_equal(arg.cpu().numpy(), np.broadcast_to(csr[:, None], (M, C)))


def _segmax_affine(xd, xbf, pt_off, csr, M, C, a, b):
    out, arg = _nan((M + 1, C)), torch.full((M + 1, C), -7, dtype=torch.int32, device=_dev())
    pd, cd = _t(pt_off), _t(csr)
    L.call("gdmae_segment_max_affine", L.ptr(xd), int(xbf), L.ptr(pd), L.ptr(cd), M, C, L.ptr(a), L.ptr(b), L.ptr(out),
           L.ptr(arg), L.stream())
    assert np.isnan(out[M].cpu().numpy()).all() and (arg[M] == -7).all()
    return out[:M], arg[:M]


@pytest.mark.parametrize("xbf", [False, True])
@pytest.mark.parametrize("C", [64, 128, 256])
def test_segment_max_affine_exact_on_a_dyadic_grid(C, xbf):
    """x, a, b on a dyadic grid: relu(a x + b) is exact in fp32, so value and arg are compared exactly, ties included."""
    sizes, (pt_off, csr, inv) = _pillars(C, 70 + C)
    M, N = len(sizes), len(inv)
    nreg = 2 * len(R.pillar_sizes(C))
    rng = np.random.default_rng(C + xbf)
    x = (rng.integers(-100, 101, (N, C)) / 64.0).astype(np.float32)
    a = rng.choice([-1.5, -1.0, -0.5, 0.5, 1.0, 1.5, 2.0], C).astype(np.float32)
    b = (rng.integers(-64, 65, C) / 64.0).astype(np.float32)
    a[0], a[5], b[5], a[6], b[6] = -1.5, 0.0, -0.25, 0.0, 0.5    # a negative scale, a dead channel, a constant positive channel
    for p in range(1, nreg, 2):
        x[csr[pt_off[p]:pt_off[p + 1]]] = x[csr[pt_off[p]]]
    dead = nreg + 3
    x[csr[pt_off[dead]:pt_off[dead + 1]]] = -np.sign(a) * 4.0    # every relu(a x + b) of this pillar is 0
    xd, x64 = _mk(x, xbf)
    assert np.array_equal(x64, x.astype(np.float64))
    out, arg = _segmax_affine(xd, xbf, pt_off, csr, M, C, _t(a), _t(b))
    ro, ra = R.segment_max_affine(x64, a, b, pt_off, csr)
    assert np.array_equal(ro.astype(np.float32).astype(np.float64), ro)
    oh, ah = out.cpu().numpy(), arg.cpu().numpy()
    assert np.array_equal(oh, ro.astype(np.float32)) and np.array_equal(ah, ra)
    nz = np.arange(C) != 6
    assert (oh[dead][nz] == 0).all() and (ah[dead] == _first(pt_off, csr, dead)).all() and (oh[:, 6] == 0.5).all()
    for p in range(1, nreg, 2):
        assert (ah[p] == _first(pt_off, csr, p)).all()
    assert (oh[:, 5] == 0).all() and (ah[:, 5] == [_first(pt_off, csr, p) for p in range(M)]).all()
    _REC["segment_max_affine, dyadic grid (exact)"] = 0.0


SCALES = (1.0, 1e-3, 1e-6, 1e-9, 0.0)


def _segmax_bwd_case(C, xbf, seed, hand_made):
    """the max layer's backward on the device's own out / arg (hand_made: the reference's, for widths the forward does not take)."""
    sizes, (pt_off, csr, inv) = _pillars(C if not hand_made else 64, seed, total=1504)      # 47 partial rows of 32 pillars, all full
    M, N = len(sizes), len(inv)
    assert M == 1504 and R.bwd_stats_rows(M) * 32 == M
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, C)).astype(np.float32)
    xd, x64 = _mk(x, xbf)
    scale = np.array([SCALES[c % 5] for c in range(C)])
    gamma = (rng.uniform(0.8, 1.2, C) * np.where(np.arange(C) % 7 == 3, -1, 1) * scale).astype(np.float32)
    beta = rng.uniform(0.45, 0.55, C).astype(np.float32)
    f = R.fold(*R.colsums(x64), N, gamma.astype(np.float64), beta.astype(np.float64), EPS)
    a32, b32 = f["a"].astype(np.float32), f["b"].astype(np.float32)
    stats = _t(np.concatenate([f["mean"], f["rstd"]]))
    ab = _t(np.concatenate([a32, b32]))
    ad, bd, gd = _t(a32), _t(b32), _t(gamma)
    h32 = np.maximum(a32.astype(np.float64) * x64 + b32, 0.0).astype(np.float32)      # the fused multiply-add's fp32 result
    ro, ra = R._segmax_values(h32, pt_off, csr)
    if hand_made:
        out, arg = _t(ro.astype(np.float32)), _t(ra.astype(np.int32))
    else:
        out, arg = _segmax_affine(xd, xbf, pt_off, csr, M, C, ad, bd)
        _hold("segment_max_affine value", _f64(out), ro, 2.0 ** -23 * (np.abs(a32.astype(np.float64) * x64).max(0) + np.abs(b32)))
        assert np.array_equal(arg.cpu().numpy(), ra)
    oh, ah = _f64(out), arg.cpu().numpy()
    dout = rng.standard_normal((M, C)).astype(np.float32)
    dd, invd = _t(dout), _t(inv)
    sums, asums = R.segmax_affine_sums(x64, oh, ah, dout)
    nblk = R.bwd_stats_rows(M)
    b0 = np.maximum(R.sum_bound(asums[0], M, nblk, R.bwd_stats_rpi(C, False)),
                    R.sum_bound(asums[0], M, nblk, R.bwd_stats_rpi(C, True)) if C % 8 == 0 else 0)
    b1 = np.maximum(R.sum_bound(asums[1], M, nblk, R.bwd_stats_rpi(C, False), R.RECON),
                    R.sum_bound(asums[1], M, nblk, R.bwd_stats_rpi(C, True), R.RECON) if C % 8 == 0 else 0)
    mean, r = f["mean"], f["rstd"]
    kref = R.bn_coeffs(sums, mean, r, a32.astype(np.float64), b32, N)
    # the sum bounds carried through the chain rule (statistics and a are the kernels' inputs here, so only the sums err)
    d_dg, d_c1, d_c0 = _chain_bounds(a32, mean, r, kref, b0, b1, N)
    dh = R.segmax_affine_dh(oh, ah, dout, inv, N)
    for route in ("a, b given", "a, b null"):
        st = _nan((2 * C,), dtype=torch.float64)
        ws = _ws(L.load().gdmae_rows_bwd_stats_workspace_bytes(C))
        given = route == "a, b given"
        L.call("gdmae_segmax_bwd_stats", L.ptr(xd), int(xbf), L.ptr(out), L.ptr(arg), L.ptr(dd), M, C, L.ptr(ad) if given else None,
               L.ptr(bd) if given else None, L.ptr(st), L.ptr(ws), L.stream())
        st2 = _nan((2 * C,), dtype=torch.float64)
        L.call("gdmae_segmax_bwd_stats", L.ptr(xd), int(xbf), L.ptr(out), L.ptr(arg), L.ptr(dd), M, C, L.ptr(ad) if given else None,
               L.ptr(bd) if given else None, L.ptr(st2), L.ptr(ws), L.stream())
        assert torch.equal(st, st2)
        sh = _f64(st).reshape(2, C)
        dg, db, c01 = _coeffs("f64", st, 0, 2, stats, ab, gd, C, N, None, None, 0)
        c64 = _f64(c01)
        dxs = {}
        for obf in (False, True):
            dx = _nan((N + 1, C), obf)
            L.call("gdmae_segmax_bn_bwd", L.ptr(xd), int(xbf), L.ptr(out), L.ptr(arg), L.ptr(dd), L.ptr(invd), N, C, L.ptr(ad), L.ptr(c01),
                   c01[C:].data_ptr(), L.ptr(dx), int(obf), L.stream())
            assert torch.isnan(dx[N]).all()
            dxs[obf] = _f64(dx[:N])
        ref_dx = a32.astype(np.float64) * dh + kref["c0"] + kref["c1"] * x64
        b_dx = d_c0 + np.abs(x64) * d_c1 + 2.0 ** -23 * (np.abs(a32 * dh) + np.abs(kref["c1"] * x64) + np.abs(kref["c0"]))
        tag = f"segmax_bwd_stats ({route}, x {'bf16' if xbf else 'fp32'})"
        ratios = {}
        for s in SCALES:                                          # every scale is held to the same bounds; recorded per scale
            m = scale == s
            tiny = 1e-300
            q = [np.max(np.abs(sh[1] - sums[1])[m] / (b1[m] + tiny)), np.max(np.abs(_f64(dg) - kref["dgamma"])[m] / (d_dg[m] + tiny)),
                 np.max(np.abs(c64[:C] - kref["c0"])[m] / (d_c0[m] + tiny)), np.max(np.abs(c64[C:] - kref["c1"])[m] / (d_c1[m] + tiny)),
                 np.max((np.abs(dxs[False] - ref_dx) / (b_dx + tiny))[:, m])]
            key = f"gamma x {s:g}, {route}"
            _SMALL[key] = [max(u, v) for u, v in zip(_SMALL.get(key, [0] * 5), q)]
            ratios[s] = q
        print(tag, {s: [f"{v:.3f}" for v in q] for s, q in ratios.items()})
        _hold(f"{tag} sum dh", sh[0], sums[0], b0)
        _hold(f"{tag} sum dh x", sh[1], sums[1], b1)
        _hold(f"{tag} -> dgamma", _f64(dg), kref["dgamma"], d_dg)
        _hold(f"{tag} -> dbeta", _f64(db), kref["dbeta"], b0 + 2 * R.U * np.abs(kref["dbeta"]))
        _hold(f"{tag} -> c0", c64[:C], kref["c0"], d_c0)
        _hold(f"{tag} -> c1", c64[C:], kref["c1"], d_c1)
        _hold(f"segmax_bn_bwd ({route}) dx fp32", dxs[False], ref_dx, b_dx)
        _hold(f"segmax_bn_bwd ({route}) dx bf16", dxs[True], ref_dx, b_dx * (1 + R.UB) + R.UB * np.abs(ref_dx))
        # the elementwise kernel alone, on the device's own c0 | c1
        own = a32.astype(np.float64) * dh + c64[:C] + c64[C:] * x64
        own_b = 2.0 ** -23 * (np.abs(a32 * dh) + np.abs(c64[C:] * x64) + np.abs(c64[:C]))
        _hold(f"segmax_bn_bwd {'v8' if C % 8 == 0 else 'scalar'} alone, dx fp32", dxs[False], own, own_b)
        _hold(f"segmax_bn_bwd {'v8' if C % 8 == 0 else 'scalar'} alone, dx bf16", dxs[True], own, own_b + R.UB * np.abs(own))
    dead = (oh <= 0)
    assert (dh[ah[dead], np.nonzero(dead)[1]] == 0).all()


@pytest.mark.parametrize("xbf", [False, True])
@pytest.mark.parametrize("C", [64, 128, 256])
def test_segmax_affine_backward_all_scales(C, xbf):
    _segmax_bwd_case(C, xbf, 80 + C + xbf, hand_made=False)


@pytest.mark.parametrize("xbf", [False, True])
@pytest.mark.parametrize("C", [48, 100])
def test_segmax_backward_scalar_twins(C, xbf):
    _segmax_bwd_case(C, xbf, 90 + C + xbf, hand_made=True)


# ====================================================================================================== row movers
@pytest.mark.parametrize("rb", [16, 96, 256, 768])
def test_gather_scatter_fill_exact(rb):
    rng = np.random.default_rng(rb)
    T, n = 700, 1000
    dev = _dev()
    for trb, col in ((rb, 0), (3 * rb, 0), (3 * rb, rb), (3 * rb, 2 * rb)):
        tab = rng.integers(0, 256, (T, trb)).astype(np.uint8)
        idx = rng.integers(-1, T, n).astype(np.int32)
        idx[::17] = -1
        out = torch.full((n + 1, rb), 0xAB, dtype=torch.uint8, device=dev)
        td, idd = _t(tab), _t(idx)
        if trb == rb:
            L.call("gdmae_gather_rows", L.ptr(td), L.ptr(idd), n, rb, L.ptr(out), L.stream())
        else:
            L.call("gdmae_gather_rows_strided", L.ptr(td), L.ptr(idd), n, rb, trb, col, L.ptr(out), L.stream())
        oh = out.cpu().numpy()
        assert np.array_equal(oh[:n], R.gather_rows(tab, idx, col, rb)) and (oh[n] == 0xAB).all()
        src = rng.integers(0, 256, (n, rb)).astype(np.uint8)
        sidx = np.full(n, -1, np.int32)
        pick = rng.choice(n, T // 2, replace=False)
        sidx[pick] = rng.permutation(T)[:T // 2]
        dst0 = rng.integers(0, 256, (T, trb)).astype(np.uint8)
        dst, srcd, sidd = _t(dst0), _t(src), _t(sidx)
        if trb == rb:
            L.call("gdmae_scatter_rows", L.ptr(srcd), L.ptr(sidd), n, rb, L.ptr(dst), L.stream())
        else:
            L.call("gdmae_scatter_rows_strided", L.ptr(srcd), L.ptr(sidd), n, rb, trb, col, L.ptr(dst), L.stream())
        assert np.array_equal(dst.cpu().numpy(), R.scatter_rows(src, sidx, dst0, col))
        keep = dst.clone()                                       # n = 0 returns without touching anything
        L.call("gdmae_gather_rows_strided", L.ptr(td), L.ptr(idd), 0, rb, trb, col, L.ptr(out), L.stream())
        L.call("gdmae_scatter_rows_strided", L.ptr(srcd), L.ptr(sidd), 0, rb, trb, col, L.ptr(dst), L.stream())
        assert torch.equal(dst, keep) and np.array_equal(out.cpu().numpy(), oh)
    _REC["gather_rows / scatter_rows (_strided) (exact)"] = 0.0


def test_gather_scatter_grid_stride():
    rng = np.random.default_rng(8)
    T, n, rb = 90001, 90000, 768                                 # n x 48 vectors > 16 384 workgroups x 256 threads
    assert n * rb // 16 > 16384 * 256
    tab = _t(rng.integers(0, 256, (T, rb)).astype(np.uint8))
    idx = rng.permutation(T)[:n].astype(np.int32)
    idx[::5] = -1
    idd = _t(idx)
    out = torch.full((n, rb), 0xAB, dtype=torch.uint8, device=_dev())
    L.call("gdmae_gather_rows", L.ptr(tab), L.ptr(idd), n, rb, L.ptr(out), L.stream())
    sel = torch.from_numpy(np.maximum(idx, 0).astype(np.int64)).to(_dev())
    ok = torch.from_numpy(idx >= 0).to(_dev())
    assert torch.equal(out, torch.where(ok[:, None], tab[sel], torch.zeros_like(out)))
    dst = torch.full((T, rb), 0xCD, dtype=torch.uint8, device=_dev())
    L.call("gdmae_scatter_rows", L.ptr(out), L.ptr(idd), n, rb, L.ptr(dst), L.stream())
    ref = torch.full((T, rb), 0xCD, dtype=torch.uint8, device=_dev())
    ref[sel[ok]] = out[ok]
    assert torch.equal(dst, ref)


@pytest.mark.parametrize("R_,rb", [(1, 16384), (3, 768), (5000001, 16), (70000, 768)])
def test_fill_rows(R_, rb):
    blocks = (R_ * (rb // 16) + 255) // 256
    assert (blocks > 16384) == (R_ == 5000001)                   # both sides of the 16 384-workgroup cap
    v = torch.from_numpy(np.random.default_rng(rb).integers(1, 255, rb).astype(np.uint8)).to(_dev())
    Z = torch.zeros(R_ + 1, rb, dtype=torch.uint8, device=_dev())
    for C, eb in ((rb // 2, 2), (rb // 4, 4)):
        Z.zero_()
        L.call("gdmae_fill_rows", L.ptr(v), R_, C, eb, L.ptr(Z), L.stream())
        assert bool((Z[:R_] == v[None, :]).all()) and bool((Z[R_] == 0).all())
    L.call("gdmae_fill_rows", L.ptr(v), 0, rb // 2, 2, L.ptr(Z[R_:]), L.stream())
    assert bool((Z[R_] == 0).all())
    _REC["fill_rows (exact)"] = 0.0


# ====================================================================================================== autograd wrappers
def _module(C, seed):
    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=MOM).to(_dev()).train()
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        bn.weight.copy_(_t((rng.uniform(0.5, 1.5, C) * np.where(rng.random(C) < 0.3, -1, 1)).astype(np.float32)))
        bn.bias.copy_(_t(rng.uniform(-0.5, 0.5, C).astype(np.float32)))
        bn.running_mean.copy_(_t(rng.standard_normal(C).astype(np.float32)))
        bn.running_var.copy_(_t(rng.uniform(0.5, 2, C).astype(np.float32)))
    return bn


def _check_module_stats(tag, bn, rm0, rv0, x64, n, bf):
    C = x64.shape[1]
    s1, s2 = R.colsums(x64)
    nblk, rpi = R.colstats_rows(n), R.colstats_rpi(C, bf)
    b1, b2 = R.sum_bound(np.abs(x64).sum(0), n, nblk, rpi), R.sum_bound(s2, n, nblk, rpi)
    g64, be64 = _f64(bn.weight), _f64(bn.bias)
    ref = R.fold(s1, s2, n, g64, be64, EPS, MOM, rm0, rv0, 0)
    fb = R.fold_bounds(None, None, b1, b2, s1, s2, n, g64, be64, EPS)
    unbf = n / (n - 1.0)
    _hold(f"{tag} running_mean", _f64(bn.running_mean), ref["running_mean"], MOM * fb["mean32"] + 4 * R.U * (np.abs(rm0) + MOM * np.abs(ref["mean"])))
    _hold(f"{tag} running_var", _f64(bn.running_var), ref["running_var"], MOM * unbf * fb["var32"] + 4 * R.U * (np.abs(rv0) + MOM * unbf * ref["var"]))
    assert int(bn.num_batches_tracked.item()) == 1
    return ref, fb


def _rows_chain(tag, x64, g64, ab64, stats64, n, bf, out, dx, dgamma, dbeta):
    """out (None: checked by the caller), dx, dgamma, dbeta of one BatchNorm+ReLU over rows against the composed reference, from the
    device's own a | b and statistics."""
    C = x64.shape[1]
    a, b = ab64[:C], ab64[C:]
    ref = np.maximum(a * x64 + b, 0.0)
    if out is not None:
        _hold(f"{tag} out", out, ref, R.elementwise_bound(a, x64, b, ref, bf))
    k = R.rows_backward(x64, a, b, g64, stats64[:C], stats64[C:], n)
    nblk = R.bwd_stats_rows(n)
    rpi = R.bwd_stats_rpi(C, True)
    dh = np.where(a * x64 + b > 0, g64, 0.0)
    B0, B1 = R.sum_bound(np.abs(dh).sum(0), n, nblk, rpi), R.sum_bound(np.abs(dh * x64).sum(0), n, nblk, rpi)
    mean, r = stats64[:C], stats64[C:]
    d_dg, d_c1, d_c0 = _chain_bounds(a, mean, r, k, B0, B1, n)
    _hold(f"{tag} dgamma", dgamma, k["dgamma"], d_dg)
    _hold(f"{tag} dbeta", dbeta, k["dbeta"], B0 + 2 * R.U * np.abs(k["dbeta"]))
    b_dx = d_c0 + np.abs(x64) * d_c1 + 2.0 ** -23 * (np.abs(a * dh) + np.abs(k["c1"] * x64) + np.abs(k["c0"]))
    _hold(f"{tag} dx", dx, k["dP"], b_dx * (1 + R.UB) + R.UB * np.abs(k["dP"]) if bf else b_dx)     # the rounded value carries b_dx too


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("N,C", [(1237, 64), (333, 256)])
@pytest.mark.parametrize("residual", [False, True])
def test_wrapper_bn_relu_rows(N, C, bf, residual):
    rng = np.random.default_rng(N + C)
    bn = _module(C, N)
    rm0, rv0 = _f64(bn.running_mean), _f64(bn.running_var)
    xd, x64 = _mk(rng.standard_normal((N, C)) * rng.uniform(0.3, 2, C) + rng.uniform(-1, 1, C), bf)
    gd, g64 = _mk(rng.standard_normal((N, C)), bf)
    rd, r64 = _mk(rng.standard_normal((N, C)), bf)
    stats, ab, _ = gbn.fold(xd, N, bn.weight.detach(), bn.bias.detach(), EPS)         # the statistics the wrapper will use (bit-repeatable)
    xd.requires_grad_(True)
    rd.requires_grad_(residual)
    out, mean, var = gvfe.BNReLURows.apply(xd, bn.weight, bn.bias, EPS, bn, rd if residual else None)
    out.backward(gd)
    tag = f"BNReLURows{' + residual' if residual else ''} {'bf16' if bf else 'fp32'}"
    ref, fb = _check_module_stats(tag, bn, rm0, rv0, x64, N, bf)
    _hold(f"{tag} mean", _f64(mean), ref["mean"], fb["mean32"])
    _hold(f"{tag} var", _f64(var), ref["var"], fb["var32"])
    _hold(f"{tag} a", _f64(ab)[:C], ref["a"], fb["a"])
    _hold(f"{tag} b", _f64(ab)[C:], ref["b"], fb["b"])
    ab64, st64 = _f64(ab), _f64(stats)
    o64 = _f64(out)
    if residual:
        y = np.maximum(ab64[:C] * x64 + ab64[C:], 0.0)
        want = R.rows_forward(x64, ab64[:C], ab64[C:], add=r64, z_bf16=bf)
        _hold(f"{tag} out", o64, want, R.elementwise_bound(ab64[:C], x64, ab64[C:], want, bf, mid=y))
        assert torch.equal(rd.grad, gd)                          # the shortcut's gradient is the output gradient
        o64 = None
    _rows_chain(tag, x64, g64, ab64, st64, N, bf, o64, _f64(xd.grad), _f64(bn.weight.grad), _f64(bn.bias.grad))


@pytest.mark.parametrize("bf", [False, True])
def test_wrapper_bn_relu_rows_cat(bf):
    N, widths = 1237, (64, 128, 64)
    rng = np.random.default_rng(77)
    bns = [_module(C, 10 + i) for i, C in enumerate(widths)]
    rm0 = [(_f64(m.running_mean), _f64(m.running_var)) for m in bns]
    xs = [_mk(rng.standard_normal((N, C)) * rng.uniform(0.3, 2, C) + rng.uniform(-1, 1, C), bf) for C in widths]
    gd, g64 = _mk(rng.standard_normal((N, sum(widths))), bf)
    folds = [gbn.fold(x, N, m.weight.detach(), m.bias.detach(), EPS) for (x, _), m in zip(xs, bns)]
    args = []
    for (x, _), m in zip(xs, bns):
        x.requires_grad_(True)
        args += [x, m.weight, m.bias]
    out = gvfe.BNReLURowsCat.apply(bns, EPS, *args)
    assert out.shape == (N, sum(widths)) and out.dtype == xs[0][0].dtype
    out.backward(gd)
    o64, col = _f64(out), 0
    for i, C in enumerate(widths):
        tag = f"BNReLURowsCat block {i} ({C}) {'bf16' if bf else 'fp32'}"
        ref, fb = _check_module_stats(tag, bns[i], rm0[i][0], rm0[i][1], xs[i][1], N, bf)
        stats, ab, _ = folds[i]
        _hold(f"{tag} a", _f64(ab)[:C], ref["a"], fb["a"])
        _hold(f"{tag} b", _f64(ab)[C:], ref["b"], fb["b"])
        _rows_chain(tag, xs[i][1], g64[:, col:col + C], _f64(ab), _f64(stats), N, bf, o64[:, col:col + C], _f64(xs[i][0].grad),
                    _f64(bns[i].weight.grad), _f64(bns[i].bias.grad))
        col += C


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("N,C", [(1237, 64), (333, 256)])
def test_wrapper_bn_relu_segment_max(N, C, bf):
    rng = np.random.default_rng(N + C + 1)
    sizes = []
    while sum(sizes) < N:
        sizes.append(int(min(rng.integers(1, 40), N - sum(sizes))))
    pt_off, csr, inv = R.make_pillars(sizes, 5)
    M = len(sizes)
    bn = _module(C, N + 1)
    rm0, rv0 = _f64(bn.running_mean), _f64(bn.running_var)
    xd, x64 = _mk(rng.standard_normal((N, C)) * rng.uniform(0.3, 2, C) + rng.uniform(-1, 1, C), bf)
    dout = rng.standard_normal((M, C)).astype(np.float32)
    stats, ab, _ = gbn.fold(xd, N, bn.weight.detach(), bn.bias.detach(), EPS)
    xd.requires_grad_(True)
    out, mean, var = gvfe.BNReLUSegmentMax.apply(xd, bn.weight, bn.bias, EPS, _t(pt_off), _t(csr), _t(inv), bn)
    out.backward(_t(dout))
    tag = f"BNReLUSegmentMax {'bf16' if bf else 'fp32'}"
    ref, fb = _check_module_stats(tag, bn, rm0, rv0, x64, N, bf)
    _hold(f"{tag} mean", _f64(mean), ref["mean"], fb["mean32"])
    _hold(f"{tag} var", _f64(var), ref["var"], fb["var32"])
    ab64, st64 = _f64(ab), _f64(stats)
    a, b = ab64[:C], ab64[C:]
    h32 = np.maximum(a * x64 + b, 0.0).astype(np.float32)
    ro, ra = R._segmax_values(h32, pt_off, csr)
    _hold(f"{tag} out", _f64(out), ro, 2.0 ** -23 * (np.abs(a * x64).max(0) + np.abs(b)))
    oh = _f64(out)
    sums, asums = R.segmax_affine_sums(x64, oh, ra, dout)
    nblk, rpi = R.bwd_stats_rows(M), R.bwd_stats_rpi(C, True)
    B0, B1 = R.sum_bound(asums[0], M, nblk, rpi), R.sum_bound(asums[1], M, nblk, rpi, R.RECON)
    mean64, r = st64[:C], st64[C:]
    k = R.bn_coeffs(sums, mean64, r, a, b, N)
    d_dg, d_c1, d_c0 = _chain_bounds(a, mean64, r, k, B0, B1, N)
    dh = R.segmax_affine_dh(oh, ra, dout, inv, N)
    ref_dx = a * dh + k["c0"] + k["c1"] * x64
    b_dx = d_c0 + np.abs(x64) * d_c1 + 2.0 ** -23 * (np.abs(a * dh) + np.abs(k["c1"] * x64) + np.abs(k["c0"]))
    _hold(f"{tag} dgamma", _f64(bn.weight.grad), k["dgamma"], d_dg)
    _hold(f"{tag} dbeta", _f64(bn.bias.grad), k["dbeta"], B0 + 2 * R.U * np.abs(k["dbeta"]))
    _hold(f"{tag} dx", _f64(xd.grad), ref_dx, b_dx * (1 + R.UB) + R.UB * np.abs(ref_dx) if bf else b_dx)
