"""Plain float64 reference of one sparse-convolution block (SubMConv2d / SparseConv2d k3 -> BatchNorm1d(train) -> ReLU, forward and
backward) on crafted scenes.  NumPy / torch only; imports no project kernel.

Scenes.  ``scene(kind, n_target, seed)`` -> ``(nbr, nbr_t, n_in, n_out)`` for ``kind`` in {"subm", "down"} on a B = 2 grid.  The
rulebooks follow the relations written down at the top of ``tests/plan_reference.py``: tokens in ascending linear key
``(b * Y + y) * X + x``; ``nbr_subm[t, 3 ky + kx]`` = token at ``(y + ky - 1, x + kx - 1)`` and its tap-flipped copy as the transpose;
``nbr_down[o, k]`` = input at ``2 o - 1 + k`` and ``nbr_down_t`` its exact inverse (``nbr_t[i, k] = o  iff  nbr[o, k] = i``).  The
module asserts that inverse relation for every scene it builds.

The grid is 48 x 40 where the requested row count fits it with room to spare, and grows in whole multiples (96 x 80, ...) for the row
counts of the large cases, so that the occupancy stays between a quarter and a half.  Every scene holds

* a fully dense 3 x 3 patch (a row with all nine taps),
* isolated sites (a row with the centre tap only),
* a checkerboard patch (a row whose only taps are the diagonal ones and the centre),
* occupied cells on both sides of the batch seam (last grid row of batch 0, first grid row of batch 1, same column) - they must not
  become neighbours,
* complete first and last grid rows and columns in both batches,

and random sites that bring the row count to ``n_target`` exactly (``n_out`` for "subm", ``n_in`` for "down").  Complete border lines
of two batches need 2 (2 X + 2 Y - 4) sites, which a scene of fewer rows cannot hold: scenes under 400 rows use a 12 x 10 grid (border:
80 sites) and scenes under 110 rows (the 33- and 65-row cases) leave the border lines out; ``scene_full(...)["features"]`` says which
features a scene holds, and tests/test_conv_block_reference_cpu.py asserts them per scene.

``reference`` places the roundings where the block does (see its docstring); ``CASES`` / ``make_inputs`` are the block cases shared by
the CPU power check and tests/test_conv_block_gpu.py.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from plan_reference import _lookup

B = 2
FEATURES_SMALL = ("dense", "isolated", "checkerboard", "seam")
FEATURES_ALL = FEATURES_SMALL + ("border",)
DIAG = (0, 2, 4, 6, 8)


def _grid(n_target, m):
    if m is None:
        m = 0 if n_target < 400 else max(1, math.ceil(math.sqrt(n_target / (0.45 * B * 48 * 40))))
    return (12, 10) if m == 0 else (48 * m, 40 * m)


def assert_inverse(nbr, nbr_t, n_in):
    """nbr_t[i, k] = o  iff  nbr[o, k] = i: the two tables list the same (o, k, i) triples, each once."""
    assert nbr_t.shape == (n_in, 9) and nbr.shape[1] == 9
    o, k = np.nonzero(nbr >= 0)
    fwd = np.stack([o, k, nbr[o, k]], axis=1)
    i, k2 = np.nonzero(nbr_t >= 0)
    bwd = np.stack([nbr_t[i, k2], k2, i], axis=1)
    assert len(fwd) == len(bwd)
    key = lambda a: np.sort((a[:, 0] * 9 + a[:, 1]) * (n_in + 1) + a[:, 2])          # noqa: E731
    assert np.array_equal(key(fwd), key(bwd)), "nbr_t is not the inverse relation of nbr"
    assert nbr.max(initial=-1) < n_in and nbr_t.max(initial=-1) < nbr.shape[0]


def scene_full(kind, n_target, seed, m=None):
    """-> dict: nbr (n_out, 9), nbr_t (n_in, 9) int64, n_in, n_out, Y, X (input grid), idx_in / idx_out (n, 3) (b, y, x), features."""
    assert kind in ("subm", "down")
    Y, X = _grid(n_target, m)
    rng = np.random.default_rng(seed)
    occ = np.zeros((B, Y, X), dtype=bool)
    keep_empty = np.zeros((B, Y, X), dtype=bool)
    # dense patch, rows / columns 3..5 of batch 0: the window of output (2, 2) of the strided convolution, centre (4, 4) for the submanifold one
    occ[0, 3:6, 3:6] = True
    # checkerboard patch, rows 7..9 / columns 3..5 of batch 0 inside an empty ring: the window of output (4, 2), centre (8, 4)
    keep_empty[0, 6:11, 2:7] = True
    for dy in range(3):
        for dx in range(3):
            if (dy + dx) % 2 == 0:
                occ[0, 7 + dy, 3 + dx] = True
    # isolated sites of batch 1 at even coordinates (the centre of an output window), each inside an empty ring
    for (y, x) in ((4, 4), (8, 6)):
        keep_empty[1, y - 1:y + 2, x - 1:x + 2] = True
        occ[1, y, x] = True
    # the batch seam
    occ[0, Y - 1, 5] = True
    occ[1, 0, 5] = True
    features = list(FEATURES_SMALL)
    border = 2 * (2 * X + 2 * Y - 4)
    if n_target >= int(occ.sum()) + border + 12:
        occ[:, 0, :] = occ[:, Y - 1, :] = True
        occ[:, :, 0] = occ[:, :, X - 1] = True
        features.append("border")
    keep_empty &= ~occ
    need = n_target - int(occ.sum())
    free = np.flatnonzero(~occ.reshape(-1) & ~keep_empty.reshape(-1))
    assert 0 <= need <= len(free), f"scene({kind}, {n_target}): {int(occ.sum())} crafted sites, {len(free)} free cells"
    occ.reshape(-1)[rng.choice(free, size=need, replace=False)] = True
    idx = np.argwhere(occ).astype(np.int64)                                     # ascending (b, y, x) = ascending linear key
    n_in = len(idx)
    assert n_in == n_target
    cmap = -np.ones(B * Y * X, dtype=np.int64)
    cmap[(idx[:, 0] * Y + idx[:, 1]) * X + idx[:, 2]] = np.arange(n_in)
    if kind == "subm":
        nbr = -np.ones((n_in, 9), dtype=np.int64)
        for k in range(9):
            nbr[:, k] = _lookup(cmap, B, Y, X, idx[:, 0], idx[:, 1] + k // 3 - 1, idx[:, 2] + k % 3 - 1)
        nbr_t = nbr[:, ::-1].copy()
        oidx = idx
    else:
        Yo, Xo = (Y - 1) // 2 + 1, (X - 1) // 2 + 1
        act = np.zeros((B, Yo, Xo), dtype=bool)
        for k in range(9):                                                     # in = 2 o - 1 + k  ->  o = (in + 1 - k) / 2
            ny, nx = idx[:, 1] + 1 - k // 3, idx[:, 2] + 1 - k % 3
            ok = (ny % 2 == 0) & (nx % 2 == 0) & (ny >= 0) & (nx >= 0) & (ny // 2 < Yo) & (nx // 2 < Xo)
            act[idx[ok, 0], ny[ok] // 2, nx[ok] // 2] = True
        oidx = np.argwhere(act).astype(np.int64)
        nbr = -np.ones((len(oidx), 9), dtype=np.int64)
        for k in range(9):
            nbr[:, k] = _lookup(cmap, B, Y, X, oidx[:, 0], 2 * oidx[:, 1] - 1 + k // 3, 2 * oidx[:, 2] - 1 + k % 3)
        nbr_t = -np.ones((n_in, 9), dtype=np.int64)
        o, k = np.nonzero(nbr >= 0)
        nbr_t[nbr[o, k], k] = o
    assert (nbr >= 0).any(axis=1).all()
    assert_inverse(nbr, nbr_t, n_in)
    return {"nbr": nbr, "nbr_t": nbr_t, "n_in": n_in, "n_out": len(oidx), "Y": Y, "X": X, "idx_in": idx, "idx_out": oidx,
            "features": tuple(features), "kind": kind}


def scene(kind, n_target, seed, m=None):
    s = scene_full(kind, n_target, seed, m)
    return s["nbr"], s["nbr_t"], s["n_in"], s["n_out"]


def scene_feature_report(s):
    """Which of the crafted features the rulebook of a scene really holds (read off the rulebook, not off the construction)."""
    nbr, idx_in, idx_out, Y, X = s["nbr"], s["idx_in"], s["idx_out"], s["Y"], s["X"]
    taps = nbr >= 0
    sets = {tuple(np.flatnonzero(r)) for r in taps}
    rep = {"dense": tuple(range(9)) in sets, "isolated": (4,) in sets, "checkerboard": DIAG in sets}
    cell = lambda b, y, x: bool(((idx_in[:, 0] == b) & (idx_in[:, 1] == y) & (idx_in[:, 2] == x)).any())      # noqa: E731
    cols = [x for x in range(X) if cell(0, Y - 1, x) and cell(1, 0, x)]
    src_b = idx_in[np.clip(nbr, 0, None), 0]
    same_batch = bool(np.all((src_b == idx_out[:, None, 0]) | ~taps))
    rep["seam"] = bool(cols) and same_batch
    line = lambda sel: int(sel.sum())                                                                           # noqa: E731
    rep["border"] = all(line((idx_in[:, 0] == b) & (idx_in[:, 1] == y)) == X for b in range(B) for y in (0, Y - 1)) and \
        all(line((idx_in[:, 0] == b) & (idx_in[:, 2] == x)) == Y for b in range(B) for x in (0, X - 1))
    return rep


# ------------------------------------------------------------------------------------------------------------------------------
# the block
# ------------------------------------------------------------------------------------------------------------------------------
def bf16_round(t):
    return t.float().bfloat16().to(t.dtype)


def reference(x, W, gamma, beta, eps, nbr, g, y=None, out=None, *, out_f32=False, rounding=True, dtype=torch.float64):
    """One conv block, forward and backward, in ``dtype`` (float64; float32 = the emulation of the kernels' own arithmetic).

    x (n_in, cin), W (cout, 3, 3, cin), gamma / beta (cout), nbr (n_out, 9), g (n_out, cout) upstream gradient.  The reference reads what
    the kernels read - bf16-rounded x and W, fp32 gamma / beta - and rounds where the block rounds:
        y = bf16(sum_k W_k x[nbr[:, k]]);  mean, biased var over the ROUNDED y, count = n_out;  a = gamma rstd, b = beta - a mean;
        out = relu(a y + b), bf16 unless out_f32;  dh = g [out > 0];  dgamma = sum dh xhat, dbeta = sum dh;
        dy = bf16(a (dh - dbeta / n - xhat dgamma / n));  dW_k = dy^T x[nbr[:, k]];  dx = bf16(sum_k dy[nbr_t[:, k]] W_k)
    (dx is formed by scattering through ``nbr``: the transposed rulebook is the kernels' business).  ``rounding=False``: no bf16 rounding
    anywhere (the fp32 library route, and the comparison with autograd).  ``y`` / ``out``: the kernel's own saved buffers - the later
    stages start from them, so ReLU-mask and statistic differences do not leak into the gradient checks.
    Returns a dict; ``y_exact`` is the unrounded sum and ``S_abs`` = sum |x| |W| per output element."""
    rd = bf16_round if rounding else (lambda t: t)
    dev = x.device
    cout, cin = W.shape[0], W.shape[3]
    xd = rd(x.to(dtype))
    Wd = rd(W.to(dtype)).reshape(cout, 9, cin)
    gamma, beta, g = gamma.to(dtype), beta.to(dtype), g.to(dtype)
    nb = torch.as_tensor(nbr, device=dev).long()
    has = nb >= 0
    src = nb.clamp_min(0)
    n_out, n_in = nb.shape[0], x.shape[0]
    y_exact = torch.zeros(n_out, cout, dtype=dtype, device=dev)
    S_abs = torch.zeros_like(y_exact)
    for k in range(9):
        rows = xd[src[:, k]] * has[:, k, None]
        y_exact += rows @ Wd[:, k].t()
        S_abs += rows.abs() @ Wd[:, k].abs().t()
    yu = rd(y_exact) if y is None else y.to(dtype)
    mean = yu.mean(0)
    var = ((yu - mean) ** 2).mean(0)
    rstd = (var + eps) ** -0.5
    a = gamma * rstd
    b = beta - a * mean
    h = a * yu + b
    out_ref = torch.relu(h)
    if rounding and not out_f32:
        out_ref = bf16_round(out_ref)
    ou = out_ref if out is None else out.to(dtype)
    dh = g * (ou > 0)
    xhat = (yu - mean) * rstd
    dgamma = (dh * xhat).sum(0)
    dbeta = dh.sum(0)
    dy = rd(a * (dh - dbeta / n_out - xhat * dgamma / n_out))
    dW = torch.zeros(cout, 9, cin, dtype=dtype, device=dev)
    dx_exact = torch.zeros(n_in, cin, dtype=dtype, device=dev)
    for k in range(9):
        rows = xd[src[:, k]] * has[:, k, None]
        dW[:, k] = dy.t() @ rows
        dx_exact.index_add_(0, src[:, k], (dy @ Wd[:, k]) * has[:, k, None])
    return {"y_exact": y_exact, "y": yu, "S_abs": S_abs, "mean": mean, "var": var, "rstd": rstd, "a": a, "b": b, "h": h, "out": out_ref,
            "dh": dh, "dgamma": dgamma, "dbeta": dbeta, "dy": dy, "dW": dW.reshape(cout, 3, 3, cin), "dx_exact": dx_exact,
            "dx": rd(dx_exact), "x": xd, "W": Wd}


def drop_pair_effect(r, nbr, o, k):
    """What the judged quantities lose when the rulebook pair (o, k) is dropped, as the rank-one updates they are (dy held fixed):
    -> (|dy| of y row o per channel, Frobenius norm of the dW change, norm of the change of dx row i, i)."""
    i = int(nbr[o, k])
    assert i >= 0
    xi, Wk, dyo = r["x"][i], r["W"][:, k], r["dy"][o]
    return (Wk @ xi).abs(), float(dyo.norm() * xi.norm()), float((dyo @ Wk).norm()), i


def row_errors(dev_rows, ref_rows):
    """relative L2 and the worst row (row error / max(row norm, 5 % of the RMS row norm)), as tests/test_layer_fused_reference.py"""
    err = (dev_rows - ref_rows).norm(dim=1)
    nrm = ref_rows.norm(dim=1)
    rms = float((nrm ** 2).mean().sqrt())
    return float((dev_rows - ref_rows).norm() / ref_rows.norm()), float((err / nrm.clamp_min(0.05 * rms)).max())


# ------------------------------------------------------------------------------------------------------------------------------
# the block cases (section (b) of tests/test_conv_block_gpu.py); flags spread so that every value of every flag is seen twice
# ------------------------------------------------------------------------------------------------------------------------------
EPS, MOMENTUM = 1e-3, 0.01
CASES = {
    "1": dict(kind="subm", cin=128, cout=128, bf16=1, x_f32=0, n=129, out_f32=0, g_f32=0, running=1),
    "2": dict(kind="subm", cin=128, cout=128, bf16=1, x_f32=1, n=65, out_f32=1, g_f32=1, running=0),
    "3": dict(kind="down", cin=128, cout=256, bf16=1, x_f32=1, n=1400, out_f32=0, g_f32=1, running=1),
    "4": dict(kind="down", cin=256, cout=256, bf16=1, x_f32=0, n=1200, m=2, out_f32=1, g_f32=0, running=0),
    "5": dict(kind="subm", cin=256, cout=256, bf16=1, x_f32=1, n=33, out_f32=1, g_f32=1, running=1),
    "6": dict(kind="subm", cin=256, cout=256, bf16=1, x_f32=0, n=4200, out_f32=0, g_f32=0, running=0),
    "7": dict(kind="subm", cin=128, cout=128, bf16=1, x_f32=0, n=8200, out_f32=1, g_f32=0, running=1),
    "8": dict(kind="subm", cin=256, cout=256, bf16=1, x_f32=1, n=32769, out_f32=0, g_f32=1, running=0),
    "9s": dict(kind="subm", cin=128, cout=128, bf16=0, x_f32=0, n=129, out_f32=0, g_f32=0, running=1),
    "9d": dict(kind="down", cin=128, cout=128, bf16=0, x_f32=0, n=129, out_f32=0, g_f32=0, running=0),
}


def route(c):
    return "library" if not c["bf16"] else ("implicit_f32x" if c["x_f32"] else "implicit_bf16x")


def make_inputs(name):
    """CPU tensors of a block case (seeded by the case): the scene, x (bf16-representable values), W ~ 0.05 randn, gamma in [0.5, 1.5],
    beta ~ 0.3 randn, g ~ randn (bf16-representable where the block reads it as bf16), and the non-zero starting values of the accumulated
    gradients and the running statistics."""
    c = CASES[name]
    seed = 1000 + sorted(CASES).index(name)
    s = scene_full(c["kind"], c["n"], seed, c.get("m"))
    gen = torch.Generator().manual_seed(seed)
    cin, cout, n_in, n_out = c["cin"], c["cout"], s["n_in"], s["n_out"]
    x = torch.randn(n_in, cin, generator=gen).bfloat16().float()
    W = torch.randn(cout, 3, 3, cin, generator=gen) * 0.05
    gamma = 0.5 + torch.rand(cout, generator=gen)
    beta = 0.3 * torch.randn(cout, generator=gen)
    g = torch.randn(n_out, cout, generator=gen)
    if c["bf16"] and not c["g_f32"]:
        g = g.bfloat16().float()
    return {"case": c, "scene": s, "x": x, "W": W, "gamma": gamma, "beta": beta, "g": g,
            "dW0": 0.01 * torch.randn(cout, 3, 3, cin, generator=gen), "dgamma0": 0.1 * torch.randn(cout, generator=gen),
            "dbeta0": 0.1 * torch.randn(cout, generator=gen), "rm0": 0.5 + torch.rand(cout, generator=gen),
            "rv0": 0.5 + torch.rand(cout, generator=gen)}
