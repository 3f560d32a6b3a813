"""Plain CPU references of the loss tail of the pre-training step (NumPy float64 / float32; no project imports).

* ``random_mask``   the MAE token mask (csrc/mask.hip): per sample the ``int(L * keep_frac)`` smallest noises are visible,
                    ties by ascending index (stable argsort)
* ``group_gt``      the reconstruction targets (``k_group_gt``, csrc/chamfer.hip): slot k of a pillar takes point
                    ``csr[off + (k if k < cnt else k % cnt)]``, relative to the pillar centre, in float32 in the kernel's operation order
* ``chamfer``       the weighted Chamfer terms and their gradient (``k_chamfer`` / ``k_chamfer16``) in float64 with the arg-minima
                    written out (lowest j for a row, lowest i for a column), with an fp32 error bound per output that is derived from
                    the reference alone
* ``mean_finish``   the weighted-mean finish (``k_weighted_mean_finish``, csrc/attention.hip) with its summation bound

The second half holds the input generators that tests/test_loss_tail_reference_cpu.py (which pins all of this against ``oracle/``
and asserts the generators' stated properties) and tests/test_loss_tail_gpu.py share.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

U = 2.0 ** -24            # unit roundoff of fp32 (round to nearest)


# ==============================================================================================
# mask
# ==============================================================================================
def random_mask(noise, sample_off, keep_frac):
    """noise (M,) float32, sample_off (B + 1,) -> (mask (M,) float32, len_keep list of B ints)."""
    noise = np.asarray(noise, dtype=np.float32)
    mask = np.empty(noise.shape[0], dtype=np.float32)
    lens = []
    for b in range(len(sample_off) - 1):
        off, end = int(sample_off[b]), int(sample_off[b + 1])
        L = end - off
        len_keep = int(L * keep_frac)                         # Python doubles, truncation
        lens.append(len_keep)
        if len_keep <= 0:
            mask[off:end] = 1.0
        elif len_keep >= L:
            mask[off:end] = 0.0
        else:
            ids = np.argsort(noise[off:end], kind="stable")   # ties: ascending index
            m = np.ones(L, dtype=np.float32)
            m[ids[:len_keep]] = 0.0
            mask[off:end] = m
    return mask, lens


# ==============================================================================================
# reconstruction targets
# ==============================================================================================
def group_gt(points, n_cols, pt_off, csr, voxel_coords, K, lo, vs):
    """points (N, n_cols) float32 rows (b, x, y, z, ...), pt_off (M + 1,), csr (N,) point ids grouped by pillar,
    voxel_coords (M, 4) int64 (b, z, y, x) -> (gt (M, K, 3) float32, gidx (M, K) int32)."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, n_cols)
    pt_off = np.asarray(pt_off, dtype=np.int64)
    csr = np.asarray(csr, dtype=np.int64)
    vc = np.asarray(voxel_coords, dtype=np.int64)
    off, cnt = pt_off[:-1, None], (pt_off[1:] - pt_off[:-1])[:, None]
    assert (cnt >= 1).all(), "a pillar without points is outside the kernel's contract"
    k = np.arange(K, dtype=np.int64)[None, :]
    src = np.where(k < cnt, k, k % cnt)
    gidx = csr[off + src]                                     # (M, K)
    lo32, vs32 = np.asarray(lo, dtype=np.float32), np.asarray(vs, dtype=np.float32)
    idx = vc[:, [3, 2, 1]].astype(np.float32)                 # x, y, z cell index
    centre = (idx + np.float32(0.5)) * vs32 + lo32            # float32 array operations: one rounding each, in this order
    assert centre.dtype == np.float32
    gt = points[gidx][:, :, 1:4] - centre[:, None, :]
    assert gt.dtype == np.float32
    return gt, gidx.astype(np.int32)


# ==============================================================================================
# Chamfer terms and gradient
# ==============================================================================================
# fp32 operations on the longest path to an output, read off csrc/chamfer.hip (squared distances are exact on the dyadic input sets):
#   term   sum of the P1 row minima (k_chamfer: `sumx += dmin`, P1 additions; k_chamfer16: gd_wave_sum, 6) and of the P2 column
#          minima (gd_wave_sum: 6 <= P2 for the bound's purpose, counted as P2), then `cx = wm / P1` (1), `cx * sumx` (1) and the
#          final addition (1): every summand passes through at most P1 + P2 + 3 roundings, all summands are >= 0
#   dpred  row part `2 * cx * d` (2 * cx is exact, cx carries 1, the product 1), each column part `2 * cy * (x - y)` the same 2, their
#          sum over at most P2 ground-truth points (k_chamfer16: `acc +=` P2 times; k_chamfer: gd_wave_sum) and the addition of the
#          two parts (1).  Counted as the P2 additions + division + product + final addition = P2 + 3.
TERM_STEPS = 3
DPRED_STEPS = 3


@dataclass
class ChamferRef:
    term: np.ndarray          # (M,) float64
    dpred: np.ndarray         # (M, P1, 3) float64, gradient of term (unscaled, as the kernel writes it)
    loss: float
    inv: float
    term_bound: np.ndarray    # (M,)
    dpred_bound: np.ndarray   # (M, P1, 3)
    row_arg: np.ndarray       # (M, P1) nearest ground-truth point of every prediction
    col_arg: np.ndarray       # (M, P2) nearest prediction of every ground-truth point
    col_arg2: np.ndarray      # (M, P2) runner-up prediction (col_arg where P1 == 1)
    row_gap: np.ndarray       # (M, P1) (second best - best) / second best, inf where P2 == 1
    col_gap: np.ndarray       # (M, P2)


def _best_two(d, axis, tie):
    """arg-min along `axis` with the tie rule written out, the runner-up and the relative gap between their distances."""
    n = d.shape[axis]
    dmin = d.min(axis=axis, keepdims=True)
    eq = d == dmin
    if tie == "lowest":
        arg = eq.argmax(axis=axis)                                            # first index that attains the minimum
    else:                                                                     # deliberately wrong rule for the tests' self-check
        arg = n - 1 - np.flip(eq, axis=axis).argmax(axis=axis)
    if n == 1:
        return arg, arg.copy(), np.full(arg.shape, np.inf)
    d2 = d.copy()
    np.put_along_axis(d2, np.expand_dims(arg, axis), np.inf, axis=axis)
    arg2 = d2.argmin(axis=axis)
    second = d2.min(axis=axis)
    best = dmin.squeeze(axis)
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(second > 0, (second - best) / second, 0.0)
    return arg, arg2, gap


def chamfer(pred, gt, w, tie="lowest", chunk=512) -> ChamferRef:
    """term_m = w_m * (mean_i min_j d + mean_j min_i d), d = |x_i - y_j|^2; dpred = d term / d pred; loss = sum(term) / sum(w)."""
    x_all, y_all, w_all = (np.asarray(a, dtype=np.float64) for a in (pred, gt, w))
    M, P1, _ = x_all.shape
    P2 = y_all.shape[1]
    term, dpred = np.zeros(M), np.zeros((M, P1, 3))
    tb, db = np.zeros(M), np.zeros((M, P1, 3))
    row_arg, col_arg, col_arg2 = np.zeros((M, P1), np.int64), np.zeros((M, P2), np.int64), np.zeros((M, P2), np.int64)
    row_gap, col_gap = np.zeros((M, P1)), np.zeros((M, P2))
    ar1 = np.arange(P1)[None, :, None]
    for a in range(0, M, chunk):                          # pillars in chunks: P1 = P2 = 64 at large M stays a few megabytes
        s = slice(a, min(a + chunk, M))
        x, y, wm = x_all[s], y_all[s], w_all[s]
        diff = [x[:, :, None, c] - y[:, None, :, c] for c in range(3)]          # (m, P1, P2) per coordinate
        d = diff[0] * diff[0] + diff[1] * diff[1] + diff[2] * diff[2]
        ja, _, rg = _best_two(d, 2, tie)                  # row i: nearest ground-truth point
        ia, ia2, cg = _best_two(d, 1, tie)                # column j: nearest prediction
        row_min = np.take_along_axis(d, ja[:, :, None], 2)[:, :, 0]
        col_min = np.take_along_axis(d, ia[:, None, :], 1)[:, 0, :]
        term[s] = wm * (row_min.sum(1) / P1 + col_min.sum(1) / P2)
        tb[s] = (P1 + P2 + TERM_STEPS) * U * term[s]
        onehot = ia[:, None, :] == ar1                    # (m, P1, P2): column j counts for prediction i
        for c in range(3):
            row = 2.0 * (wm / P1)[:, None] * np.take_along_axis(diff[c], ja[:, :, None], 2)[:, :, 0]
            col = 2.0 * (wm / P2)[:, None] * np.where(onehot, diff[c], 0.0).sum(2)
            col_abs = 2.0 * (wm / P2)[:, None] * np.where(onehot, np.abs(diff[c]), 0.0).sum(2)
            dpred[s, :, c] = row + col
            db[s, :, c] = (P2 + DPRED_STEPS) * U * (np.abs(row) + col_abs)
        row_arg[s], col_arg[s], col_arg2[s], row_gap[s], col_gap[s] = ja, ia, ia2, rg, cg
    sw = float(w_all.sum())
    inv = 1.0 / sw if sw > 0 else 0.0
    return ChamferRef(term, dpred, float(term.sum()) * inv, inv, tb, db, row_arg, col_arg, col_arg2, row_gap, col_gap)


def near_tie_points(ref: ChamferRef, tol):
    """(rows (M, P1), cols (M, P2), points (M, P1)): rows / columns whose best and second-best distance differ by a relative gap in
    (0, tol) - an fp32 kernel may legitimately pick the other minimiser - and the predictions whose gradient such a choice changes (the
    row's own prediction; both candidate predictions of a column).  A gap of exactly 0 is not a near tie: in float64 it only arises
    from duplicated points, whose fp32 distances are computed by the same operations on the same operands and are therefore bit-equal
    in the kernel too, so the tie rule decides."""
    rows = (ref.row_gap > 0) & (ref.row_gap < tol)
    cols = (ref.col_gap > 0) & (ref.col_gap < tol)
    pts = rows.copy()
    m, j = np.nonzero(cols)
    pts[m, ref.col_arg[m, j]] = True
    pts[m, ref.col_arg2[m, j]] = True
    return rows, cols, pts


def mean_finish(term32, w32):
    """(loss, inv, loss_bound, inv_rel_bound) of k_weighted_mean_finish on fp32 inputs, evaluated in float64.
    The kernel adds n values in fp32 in a fixed tree (any association errs by at most n * u * sum|term|), forms inv = 1 / sum(w)
    (one rounding; the generators keep sum(w) exact in fp32 in any order, asserted by weights_sum_exact) and multiplies (one rounding):
    |loss error| <= inv * n * u * sum|term| + 3 u |loss|."""
    t, w = np.asarray(term32, dtype=np.float32).astype(np.float64), np.asarray(w32, dtype=np.float32).astype(np.float64)
    n = t.shape[0]
    sw = float(w.sum())
    inv = 1.0 / sw if sw > 0 else 0.0
    loss = float(t.sum()) * inv
    return loss, inv, inv * n * U * float(np.abs(t).sum()) + 3 * U * abs(loss), 2 * U


def weights_sum_exact(w):
    """True when every partial sum of w, in any order, is representable in fp32: all weights are multiples of one power of two q and
    sum(w) / q < 2^24."""
    w = np.asarray(w, dtype=np.float64)
    nz = w[w != 0]
    if nz.size == 0:
        return True
    q = 2.0 ** np.floor(np.log2(np.abs(nz).min()))
    while not np.all(np.round(nz / q) == nz / q):
        q /= 2
        if q < 2.0 ** -60:
            return False
    return float(np.abs(nz).sum() / q) < 2 ** 24


# ==============================================================================================
# input generators (shared by the CPU pins and the GPU tests)
# ==============================================================================================
# ---- mask
MASK_LAUNCHES = {
    "seven": [1, 0, 1023, 1024, 1025, 16384, 16385],      # both sides of the 1024-element round and of the 16 * 1024 register cache
    "three": [40000, 3, 16385],                           # uncached body first, then a tiny sample behind it
    "hundred": [100, 7, 2049],                            # 100 * 0.71 is exactly 71.0 in doubles, 100 * 0.57 is 56.99999999999999
}
MASK_KINDS = ["distinct", "coarse", "equal", "signed"]
# 0.57 is the truncation case: L * 0.57 falls just below an integer in doubles for L = 100 (-> 56) and L = 40000 (-> 22799)
MASK_KEEP_FRACS = [0.0, 1.0, 0.25, 0.71, 1 - 0.85, 0.57, 1.0 / 2048]      # 1 / 2048 < 1 / L for every L <= 2047: len_keep truncates to 0


def mask_noise(kind, lengths, seed=0):
    """-> (noise (sum L,) float32, sample_off (B + 1,) int32).  No input holds -0.0: the kernel's key orders it before +0.0 and a
    stable argsort treats the two as equal; torch.rand, the product's noise source, never produces it."""
    rng = np.random.default_rng(seed)
    parts = []
    for L in lengths:
        if kind == "distinct":
            v = rng.permutation(L).astype(np.float64) / max(L, 1)
        elif kind == "coarse":                            # ~L / 50 copies of every value: ties straddle the boundary and the rounds
            v = rng.integers(0, 50, L) / 50
        elif kind == "equal":                             # every pillar ties: ties_to_keep = len_keep
            v = np.full(L, 0.375)
        else:                                             # negative and mixed-sign finite values over many binades, with ties
            v = rng.standard_normal(L) * 10.0 ** rng.integers(-20, 20, L)
            t = rng.random(L) < 0.5
            v[t] = rng.integers(-25, 25, int(t.sum())) / 25
        v = v.astype(np.float32)
        v[v == 0] = 0.0                                   # +0.0 only
        parts.append(v)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return (np.concatenate(parts) if parts else np.zeros(0, np.float32)), off


# ---- reconstruction targets
GT_LO, GT_VS, GT_GRID = (-75.2, -75.2, -2.0), (0.32, 0.32, 6.0), 470


def gt_scene(K, n_cols, sizes=None, reps=30, seed=0, lo=GT_LO, vs=GT_VS, grid=GT_GRID, dyadic=False):
    """Pillars of the crafted sizes in distinct cells of a grid x grid map (cell (0, 0) and the last cell included, batch 0..2).
    The point rows are shuffled, and csr lists every pillar's points as a random permutation of its ascending list, so a kernel
    that sorted them or took them in row order would show.  ``dyadic``: offsets from the centre are multiples of 1 / 64."""
    rng = np.random.default_rng(seed)
    if sizes is None:
        sizes = np.array([1, 2, K - 1, K, K + 1, 5 * K, 63, 64, 65] * reps)
    sizes = np.asarray(sizes, dtype=np.int64)
    M, N = len(sizes), int(sizes.sum())
    cells = rng.choice(3 * grid * grid - 2, M - 2, replace=False) + 1 if M > 2 else np.zeros(0, np.int64)
    cells = np.concatenate([[0], np.sort(cells), [3 * grid * grid - 1]])[:M]
    vc = np.stack([cells // (grid * grid), np.zeros(M, np.int64), (cells // grid) % grid, cells % grid], 1).astype(np.int64)
    owner = np.repeat(np.arange(M), sizes)
    owner = owner[rng.permutation(N)]                     # pillar of every point row
    pts = np.zeros((N, n_cols), dtype=np.float32)
    pts[:, 0] = vc[owner, 0]
    lo32, vs32 = np.asarray(lo, np.float32), np.asarray(vs, np.float32)
    centre = (vc[owner][:, [3, 2, 1]].astype(np.float32) + np.float32(0.5)) * vs32 + lo32
    if dyadic:
        frac = rng.integers(-16, 17, (N, 3)) / 64.0
        frac[:, 2] = rng.integers(-128, 129, N) / 64.0
        pts[:, 1:4] = centre + frac.astype(np.float32)
    else:
        pts[:, 1:4] = centre + (rng.uniform(-0.5, 0.5, (N, 3)) * vs32).astype(np.float32)
    if n_cols > 4:
        pts[:, 4:] = rng.random((N, n_cols - 4), dtype=np.float32)
    order = np.argsort(owner, kind="stable")              # ascending point ids inside every pillar
    pt_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    csr = order.copy()
    for p in range(M):
        a, b = pt_off[p], pt_off[p + 1]
        if b - a > 1:
            csr[a:b] = rng.permutation(order[a:b])
    return {"points": pts, "pt_off": pt_off, "csr": csr.astype(np.int32), "voxel_coords": vc, "M": M,
            "lo": tuple(float(v) for v in lo), "vs": tuple(float(v) for v in vs)}


def gt_scene_many(seed=1):
    """M = 4 * 8192 + 5 pillars of 1 to 3 points: past the grid cap, every wave walks a second pillar."""
    rng = np.random.default_rng(seed)
    return gt_scene(64, 4, sizes=rng.integers(1, 4, 4 * 8192 + 5), seed=seed)


# ---- Chamfer
CHAMFER_FAST = [(16, 1), (16, 2), (16, 3), (16, 5), (16, 63), (16, 64)]
CHAMFER_GENERIC = [(1, 1), (1, 64), (15, 64), (17, 64), (64, 64), (64, 1), (3, 5)]
CHAMFER_M = 203
CHAMFER_MANY = [(16, 64), (16, 3), (3, 5)]
CHAMFER_M_MANY = 4 * 8192 + 5
CHAMFER_RANDOM = [(16, 64), (24, 33)]
WEIGHTS = np.array([0.0, 1.0, 0.5, 2.0 ** -10, 3.0], dtype=np.float32)
N_PLANTED = 4


def chamfer_weights(M, seed, runs=False):
    """Weights from {0, 1, 0.5, 2^-10, 3}.  ``runs``: constant over runs of 1 to 9 pillars, so that at M past the grid cap a wave meets
    zero-weight pillars between live ones inside its loop; zero is drawn half of the time, which also keeps sum(w) exact in fp32."""
    rng = np.random.default_rng(seed)
    if not runs:
        w = WEIGHTS[rng.integers(0, 5, M)]
        w[:N_PLANTED] = WEIGHTS[1 + np.arange(N_PLANTED) % 4]         # the planted pillars stay live
        return w
    out = []
    while sum(len(o) for o in out) < M:
        out.append(np.full(int(rng.integers(1, 10)), WEIGHTS[rng.choice(5, p=[0.5, 0.2, 0.15, 0.1, 0.05])]))
    w = np.concatenate(out)[:M].astype(np.float32)
    w[:N_PLANTED] = WEIGHTS[1 + np.arange(N_PLANTED) % 4]
    # the launch has 4 * 8192 waves: pillar m and pillar m + 4 * 8192 share a wave and its LDS rows.  Waves 0 - 2 take two live
    # pillars, wave 3 a live one and then a zero-weight one, wave 4 a zero-weight one (the early `continue`) and then a live one
    s = 4 * 8192
    if M > s + 4:
        w[4] = 0.0
        w[s:s + 5] = [1.0, 0.5, 2.0 ** -10, 0.0, 3.0]
    return w


def chamfer_dyadic(kind, M, P1, P2, seed=0):
    """-> (pred (M, P1, 3), gt (M, P2, 3)) float32.
    "fine":   multiples of 1 / 64 in [-4, 4]: every squared distance is exact in fp32 (|difference| <= 512 / 64, three squares of at
              most 2^18 / 2^12 add up below 2^24 / 2^12)
    "coarse": multiples of 1 / 2 in [-2, 2]: many exact ties between distinct points, plus four planted pillars:
              0 duplicated predicted points, 1 duplicated ground-truth points, 2 all ground-truth points equal (a one-point pillar after
              the cyclic padding), 3 pred == gt over the first min(P1, P2) points (d = +0)."""
    rng = np.random.default_rng(seed)
    if kind == "fine":
        pred = rng.integers(-256, 257, (M, P1, 3)) / 64.0
        gt = rng.integers(-256, 257, (M, P2, 3)) / 64.0
    else:
        pred = rng.integers(-4, 5, (M, P1, 3)) / 2.0
        gt = rng.integers(-4, 5, (M, P2, 3)) / 2.0
        h1, h2 = P1 // 2, P2 // 2
        pred[0, h1:2 * h1] = pred[0, :h1]
        gt[1, h2:2 * h2] = gt[1, :h2]
        gt[2, :] = gt[2, 0]
        n = min(P1, P2)
        pred[3, :n] = gt[3, :n]
    return pred.astype(np.float32), gt.astype(np.float32)


def chamfer_random(M, P1, P2, seed=2):
    """The inputs of tests/test_hip_parity.py::test_chamfer_matches_oracle (same seed, same draw order)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(M, P1, 3, generator=g)
    gt = torch.randn(M, P2, 3, generator=g)
    gt[5, 1] = gt[5, 0]
    w = (torch.rand(M, generator=g) < 0.8).float()
    return pred.numpy(), gt.numpy(), w.numpy()


# ---- weighted-mean finish
FINISH_N = [1, 3, 4, 5, 4095, 4096, 4097, 16384 + 5]      # around the 16-byte vector width and the 4 x 1024-vector sweep of the kernel


def finish_inputs(seed=5):
    """The reference's own terms of a coarse (3, 5) case of max(FINISH_N) pillars, rounded to fp32, and their weights."""
    n = max(FINISH_N)
    pred, gt = chamfer_dyadic("coarse", n, 3, 5, seed=seed)
    w = chamfer_weights(n, seed)
    return chamfer(pred, gt, w).term.astype(np.float32), w


# ---- the chained case: crafted points -> targets -> Chamfer
CHAIN_LO, CHAIN_VS = (-64.0, -64.0, -2.0), (0.5, 0.5, 4.0)     # centres are multiples of 1 / 4: offsets stay multiples of 1 / 64


def chain_scene(seed=3):
    sc = gt_scene(64, 4, reps=12, seed=seed, lo=CHAIN_LO, vs=CHAIN_VS, grid=256, dyadic=True)
    rng = np.random.default_rng(seed + 100)
    sc["perturb"] = (rng.integers(-64, 65, (sc["M"], 16, 3)) / 64.0).astype(np.float32)
    sc["w"] = chamfer_weights(sc["M"], seed)
    return sc
