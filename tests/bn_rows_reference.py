"""Plain float64 reference of the BatchNorm(train)+ReLU row kernels (csrc/segment.hip, csrc/decoder.hip): the statistics fold, the
elementwise forward / backward over rows, the segmented maximum with its tie rule, the row movers, and the rounding-model bounds the
GPU tests hold the kernels to.  NumPy / torch on the CPU, no project imports.  tests/test_bn_rows_reference_cpu.py pins every
function to torch.nn.functional.batch_norm under autograd and shows that an fp32 emulation of the kernels' summation shape sits
inside the bounds with a factor 4 to spare; tests/test_bn_rows_gpu.py runs the kernels against it.

Rounding model (the only source of the bounds; nothing is fitted to a kernel's output)
  * a column sum is formed in three levels: every thread adds the terms of its strided rows in fp32, one after the other
    (m = ceil(chunk / rows_per_iter) additions, chunk = ceil(n / nblk) rows per workgroup), the per-thread sums of a column meet in
    LDS in fp32 (min(rows_per_iter, chunk) of them hold anything), the nblk partial rows are combined in fp64 (no error at this
    scale).  Worst case for depth = m + min(rows_per_iter, chunk) additions plus the product's rounding:
    |err| <= (depth + 2) u sum|t|, u = 2^-24.
  * the max layer's backward may take x at an arg-max as (out - b) / a instead of reading it, where that quotient is within a few
    roundings of x; RECON more roundings per term are allowed for it, for every channel alike (no allowance grows with 1 / a).
  * an elementwise result a*P + b is one fused multiply-add: |err| <= 2^-23 (|a P| + |b|) is a loose cover of u |result|; a bf16
    result adds 2^-8 |ref| (bf16's unit roundoff: 8 significant bits), and a rounded intermediate (relu before `sub` / `add`)
    adds 2^-8 of that intermediate.
"""

import numpy as np
import torch

U = 2.0 ** -24           # fp32 unit roundoff
UB = 2.0 ** -8           # bf16 unit roundoff: 8 significant bits, half an ulp just above a power of two is 2^-8 of the value
RECON = 8                # roundings allowed per term where the max-layer backward takes x as (out - b) / a instead of reading it


# ------------------------------------------------------------------------------------------------ number formats
def bf16_round(x):
    """float64/float32 array -> the nearest bf16 value (ties to even), as float64; via fp32 like the device (dec_f2bf)."""
    f = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    t = torch.from_numpy(f.reshape(-1).copy()).to(torch.bfloat16).to(torch.float32).numpy().reshape(f.shape)
    return t.astype(np.float64)


def round_to(x, bf16):
    return bf16_round(x) if bf16 else np.asarray(x, np.float64)


# ------------------------------------------------------------------------------------------------ statistics
def fold(s1, s2, count, gamma, beta, eps, momentum=0.1, running_mean=None, running_var=None, num_batches_tracked=None):
    """Column sums s1 / sums of squares s2 of an (R, C) matrix over ``count`` >= R samples (the missing ones are zeros) ->
    dict(mean, var (biased), rstd, a = gamma rstd, b = beta - a mean) and, when running statistics are given, their update as
    nn.BatchNorm does it (unbiased variance count / (count - 1), momentum, counter + 1)."""
    s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    mean = s1 / count
    var = np.maximum(s2 / count - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + eps)
    a = gamma * rstd
    out = dict(mean=mean, var=var, rstd=rstd, a=a, b=beta - a * mean)
    if running_mean is not None:
        unb = var * (count / (count - 1.0)) if count > 1 else var
        out["running_mean"] = (1.0 - momentum) * np.asarray(running_mean, np.float64) + momentum * mean
        out["running_var"] = (1.0 - momentum) * np.asarray(running_var, np.float64) + momentum * unb
        out["num_batches_tracked"] = int(num_batches_tracked) + 1
    return out


def colsums(X):
    X = np.asarray(X, np.float64)
    return X.sum(0), (X * X).sum(0)


# ------------------------------------------------------------------------------------------------ elementwise rows
def rows_forward(P, a, b, site=None, Z0=None, zrow=None, col0=0, sub=None, add=None, z_bf16=False):
    """Z[site[r] or r, col0:col0+C] = relu(a P[r] + b)  [- sub[c] | + add[r], each after rounding the ReLU to Z's dtype].
    Z0 (rows, zrow) is the map before the call (default: n rows of NaN); every other element keeps its value.  float64 out,
    NOT rounded to Z's dtype at the end (the caller's bound carries that rounding)."""
    P = np.asarray(P, np.float64)
    n, C = P.shape
    zrow = C if zrow is None else zrow
    Z = np.full((n, zrow), np.nan) if Z0 is None else np.array(Z0, np.float64, copy=True)
    y = np.maximum(np.asarray(a, np.float64) * P + np.asarray(b, np.float64), 0.0)
    if sub is not None:
        y = round_to(y, z_bf16) - np.asarray(sub, np.float64)[None, :]
    if add is not None:
        y = round_to(y, z_bf16) + np.asarray(add, np.float64)
    rows = np.arange(n) if site is None else np.asarray(site, np.int64)
    Z[rows, col0:col0 + C] = y
    return Z


def rows_backward_sums(P, a, b, G):
    """G (n, C) = the rows of dZ the kernel reads.  -> (3, C): column sums of dh = G [a P + b > 0], dh P, G; and dh."""
    P, G = np.asarray(P, np.float64), np.asarray(G, np.float64)
    dh = np.where(np.asarray(a, np.float64) * P + np.asarray(b, np.float64) > 0.0, G, 0.0)
    return np.stack([dh.sum(0), (dh * P).sum(0), G.sum(0)]), dh


def bn_coeffs(sums, mean, rstd, a, b, count, tot=None):
    """BatchNorm chain rule from the column sums, written from y = gamma (x - mean) rstd + beta:
      dbeta = sum dh (+ the background's share (tot - sum g) where its constant relu(b) is positive),
      dgamma = sum dh (x - mean) rstd,  dx = a dh + c0 + c1 x  with  c1 = -a rstd dgamma / count,  c0 = -a dbeta / count - c1 mean."""
    sums = np.asarray(sums, np.float64)
    dbeta = sums[0].copy()
    if tot is not None:
        dbeta = dbeta + np.where(np.asarray(b, np.float64) > 0.0, np.asarray(tot, np.float64) - sums[2], 0.0)
    dgamma = (sums[1] - mean * dbeta) * rstd
    c1 = -a * rstd * dgamma / count
    c0 = -a * dbeta / count - c1 * mean
    return dict(dgamma=dgamma, dbeta=dbeta, c0=c0, c1=c1)


def rows_backward(P, a, b, G, mean, rstd, count, tot=None):
    sums, dh = rows_backward_sums(P, a, b, G)
    k = bn_coeffs(sums, mean, rstd, np.asarray(a, np.float64), b, count, tot)
    k["sums"] = sums
    k["dP"] = np.asarray(a, np.float64) * dh + k["c0"] + k["c1"] * np.asarray(P, np.float64)
    return k


# ------------------------------------------------------------------------------------------------ segmented maximum
def _segmax_values(H, pt_off, csr):
    """H (N, C) values to maximise.  Per segment the points are visited in ascending point id; the first point is always taken and a
    later one only when strictly larger (so ties and a leading NaN / -inf resolve to the lowest id).  -> out (M, C), arg (M, C)."""
    H = np.asarray(H, np.float64)
    pt_off, csr = np.asarray(pt_off, np.int64), np.asarray(csr, np.int64)
    M, C = len(pt_off) - 1, H.shape[1]
    out, arg = np.empty((M, C)), np.empty((M, C), np.int64)
    for p in range(M):
        ids = np.sort(csr[pt_off[p]:pt_off[p + 1]])
        best, bi = H[ids[0]].copy(), np.full(C, ids[0], np.int64)
        if len(ids) > 1:
            X = H[ids[1:]]
            if np.isnan(best).any() or np.isnan(X).any():
                for j, i in enumerate(ids[1:]):
                    m = X[j] > best
                    best[m], bi[m] = X[j][m], i
            else:
                k = np.argmax(H[ids], axis=0)               # first occurrence = lowest id
                best, bi = H[ids][k, np.arange(C)], ids[k]
        out[p], arg[p] = best, bi
    return out, arg


def segment_max(x, pt_off, csr):
    return _segmax_values(x, pt_off, csr)


def segment_max_affine(x, a, b, pt_off, csr):
    h = np.maximum(np.asarray(a, np.float64) * np.asarray(x, np.float64) + np.asarray(b, np.float64), 0.0)
    return _segmax_values(h, pt_off, csr)


def segment_max_bwd(dout, arg, inv, N):
    """dx[i, c] = dout[inv[i], c] where arg[inv[i], c] == i, else 0."""
    dout, arg, inv = np.asarray(dout, np.float64), np.asarray(arg, np.int64), np.asarray(inv, np.int64)
    return np.where(arg[inv] == np.arange(N)[:, None], dout[inv], 0.0)


def segmax_affine_dh(out, arg, dout, inv, N):
    """dh[i, c] = dout[p, c] where arg[p, c] == i and out[p, c] > 0 (p = inv[i])."""
    return segment_max_bwd(np.where(np.asarray(out) > 0, np.asarray(dout, np.float64), 0.0), arg, inv, N)


def segmax_affine_sums(x, out, arg, dout):
    """(2, C): column sums of dh and dh x over the arg-max points (walks the (M, C) outputs like the kernel)."""
    x, dout = np.asarray(x, np.float64), np.asarray(dout, np.float64)
    g = np.where(np.asarray(out) > 0, dout, 0.0)
    xa = x[np.asarray(arg, np.int64), np.arange(x.shape[1])[None, :]]
    return np.stack([g.sum(0), (g * xa).sum(0)]), np.stack([np.abs(g).sum(0), np.abs(g * xa).sum(0)])


# ------------------------------------------------------------------------------------------------ row movers (any dtype)
def gather_rows(table, idx, col0=0, width=None):
    table, idx = np.asarray(table), np.asarray(idx, np.int64)
    width = table.shape[1] - col0 if width is None else width
    out = np.zeros((len(idx), width), table.dtype)
    ok = idx >= 0
    out[ok] = table[idx[ok], col0:col0 + width]
    return out


def scatter_rows(src, idx, table, col0=0):
    src, idx = np.asarray(src), np.asarray(idx, np.int64)
    out = np.array(table, copy=True)
    ok = idx >= 0
    out[idx[ok], col0:col0 + src.shape[1]] = src[ok]
    return out


def fill_rows(v, R):
    return np.tile(np.asarray(v)[None, :], (R, 1))


# ------------------------------------------------------------------------------------------------ summation geometry and bounds
def colstats_rows(R):
    """partial rows of gdmae_colstats / gdmae_bn_fold: clamp(R / 64, 1, 512), 1024 from 2^20 rows."""
    return 1024 if R >= (1 << 20) else max(1, min(512, R // 64))


def bwd_stats_rows(n):
    """partial rows of gdmae_rows_bwd_stats / gdmae_segmax_bwd_stats: clamp(n / 32, 1, 512)."""
    return max(1, min(512, n // 32))


def colstats_rpi(C, bf16):
    return 256 // (C // (8 if bf16 else 4))


def bwd_stats_rpi(C, v8):
    return 256 // (C // 8) if v8 else max(1, 256 // C)


def sum_depth(n, nblk, rpi):
    """additions behind one partial-row entry: m per thread, then the per-thread sums that hold anything (a thread whose first row
    lies beyond the chunk contributes an exact zero)."""
    chunk = -(-n // nblk)
    return -(-chunk // rpi) + min(rpi, chunk)


def sum_bound(abs_sum, n, nblk, rpi, extra=0):
    """worst-case error of the three-level column sum of terms whose absolute values add up to abs_sum."""
    return (sum_depth(n, nblk, rpi) + 2 + extra) * U * np.asarray(abs_sum, np.float64)


def emulate_sum(T, nblk, rpi):
    """fp32 emulation of the kernels' summation: T (n, C) fp32 terms -> (column sums float64, the nblk fp32 partial rows).
    Per workgroup: rpi per-thread sequential fp32 sums over rows r0 + tr, r0 + tr + rpi, ...; fp32 combine in tr order; fp64 over blocks."""
    T = np.asarray(T, np.float32)
    n, C = T.shape
    chunk = -(-n // nblk)
    part = np.zeros((nblk, C), np.float32)
    for blk in range(nblk):
        r0, r1 = blk * chunk, min(blk * chunk + chunk, n)
        acc = np.zeros(C, np.float32)
        for tr in range(rpi):
            s = np.zeros(C, np.float32)
            for r in range(r0 + tr, r1, rpi):
                s = s + T[r]
            acc = acc + s
        part[blk] = acc
    return part.astype(np.float64).sum(0), part


def fold_bounds(abs1, abs2, e1, e2, s1, s2, count, gamma, beta, eps):
    """Bounds on mean, var, rstd, a, b of ``fold`` when the sums carry errors <= e1, e2 (propagated through s2 / count - mean^2, so the
    variance bound widens with mean^2 / var by construction), plus one fp32 rounding where the kernel stores fp32 (a, b, mean, var)."""
    f = fold(s1, s2, count, gamma, beta, eps)
    mean, var, r = f["mean"], f["var"], f["rstd"]
    d_mean = e1 / count
    d_var = e2 / count + 2.0 * np.abs(mean) * d_mean + d_mean * d_mean
    r_lo = 1.0 / np.sqrt(var + d_var + eps)
    r_hi = 1.0 / np.sqrt(np.maximum(var - d_var, 0.0) + eps)
    d_r = np.maximum(r - r_lo, r_hi - r) + 4 * 2.0 ** -53 * r
    g = np.abs(np.asarray(gamma, np.float64))
    d_a = g * d_r + U * np.abs(f["a"])
    d_b = d_a * np.abs(mean) + np.abs(f["a"]) * d_mean + U * (np.abs(f["b"]) + np.abs(f["a"] * mean) + np.abs(beta))
    return dict(mean=d_mean, var=d_var, rstd=d_r, a=d_a, b=d_b, mean32=d_mean + U * np.abs(mean), var32=d_var + U * var)


def elementwise_bound(a, P, b, ref, bf16, mid=None):
    """|Z - ref| allowed for Z = relu(fma(a, P, b)) [-/+ v]: 2^-23 (|a P| + |b|), for bf16 Z additionally 2^-8 |ref| and - where the
    ReLU was rounded before a second operand was applied - 2^-8 of that intermediate (``mid``)."""
    t = 2.0 ** -23 * (np.abs(np.asarray(a, np.float64) * np.asarray(P, np.float64)) + np.abs(np.asarray(b, np.float64)))
    if bf16:
        t = t + UB * np.abs(ref) + (UB * np.abs(mid) if mid is not None else 0.0)
    elif mid is not None:
        t = t + 2.0 ** -23 * np.abs(ref)
    return t


# ------------------------------------------------------------------------------------------------ input generators (seeded, CPU)
FAMILIES = (0.0, 1.0, 30.0, 300.0)        # mean / std of the column families


def stats_matrix(R, C, seed, bf16):
    """(R, C) fp32 matrix (bf16-representable when bf16) whose columns cycle through: mean/std in FAMILIES (std = 0.5), then one
    constant column (2.5), then one column of zeros.  -> (X fp32, family id per column: 0..3 = FAMILIES, 4 = constant, 5 = zeros)."""
    rng = np.random.default_rng(seed)
    fam = np.arange(C) % 6
    X = np.empty((R, C), np.float32)
    for c in range(C):
        k = fam[c]
        if k < 4:
            X[:, c] = (0.5 * rng.standard_normal(R) + 0.5 * FAMILIES[k]).astype(np.float32)
        elif k == 4:
            X[:, c] = 2.5
        else:
            X[:, c] = 0.0
    if bf16:
        X = bf16_round(X).astype(np.float32)
    return X, fam


def make_pillars(sizes, seed):
    """Segments of the given sizes over N = sum(sizes) points whose ids are interleaved across segments (not segment-major) and
    ascending inside each segment, as the plan's CSR is.  -> pt_off (M + 1), csr (N), inv (N)."""
    rng = np.random.default_rng(seed)
    M, N = len(sizes), int(np.sum(sizes))
    inv = np.repeat(np.arange(M), sizes)
    inv = inv[rng.permutation(N)]
    csr = np.argsort(inv, kind="stable")
    pt_off = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=M))])
    return pt_off.astype(np.int32), csr.astype(np.int32), inv.astype(np.int32)


def pillar_sizes(C):
    G = 64 // (C // 4)
    return sorted({1, max(G - 1, 1), G, G + 1, 2 * G + 1, 1000})
