"""Float64 reference of the optimizer step of csrc/optim.hip (global-norm clip, decoupled decay, Adam, bf16 shadow), its rounding
bound, wrong variants of it and the crafted inputs of tests/test_optimizer_reference_cpu.py and tests/test_optimizer_step_gpu.py.
Plain numpy: no GPU code, nothing here imports the package.

Semantics (oracle/optim_oracle.py documents where the reference optimizer defines them):
    total = sqrt(sq_norm) * grad_scale                           norm of the AVERAGED gradient
    coef  = grad_scale * min(max_norm / (total + 1e-6), 1)       when max_norm > 0, else grad_scale (sq_norm is not read)
    inside the segments:   p *= 1 - wd * lr;  g' = g * coef;  m' = beta1 m + (1 - beta1) g';  v' = beta2 v + (1 - beta2) g'^2
                           p' = p - lr / (1 - beta1^t) * m' / (sqrt(v') / sqrt(1 - beta2^t) + eps)
    outside the segments:  nothing changes
``sq_norm`` is an INPUT, as in the C entry, so the rounding of the norm kernels does not enter the check of the Adam kernel.
The scalar arguments are rounded to float32 first: that is what crosses the C ABI (``float lr, float beta1, ...``), and the
reference describes the step the kernel was asked for.

Rounding bound (``bounds``): first-order count over the kernel's operation sequence (k_adam; the library is compiled without
floating-point contraction and with correctly rounded division and square root, so every operation contributes one unit
u = 2^-24 relative to ITS OWN result).  The units multiply the magnitudes of the TERMS, not of the result - m' can cancel.
    coef   c = 6 when max_norm > 0: the constant 1e-6f (1), sqrtf (1), * grad_scale (1), + 1e-6f (1), the division (1),
           grad_scale * min (1); c = 0 when max_norm <= 0 (coef is the argument itself)
    g'     g * coef: c + 1
    decay  1 - wd * lr: the product (1, of a term <= 1e-4 of the result) and the difference (1): 2;  p * decay: 1
           -> 3 |p|
    m'     1 - beta1 (1), its product with g' (1), the sum (1), on top of g' (c + 1): (c + 4) |(1 - beta1) g'|;
           beta1 * m (1) and the sum (1): 2 |beta1 m|
    v'     1 - beta2 (1), * g' (1), * g' (1), the sum (1), g' twice (2 c + 2): (2 c + 6) (1 - beta2) g'^2;
           beta2 * v (1) and the sum (1): 2 beta2 v
    denom  sqrtf halves the relative error of v' and adds 1; bc2_sqrt is a rounded float (1); the division (1); + eps (1):
           E_v / (2 sqrt(v')) + 4 |denom|   (E_v in units, absolute)
    update m' / denom (1), step = lr / bc1 with bc1 a rounded float (2), step * quotient (1):
           step E_m / denom + |upd| (E_denom / denom + 4)
    p'     the difference (1, of |p decay| + |upd| at most): 3 |p| + E_upd + |p| + |upd|
The sum is multiplied by ONE factor of 2: a compiler that fuses a multiply-add drops a rounding but changes the order in which the
remaining ones combine, and the count is first order.  Three units of the smallest denormal (2^-149) per tensor cover operations
whose result is below the normal range (none in the crafted inputs: |g coef| >= 1e-18 is asserted, so g'^2 >= 1e-36 stays
normal; the floor keeps the bound from being exactly zero where the terms are).
Outside the segments the bound is zero: the buffers must keep their bits.
"""
from __future__ import annotations

import functools
import math
import types

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
F32 = np.float32
BETA2, EPS = 0.99, 1e-8
KERNEL_GRID_SPAN = 4096 * 256           # k_adam: elements of a segment one sweep of the largest grid covers
NORM_SWEEP = 1024 * 256 * 4 * 4         # k_sq_partials: floats per sweep (1024 x 256 threads, four float4 each)


def _r32(x):
    return float(F32(x))


def _coef(max_norm, grad_scale, sq_norm, total_has_scale=True):
    gs = _r32(grad_scale)
    if not _r32(max_norm) > 0.0:
        return gs
    total = math.sqrt(float(sq_norm)) * (gs if total_has_scale else 1.0)
    return gs * min(_r32(max_norm) / (total + _r32(1e-6)), 1.0)


def _mask(n, segments):
    inside = np.zeros(n, dtype=bool)
    for b, e in segments:
        inside[b:e] = True
    return inside


def step_f64(p, g, m, v, segments, lr, beta1, beta2, eps, wd, t, max_norm, grad_scale, sq_norm, _variant=None):
    """The reference step in float64 on flat arrays: returns (p', m', v'); the inputs are not modified.  ``segments`` is a list
    of [begin, end) pairs; ``sq_norm`` = |g|^2 of the un-averaged gradient (not read when max_norm <= 0)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    lr, beta1, beta2, eps, wd = _r32(lr), _r32(beta1), _r32(beta2), _r32(eps), _r32(wd)
    coef = _coef(max_norm, grad_scale, sq_norm, total_has_scale=_variant != "d")
    tb = t - 1 if _variant == "c" else t
    with np.errstate(divide="ignore", invalid="ignore"):
        bc1 = 1.0 - beta1 ** tb
        bc2s = math.sqrt(1.0 - beta2 ** tb)
        decay = 1.0 - wd * lr
        gi = g * coef
        mn = beta1 * m + (1.0 - beta1) * gi
        vn = beta2 * v + (1.0 - beta2) * gi * gi
        if _variant == "b":
            denom = (np.sqrt(vn) + eps) / bc2s
        else:
            denom = np.sqrt(vn) / bc2s + eps
        upd = (lr / bc1) * (mn / denom) if bc1 != 0.0 else np.full_like(mn, np.nan)
        pn = (p - upd) * decay if _variant == "a" else p * decay - upd
    inside = _mask(p.size, segments)
    if _variant == "f":
        for b, e in segments:
            if e > b:
                inside[e - 1] = False
    if _variant == "g":
        for b, e in segments:
            inside[b + KERNEL_GRID_SPAN:e] = False      # 1 048 576: where the grid-stride loop runs a second time
    po, mo, vo = np.where(inside, pn, p), np.where(inside, mn, m), np.where(inside, vn, v)
    if _variant == "e":
        real = _mask(p.size, segments)
        for b, e in segments:
            po[e:e + 8] = np.where(real[e:e + 8], po[e:e + 8], p[e:e + 8] * decay)
    return po, mo, vo


def step_f32(p, g, m, v, segments, lr, beta1, beta2, eps, wd, t, max_norm, grad_scale, sq_norm):
    """The same step in numpy float32 in the oracle's operation order (AdamOneCycle.step: python-double scalars rounded to float32
    where they meet a tensor, mul_ / add_(alpha) / addcmul_(value) / addcdiv_(value))."""
    p, g, m, v = (np.asarray(a, dtype=F32) for a in (p, g, m, v))
    lr, beta1, beta2, eps, wd = _r32(lr), _r32(beta1), _r32(beta2), _r32(eps), _r32(wd)
    gs = F32(grad_scale)
    if _r32(max_norm) > 0.0:
        total = np.sqrt(F32(sq_norm)) * gs
        coef = gs * np.minimum(F32(max_norm) / (total + F32(1e-6)), F32(1.0))
    else:
        coef = gs
    bc1 = 1.0 - beta1 ** t
    bc2 = 1.0 - beta2 ** t
    gi = g * F32(coef)
    pn = p * F32(1.0 - wd * lr)
    mn = m * F32(beta1) + gi * F32(1.0 - beta1)
    vn = v * F32(beta2) + F32(1.0 - beta2) * gi * gi
    denom = np.sqrt(vn) / F32(math.sqrt(bc2)) + F32(eps)
    pn = pn + F32(-lr / bc1) * (mn / denom)
    inside = _mask(p.size, segments)
    return np.where(inside, pn, p), np.where(inside, mn, m), np.where(inside, vn, v)


def bounds(p, g, m, v, segments, lr, beta1, beta2, eps, wd, t, max_norm, grad_scale, sq_norm, _ref=None):
    """Per-element absolute bounds (E_p, E_m, E_v) of a float32 evaluation of the step against ``step_f64``; the count is in
    the module docstring.  Zero outside the segments.  ``_ref``: the result of step_f64 on the same arguments, if at hand (the
    update's own magnitude enters E_p)."""
    kw = dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, wd=wd, t=t, max_norm=max_norm, grad_scale=grad_scale, sq_norm=sq_norm)
    ref = step_f64(p, g, m, v, segments, **kw) if _ref is None else _ref
    p, g, m, v = (np.abs(np.asarray(a, dtype=np.float64)) for a in (p, g, m, v))
    lr, beta1, beta2, eps, wd = _r32(lr), _r32(beta1), _r32(beta2), _r32(eps), _r32(wd)
    c = 6.0 if _r32(max_norm) > 0.0 else 0.0
    coef = abs(_coef(max_norm, grad_scale, sq_norm))
    step = lr / (1.0 - beta1 ** t)
    bc2s = math.sqrt(1.0 - beta2 ** t)
    gi = g * coef
    # in units of u, on the magnitudes of the terms
    e_m = 2.0 * beta1 * m + (c + 4.0) * (1.0 - beta1) * gi
    e_v = 2.0 * beta2 * v + (2.0 * c + 6.0) * (1.0 - beta2) * gi * gi
    rt = np.sqrt(beta2 * v + (1.0 - beta2) * gi * gi)
    denom = rt / bc2s + eps
    e_rt = np.where(rt > 0.0, e_v / (2.0 * np.where(rt > 0.0, rt, 1.0)), 0.0)
    e_den = e_rt / bc2s + 4.0 * denom
    upd = step * np.abs(ref[1]) / denom
    e_upd = step * e_m / denom + upd * (e_den / denom + 4.0)
    e_p = 3.0 * p + e_upd + (p + upd)
    inside = _mask(p.size, segments)
    return tuple(np.where(inside, 2.0 * U * e + 3.0 * TINY, 0.0) for e in (e_p, e_m, e_v))


def step_bounds(p, g, m, v, segments, **kw):
    """(reference (p', m', v'), bounds (E_p, E_m, E_v)) of one crafted call."""
    ref = step_f64(p, g, m, v, segments, **kw)
    return ref, bounds(p, g, m, v, segments, _ref=ref, **kw)


def bf16_bits(x):
    """float32 -> bfloat16 bit patterns (uint16), round to nearest even; a NaN stays a quiet NaN."""
    b = np.asarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((b >> 16) | 0x40).astype(np.uint16), r)


def bf16_bits_truncated(x):
    return (np.asarray(x, dtype=F32).view(np.uint32) >> 16).astype(np.uint16)


# wrong variants: name -> (what it breaks, kind, function).  kind "step": same signature as step_f64; "shadow": as bf16_bits
MUTATIONS = {
    "a": ("decay applied after the Adam update", "step", functools.partial(step_f64, _variant="a")),
    "b": ("eps added before the division by sqrt(1 - beta2^t)", "step", functools.partial(step_f64, _variant="b")),
    "c": ("bias corrections with t - 1", "step", functools.partial(step_f64, _variant="c")),
    "d": ("clip from the un-averaged norm (grad_scale missing in total)", "step", functools.partial(step_f64, _variant="d")),
    "e": ("the gap after a segment decayed", "step", functools.partial(step_f64, _variant="e")),
    "f": ("the last element of a segment skipped", "step", functools.partial(step_f64, _variant="f")),
    "g": ("elements at or beyond 1 048 576 of a segment untouched", "step", functools.partial(step_f64, _variant="g")),
    "h": ("shadow by truncation instead of round-to-nearest-even", "shadow", bf16_bits_truncated),
}


# ---------------------------------------------------------------------------------------------------------------------------
# crafted inputs
# ---------------------------------------------------------------------------------------------------------------------------
LR_MAX, LR_START, LR_END = 0.003, 0.003 / 10, 0.003 / 10 / 1e4       # the shipped one-cycle schedule: peak, first step, last step


def _ps(name, t, beta1, wd, lr, max_norm, grad_scale, total):
    """``total`` = the norm of the averaged gradient the call is told about (None: sq_norm holds NaN and must not be read)."""
    sq = float("nan") if total is None else float(F32((total / grad_scale) ** 2))
    return types.SimpleNamespace(name=name, total=total, kw=dict(lr=lr, beta1=beta1, beta2=BETA2, eps=EPS, wd=wd, t=t,
                                                                 max_norm=max_norm, grad_scale=grad_scale, sq_norm=sq))


# steps 1, 2, 1000, 100 000; beta1 0.85 / 0.95; wd 0 / 0.01; lr at the peak, the first and the last step of the schedule (at the
# last, 3e-8, the update is below one ulp of an O(1) parameter); clip inactive / active / total == max_norm exactly (80 / 8 = 10:
# sqrtf and the product are exact); max_norm = 0 with a NaN in sq_norm; grad_scale 1 and 1/8
PARAM_SETS = [
    _ps("t1-noclip", 1, 0.95, 0.01, LR_START, 10.0, 1.0, 2.5),
    _ps("t1-clip", 1, 0.95, 0.01, LR_START, 10.0, 1.0, 400.0),
    _ps("t2-clip-gs8", 2, 0.85, 0.01, LR_MAX, 10.0, 0.125, 37.0),
    _ps("t2-total-eq-max", 2, 0.85, 0.0, LR_MAX, 10.0, 0.125, 10.0),
    _ps("t1000-lrend", 1000, 0.95, 0.01, LR_END, 10.0, 1.0, 3.0),
    _ps("t1000-gs8-noclip", 1000, 0.85, 0.0, LR_MAX, 10.0, 0.125, 0.5),
    _ps("t100000-lrend-clip-gs8", 100000, 0.95, 0.01, LR_END, 10.0, 0.125, 1234.0),
    _ps("t100000-nonorm", 100000, 0.85, 0.01, LR_MAX, 0.0, 1.0, None),
    _ps("t2-nonorm-gs8", 2, 0.95, 0.01, LR_MAX, 0.0, 0.125, None),
]
PARAM_SET = {ps.name: ps for ps in PARAM_SETS}
assert PARAM_SET["t2-total-eq-max"].kw["sq_norm"] == 6400.0

SINGLE_SIZES = [1, 255, 256, 257, 1048576, 1048577, 2500001]
# name -> (buffer length, segments).  Odd unaligned begins and ends; two segments that touch; empty segments between real ones; a
# short segment before a 1.2 M one (the grid is sized by the LONGEST) and after it; 64 segments (the most the entry takes)
SEGMENT_LISTS = {
    "odd": (5000, [(3, 1001), (1500, 1501), (2001, 4998)]),
    "touching": (1000, [(7, 300), (300, 777)]),
    "empties": (1000, [(5, 5), (10, 201), (250, 250), (260, 260), (301, 902), (1000, 1000)]),
    "short-long": (1300000, [(3, 40), (101, 101 + 1200001)]),
    "long-short": (1300000, [(5, 5 + 1200001), (1250001, 1250034)]),
    "64": (64 * 50, [(50 * k + 1 + k % 3, 50 * k + 40 + k % 2) for k in range(64)]),
}


def make_data(n, ps, seed=0):
    """(p, g, m, v) float32, length n.  |g| log-uniform over 1e-12 .. 1e3 and |p| over 1e-4 .. 10, signs mixed; m on the scale of g
    with its own sign, v on the scale of g^2; every 16th element's m nearly cancels (1 - beta1) g coef / beta1 (the bound has
    to work on the terms); elements with index % 97 in 40..47 hold g = m = v = 0 (decay only).  |g coef| >= 1e-18 is asserted, so
    that g'^2 stays a normal float32."""
    r = np.random.default_rng(1000 + seed)
    sign = lambda: r.integers(0, 2, n) * 2.0 - 1.0
    g = sign() * 10.0 ** r.uniform(-12.0, 3.0, n)
    p = sign() * 10.0 ** r.uniform(-4.0, 1.0, n)
    m = sign() * np.abs(g) * 10.0 ** r.uniform(-2.0, 1.0, n)
    v = g * g * 10.0 ** r.uniform(-2.0, 1.0, n)
    k = ps.kw
    coef = _coef(k["max_norm"], k["grad_scale"], 0.0 if ps.total is None else k["sq_norm"])
    idx = np.arange(n)
    c16 = idx % 16 == 5
    m[c16] = -(1.0 - k["beta1"]) / k["beta1"] * coef * g[c16] * (1.0 + r.uniform(-1e-3, 1e-3, int(c16.sum())))
    z = (idx % 97 >= 40) & (idx % 97 < 48)
    g[z] = m[z] = v[z] = 0.0
    p, g, m, v = (a.astype(F32) for a in (p, g, m, v))
    nz = g != 0
    assert not nz.any() or np.abs(g[nz].astype(np.float64) * coef).min() >= 1e-18
    return p, g, m, v


@functools.lru_cache(maxsize=2)
def case(n, ps_name, segments):
    """One crafted call, computed once and shared: data, reference and bounds (treat as read-only).  ``segments``: a tuple of pairs."""
    ps = PARAM_SET[ps_name]
    p, g, m, v = make_data(n, ps)
    seg = [tuple(s) for s in segments]
    ref, bnd = step_bounds(p, g, m, v, seg, **ps.kw)
    return types.SimpleNamespace(n=n, ps=ps, segments=seg, p=p, g=g, m=m, v=v, ref=ref, bounds=bnd, inside=_mask(n, seg))


# float32 bit patterns of the shadow's rounding edges: bf16 ties with an even / odd upper bit (both signs), one bit either side of
# a tie, +-0, denormals (smallest, largest, a tie), the largest finite float (rounds to infinity) and its neighbour below the tie
SHADOW_EDGE_BITS = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,
                             0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x80018000,
                             0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x3F800000, 0x40490FDB], dtype=np.uint32)
SHADOW_EDGE_EXPECT = np.array([0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F81, 0x3F80, 0x3F82, 0x3F81,
                               0x0000, 0x8000, 0x0000, 0x0080, 0x0000, 0x0002, 0x8002,
                               0x7F80, 0xFF80, 0x7F7F, 0x3F80, 0x4049], dtype=np.uint16)

# the norm: sizes around the float4 body / scalar tail and the 4 194 304-float sweep of k_sq_partials
NORM_SIZES = [1, 2, 3, 4, 5, 7, 1023, 1048575, 1048576, 1048577, 4194301, 4194304, 4194305, 4194311, 9000003]
NORM_SLOT = 262144 * 4            # floats per 262 144-float4 slot (one unrolled load of the whole grid)
# roundings on the longest chain of the norm at n = 9 000 003 (three sweeps): inside a float4 w*w and three fmaf (4), one fmaf into
# the accumulator per sweep (3), the scalar tail's fmaf (1), (a0 + a1) + (a2 + a3) (2), gd_wave_sum (6), the four wave sums (3):
# 19 in k_sq_partials; k_sum_partials over 1024 partials: a0 += part (1), (a0 + a1) + (a2 + a3) (2), gd_wave_sum (6), 16 wave sums
# (16), * scale (1): 26.  45 in all; every term is non-negative, so the relative error is at most 45 u (1 + 45 u)
NORM_CHAIN = 45


def planted_indices(n):
    """where a lone 1 is planted for size n: both ends, both sides of the float4 body's end, the first float of every slot"""
    idx = {0, n - 1, 4 * (n // 4) - 1, 4 * (n // 4)} | set(range(0, n, NORM_SLOT))
    return sorted(i for i in idx if 0 <= i < n)
