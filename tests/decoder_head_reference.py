"""Plain float64 reference of the generative decoder head (reference spt_backbone_mae.py:30-52,125-135, from the deconvolution rows on) by
torch autograd on the DENSE map, on crafted small maps.  torch / numpy only; imports no project code.

Dataflow of ``run``: per source stage a zero map (R = B H W sites, 128 channels) with the rows P_i scattered at the stage's sites ->
BatchNorm2d(train, biased variance over all R sites, eps1) + ReLU -> channel concat (384) -> conv2d 3 x 3, padding 1 -> BatchNorm2d(train,
eps2) + ReLU -> gather at ``pillar_cell``; loss = (out * up).sum().  Sites are rows of a channels-last (R, C) matrix, site (b H + y) W + x.

``run(case, ...)`` returns a dict of float64 tensors:
  out, dense (relu(bn2(Y)) on all sites, (R, C)), Y (R, C), mean2 / var2, mean_s{i} / var_s{i} (the stages), running_mean{i} / running_var{i} (i = 0..2 the
  stages, 3 the output BatchNorm; momentum, unbiased factor R / (R - 1) with R the DENSE count), num_batches_tracked (= 1: the modules
  start at 0), and the gradients dW (128, 384, 3, 3), dgamma2, dbeta2, dP{i}, dgamma{i}, dbeta{i}.
  Y_given (R, C): the gradients at a GIVEN conv output, straight-through: Y = conv(Z, w) + (Y_given - conv(Z, w)).detach() - a kernel's
    backward is judged at the kernel's own Y, so that forward rounding does not enter the gradient bounds ("backward_at").
  emulate=True: straight-through rounding nodes where the 16-bit head rounds - the Z operand and the conv weight (values), Y (value), dY
    (gradient), the input-gradient rows at the stages' active sites (gradient; the background's share is a closed form in float64 and
    is not rounded), dP (result).  All to bf16: the tile convolution multiplies fp16 operands, which are finer.
  dtype=torch.float32: the same graph in fp32 on the CPU (the fp32 head's yardstick).
  mutation: one of MUTATIONS, a deliberately wrong backward (or running variance) - tests/test_decoder_head_reference_cpu.py shows that
    every one of them lands far outside the bounds tests/test_decoder_head_gpu.py uses.  m1 - m6 keep every forward value (the change
    is straight-through), so they are exactly "a backward formula error".

``d_ref(case, kind)`` -> {tensor name: distance}: kind "bf16" = emulated run against the exact one (forward tensors; gradients with both
at the emulated run's own Y), kind "fp32" = the fp32 run against float64 in the same way.  Computed from the reference alone and cached.
``metrics(got, want)`` -> the same names: relative L2 for every tensor, dW per stage column block and tap ("dW[s1,k4]"), dP
additionally by worst row ("dP1.row": max row error over the RMS row norm).
"""
from __future__ import annotations

import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

C = 128
EPS1 = EPS2 = 1e-3
# the modules' momentum: large, so that the unbiased factor of the running variance is visible at rtol 1e-4 next to the initial value
MOMENTUM = 0.5
UPS = (1, 2, 4)
MUTATIONS = {
    "m1": "the four diagonal pad cells hold the background instead of zero (corner term of the closed form dropped)",
    "m2": "the pad column x = -1 holds the background (one edge term dropped)",
    "m3": "pillar rows ignored for pillars on row H - 1",
    "m4": "relu' = 1 at background sites for all channels",
    "m5": "one (active site, tap) pair dropped",
    "m6": "sites with x >= 8 floor(W / 8) get dY = 0 (the partial tile lost)",
    "m7": "running variance of the stages with the token-site count instead of R",
}


# ------------------------------------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------------------------------------
def upsampled(tok, Ys, Xs, u):
    """(n_tok * u * u,) fine cells of the coarse cells ``tok``, row (token, dy * u + dx)"""
    tok = np.asarray(tok, dtype=np.int64)
    x, r = tok % Xs, tok // Xs
    y, b = r % Ys, r // Ys
    d = np.arange(u)
    yy = (y * u)[:, None, None] + d[None, :, None]
    xx = (x * u)[:, None, None] + d[None, None, :]
    return ((b[:, None, None] * (Ys * u) + yy) * (Xs * u) + xx).reshape(-1)


def _cells(B, Ys, Xs, fixed, n_random, rng, allowed=None):
    """sorted coarse cells: ``fixed`` (b, y, x) triples + n_random more, drawn from ``allowed`` (a (B, Ys, Xs) bool mask) or anywhere"""
    occ = np.zeros((B, Ys, Xs), dtype=bool)
    for b, y, x in fixed:
        occ[b, y, x] = True
    free = np.flatnonzero(~occ.reshape(-1) & (np.ones(B * Ys * Xs, dtype=bool) if allowed is None else allowed.reshape(-1)))
    occ.reshape(-1)[rng.choice(free, size=n_random, replace=False)] = True
    return np.flatnonzero(occ.reshape(-1))


def _corners(B, Ys, Xs, items=None):
    return [(b, y, x) for b in (range(B) if items is None else items) for y in (0, Ys - 1) for x in (0, Xs - 1)]


def _box(B, Ys, Xs, y0, y1, x0, x1):
    m = np.zeros((B, Ys, Xs), dtype=bool)
    m[:, y0:y1, x0:x1] = True
    return m


def _geometry(name, rng):
    """-> B, H, W, [coarse cells per stage], pillar cells (sorted, unique)"""
    if name == "A" or name == "C":
        B, H, W = (1, 20, 28) if name == "A" else (2, 24, 16)
        n_rand = {"A": (30, 10, 5), "C": (40, 10, 3)}[name]
        toks = [_cells(B, H // u, W // u, _corners(B, H // u, W // u), n, rng) for u, n in zip(UPS, n_rand)]
        edges = [(b, 0, W // 2 - 1) for b in range(B)] + [(b, H - 1, W // 2) for b in range(B)] + [(b, H // 2, 0) for b in range(B)] + \
                [(b, H // 2 - 1, W - 1) for b in range(B)]
        pil = np.union1d(toks[0], _cells(B, H, W, edges, 40, rng))
    elif name == "B":
        B, H, W = 2, 8, 8
        toks = [_cells(B, 8, 8, _corners(B, 8, 8), 0, rng), _cells(B, 4, 4, [], 3, rng), _cells(B, 2, 2, [(1, 1, 0)], 0, rng)]
        fixed = _corners(B, 8, 8) + [(0, 0, 3), (0, 7, 4), (0, 3, 0), (0, 4, 7), (0, 3, 3), (1, 0, 5), (1, 7, 2), (1, 5, 0), (1, 2, 7), (1, 4, 5)]
        pil = _cells(B, 8, 8, fixed, 0, rng)
    elif name == "D":
        # every token inside fine rows 9..30 / columns 9..22 of its item: with the one-site halo the tile rows 1..3 / columns 1..2, so
        # every tile on the rim of the 5 x 4 tile grid is non-active
        B, H, W = 2, 40, 32
        toks = [_cells(B, 40, 32, [], 150, rng, _box(B, 40, 32, 9, 31, 9, 23)), _cells(B, 20, 16, [], 37, rng, _box(B, 20, 16, 5, 15, 5, 11)),
                _cells(B, 10, 8, [], 13, rng, _box(B, 10, 8, 3, 7, 3, 5))]
        fixed = _corners(B, 40, 32, items=(0,)) + [(0, 0, 15), (0, 39, 16), (0, 20, 0), (0, 19, 31), (0, 3, 3), (1, 36, 28), (1, 0, 9), (1, 39, 31)]
        pil = np.union1d(toks[0], _cells(B, H, W, fixed, 40, rng))
    elif name == "E":
        B, H, W = 1, 24, 40
        t1 = [(0, 0, x) for x in (0, 7, 8, 15, 16, 30, 39)] + [(0, y, 39) for y in (5, 7, 8, 16, 23)]       # fine x = 7 | 8, y = 7 | 8: a tile boundary
        t2 = [(0, 0, x) for x in (0, 3, 4, 11, 19)] + [(0, y, 19) for y in (3, 4, 8, 11)]                    # coarse 3 | 4 = fine 6..7 | 8..9
        t4 = [(0, 0, x) for x in (1, 2, 9)] + [(0, y, 9) for y in (1, 2, 5)]                                 # coarse 1 | 2 = fine 4..7 | 8..11
        toks = [_cells(B, H // u, W // u, t, 0, rng) for u, t in zip(UPS, (t1, t2, t4))]
        active = np.zeros(B * H * W, dtype=bool)
        for u, t in zip(UPS, toks):
            active[upsampled(t, H // u, W // u, u)] = True
        fixed = [(0, 23, 0), (0, 23, 20), (0, 12, 0), (0, 2, 0), (0, 1, 16), (0, 12, 35)]
        assert not any(active[(b * H + y) * W + x] for b, y, x in fixed)
        pil = _cells(B, H, W, fixed, 60, rng, ~active.reshape(B, H, W))
    elif name == "F":
        B, H, W = 2, 20, 28
        toks = [_cells(B, 20, 28, [(1, 0, 0)], 0, rng), _cells(B, 10, 14, [(1, 9, 13)], 0, rng), _cells(B, 5, 7, [(1, 2, 3)], 0, rng)]
        pil = _cells(B, H, W, [(1, 19, 27)], 0, rng)
    else:
        raise KeyError(name)
    return B, H, W, toks, pil


CASES = ("A", "B", "C", "D", "E", "F")
_SEEDS = {"A": 101, "B": 102, "C": 103, "D": 104, "E": 105, "F": 106}


@functools.lru_cache(maxsize=None)
def make_case(name):
    """geometry + seeded operands of one case (float64 CPU tensors; never modified)"""
    rng = np.random.default_rng(_SEEDS[name])
    gen = torch.Generator().manual_seed(_SEEDS[name])
    B, H, W, toks, pil = _geometry(name, rng)
    R = B * H * W
    c = types.SimpleNamespace(name=name, B=B, H=H, W=W, R=R, ups=UPS, tok=[torch.from_numpy(t) for t in toks],
                              sites=[torch.from_numpy(upsampled(t, H // u, W // u, u)) for u, t in zip(UPS, toks)],
                              pillar_cell=torch.from_numpy(np.asarray(pil, dtype=np.int64)))
    assert all(s.unique().numel() == s.numel() for s in c.sites) and c.pillar_cell.unique().numel() == c.pillar_cell.numel()
    c.M = c.pillar_cell.numel()
    c.conv_w = (torch.randn(C, 3 * C, 3, 3, generator=gen) * 0.05).double()
    c.gamma2, c.beta2 = (torch.rand(C, generator=gen) + 0.5).double(), (torch.randn(C, generator=gen) * 0.3).double()
    c.P, c.gamma, c.beta = [], [], []
    for s in c.sites:
        c.P.append(torch.randn(s.numel(), C, generator=gen).bfloat16().double())
        c.gamma.append((torch.rand(C, generator=gen) + 0.5).double())
        c.beta.append((torch.randn(C, generator=gen) * 0.3).double())
    c.up = torch.randn(c.M, C, generator=gen).double()
    # initial running statistics of the four BatchNorm2d modules (0..2 the stages, 3 the output's), float32-valued
    c.rm0 = [(torch.randn(C, generator=gen) * 0.1).double() for _ in range(4)]
    c.rv0 = [(torch.rand(C, generator=gen) * 0.1 + 0.05).double() for _ in range(4)]
    # the pair of m5: an active site and a tap whose output site is a pillar (the centre tap if a stage-1 token is one), so that the
    # dropped product carries a pillar row and not only the small dense part k0 + k1 Y of the output gradient
    pil, c.m5 = set(c.pillar_cell.tolist()), None
    for ky, kx in [(1, 1)] + [(a, b_) for a in range(3) for b_ in range(3) if (a, b_) != (1, 1)]:
        for s in torch.cat(c.sites).tolist():
            b, y, x = s // (H * W), (s // W) % H, s % W
            yo, xo = y - ky + 1, x - kx + 1
            if c.m5 is None and 0 <= yo < H and 0 <= xo < W and (b * H + yo) * W + xo in pil:
                c.m5 = (b, y, x, ky, kx)
    assert c.m5 is not None
    return c


def site_class(c, cells):
    """border class 3 * (0 top / 1 middle / 2 bottom) + (0 left / 1 middle / 2 right) of fine cells"""
    y, x = (cells // c.W) % c.H, cells % c.W
    cy = torch.where(y == 0, 0, torch.where(y == c.H - 1, 2, 1))
    cx = torch.where(x == 0, 0, torch.where(x == c.W - 1, 2, 1))
    return 3 * cy + cx


def active_tiles(c):
    """(B * ceil(H / 8) * ceil(W / 8),) bool: the 8 x 8 tiles whose one-site halo touches a site covered by a token of any stage"""
    act = torch.zeros(c.R, dtype=torch.bool)
    for s in c.sites:
        act[s] = True
    dil = F.max_pool2d(act.view(c.B, 1, c.H, c.W).float(), 3, 1, 1)[:, 0] > 0
    TH, TW = (c.H + 7) // 8, (c.W + 7) // 8
    pad = torch.zeros(c.B, TH * 8, TW * 8, dtype=torch.bool)
    pad[:, :c.H, :c.W] = dil
    return pad.view(c.B, TH, 8, TW, 8).any(4).any(2).flatten()


def tile_of(c, cells):
    TH, TW = (c.H + 7) // 8, (c.W + 7) // 8
    b, y, x = cells // (c.H * c.W), (cells // c.W) % c.H, cells % c.W
    return (b * TH + y // 8) * TW + x // 8


# ------------------------------------------------------------------------------------------------------------------------------
# the head
# ------------------------------------------------------------------------------------------------------------------------------
class _RoundGrad(torch.autograd.Function):
    """identity whose gradient is rounded to bf16 (where ``mask``, everywhere if None)"""

    @staticmethod
    def forward(ctx, x, mask):
        ctx.mask = mask
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        r = g.bfloat16().to(g.dtype)
        return (r if ctx.mask is None else torch.where(ctx.mask, r, g)), None


def _rnd(x):
    """x rounded to bf16, gradient straight through"""
    return x + (x.bfloat16().to(x.dtype) - x).detach()


def run(c, dtype=torch.float64, emulate=False, Y_given=None, mutation=None, grads=True):
    assert mutation is None or mutation in MUTATIONS
    B, H, W, R = c.B, c.H, c.W, c.R
    leaf = lambda t: t.to(dtype).clone().requires_grad_()                       # noqa: E731
    conv_w, g2, b2 = leaf(c.conv_w), leaf(c.gamma2), leaf(c.beta2)
    Ps, gs, bs = [leaf(t) for t in c.P], [leaf(t) for t in c.gamma], [leaf(t) for t in c.beta]
    up = c.up.to(dtype)
    res = {}
    Zs, bgs, act = [], [], []
    for i, (sites, P, g, b) in enumerate(zip(c.sites, Ps, gs, bs)):
        x = torch.zeros(R, C, dtype=dtype).index_copy(0, sites, P)
        mean, var = x.mean(0), x.var(0, unbiased=False)
        h = (x - mean) * torch.rsqrt(var + EPS1) * g + b
        z = torch.relu(h)
        on = torch.zeros(R, dtype=torch.bool)
        on[sites] = True
        if mutation == "m4":
            z = torch.where(on[:, None], z, h + (z - h).detach())
        Zs.append(z)
        act.append(on[:, None].expand(R, C))
        bgs.append(torch.relu(b - mean * torch.rsqrt(var + EPS1) * g))               # the value of every site without a token
        n_unb = sites.numel() if mutation == "m7" else R
        res["mean_s%d" % i], res["var_s%d" % i] = mean, var
        res["running_mean%d" % i] = (1 - MOMENTUM) * c.rm0[i].to(dtype) + MOMENTUM * mean
        res["running_var%d" % i] = (1 - MOMENTUM) * c.rv0[i].to(dtype) + MOMENTUM * var * (n_unb / (n_unb - 1) if n_unb > 1 else float("inf"))
        res["bg_signs%d" % i] = (int((bgs[-1] > 0).sum()), int((bgs[-1] == 0).sum()))
    Z, bg, w = torch.cat(Zs, 1), torch.cat(bgs), conv_w
    if emulate:
        Z, w = _rnd(_RoundGrad.apply(Z, torch.cat(act, 1))), _rnd(w)
    Zm = Z.view(B, H, W, 3 * C).permute(0, 3, 1, 2)
    Y = F.conv2d(Zm, w, None, 1, 1)
    if mutation in ("m1", "m2"):
        pad = torch.zeros(1, 1, H + 2, W + 2, dtype=dtype)
        if mutation == "m1":
            pad[0, 0, [0, 0, H + 1, H + 1], [0, W + 1, 0, W + 1]] = 1
        else:
            pad[0, 0, 1:H + 1, 0] = 1
        Ym = F.conv2d(F.pad(Zm, (1, 1, 1, 1)) + pad * bg[None, :, None, None], w, None, 1, 0)
        Y = Y.detach() + (Ym - Ym.detach())
    if mutation == "m5":
        b_, y_, x_, ky, kx = c.m5
        contrib = w[:, :, ky, kx] @ Zm[b_, :, y_, x_]
        hot = torch.zeros(B, 1, H, W, dtype=dtype)
        hot[b_, 0, y_ - ky + 1, x_ - kx + 1] = 1
        Y = Y - hot * (contrib - contrib.detach())[None, :, None, None]
    if emulate:
        Y = _RoundGrad.apply(_rnd(Y), None)
    if Y_given is not None:
        Y = Y + (Y_given.to(dtype).view(B, H, W, C).permute(0, 3, 1, 2) - Y).detach()
    if mutation == "m6":
        lost = (torch.arange(W) >= 8 * (W // 8))[None, None, None, :]
        Y = torch.where(lost, Y.detach(), Y)
    Yr = Y.permute(0, 2, 3, 1).reshape(R, C)
    mean2, var2 = Yr.mean(0), Yr.var(0, unbiased=False)
    a2 = torch.rsqrt(var2 + EPS2) * g2
    yr = Yr[c.pillar_cell]
    if mutation == "m3":
        yr = torch.where(((c.pillar_cell // W) % H == H - 1)[:, None], yr.detach(), yr)
    out = torch.relu((yr - mean2) * a2 + b2)
    res.update(out=out, dense=torch.relu((Yr - mean2) * a2 + b2), Y=Yr, mean2=mean2, var2=var2, mean3=mean2, var3=var2,
               running_mean3=(1 - MOMENTUM) * c.rm0[3].to(dtype) + MOMENTUM * mean2,
               running_var3=(1 - MOMENTUM) * c.rv0[3].to(dtype) + MOMENTUM * var2 * (R / (R - 1)), num_batches_tracked=1)
    if grads:
        leaves = [conv_w, g2, b2] + [t for tr in zip(Ps, gs, bs) for t in tr]
        names = ["dW", "dgamma2", "dbeta2"] + [n + str(i) for i in range(len(Ps)) for n in ("dP", "dgamma", "dbeta")]
        for n, g in zip(names, torch.autograd.grad((out * up).sum(), leaves)):
            res[n] = _rnd(g) if (emulate and n.startswith("dP")) else g
    return {k: (v.detach().double() if torch.is_tensor(v) else v) for k, v in res.items()}


def backward_at(c, Y_given, **kw):
    return run(c, Y_given=Y_given, **kw)


# ------------------------------------------------------------------------------------------------------------------------------
# distances
# ------------------------------------------------------------------------------------------------------------------------------
FORWARD = ("out", "dense", "mean2", "var2")
GRADS = ("dgamma2", "dbeta2") + tuple(n + str(i) for i in range(3) for n in ("dP", "dgamma", "dbeta"))


def _rel(got, want):
    return float((got.double() - want.double()).norm()) / max(float(want.double().norm()), 1e-300)


def metrics(got, want, names=None):
    """{name: distance} over the tensors both dicts hold (see the module docstring)"""
    m = {}
    for n in FORWARD + GRADS:
        if n in got and n in want and (names is None or n in names):
            m[n] = _rel(got[n], want[n])
            if n.startswith("dP"):
                d, wt = got[n].double() - want[n].double(), want[n].double()
                m[n + ".row"] = float(d.norm(dim=1).max()) / max(float(wt.norm(dim=1).pow(2).mean().sqrt()), 1e-300)
    if "dW" in got and "dW" in want and (names is None or "dW" in names):
        for s in range(3):
            for k in range(9):
                m["dW[s%d,k%d]" % (s, k)] = _rel(got["dW"][:, s * C:(s + 1) * C, k // 3, k % 3], want["dW"][:, s * C:(s + 1) * C, k // 3, k % 3])
    return m


@functools.lru_cache(maxsize=None)
def exact(name):
    """the float64 run of a case (shared; never modified)"""
    return run(make_case(name))


@functools.lru_cache(maxsize=None)
def d_ref(name, kind):
    c = make_case(name)
    kw = dict(emulate=True) if kind == "bf16" else dict(dtype=torch.float32)
    low = run(c, **kw)
    d = metrics({k: low[k] for k in FORWARD}, exact(name))
    d.update(metrics({k: v for k, v in low.items() if k not in FORWARD}, backward_at(c, low["Y"])))
    return d


MARGIN = {"bf16": 3.0, "fp32": 10.0}


def bounds(name, kind):
    """the GPU test's bound per tensor: 3 x d_ref on the 16-bit routes (fp32 accumulation order over K = 3456, fp16-versus-bf16
    placement of the operand rounding, single ReLU / bf16-boundary flips), 10 x d_ref on the fp32 route (the three-term kernel and the
    library GEMMs sum in other orders; a formula error is >= 1e-3)"""
    return {k: MARGIN[kind] * v for k, v in d_ref(name, kind).items()}


# running statistics / batch statistics: rtol, and an absolute floor for elements near zero (the figures of
# test_conv3x3_tiles_matches_dense_conv)
def close_ratio(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|): <= 1 is torch.allclose"""
    return float(((got.double() - want.double()).abs() / (atol + rtol * want.double().abs())).max())
