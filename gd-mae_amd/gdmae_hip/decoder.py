"""Sparse-aware generative decoder: the same arithmetic as the reference's dense decoder
(pcdet/models/backbones_3d/spt_backbone_mae.py:120-143: densify -> ConvTranspose2d(k = s) + BN2d + ReLU per
source stage -> cat -> Conv2d 3x3 + BN2d + ReLU -> gather at all pillar sites), restructured around what
is actually dense.

Exact identities used (no approximation):
* ConvTranspose2d with kernel = stride maps each input site to its own s x s output block, so on a map
  that is zero outside the active set it is one token GEMM  P = X @ W.view(Cin, s*s*Cout)  and zeros
  elsewhere.
* BatchNorm2d statistics over ALL B*Y*X sites of such a map follow from the token values alone
  (sum and sum of squares over tokens, divided by the dense count); after BN + ReLU every empty site
  holds the same per-channel constant relu(beta - gamma*mean/sigma).
* The concatenated 384-channel map is therefore "constant background + token rows".
* The forward 3x3 convolution is the one genuinely dense contraction.  Two forward schedules:
  "tiles" (throughput mode, bf16): the library's own bf16-MFMA implicit GEMM over the ACTIVE 8x8 TILES of the map
  (csrc/conv_tiles.hip).  The 384-channel input map is never written (the kernel gathers the deconvolution rows through the stages'
  cell -> token maps and applies BN + ReLU on the way into LDS), sites outside the active tiles hold one of 9 border-class
  constants, and the BatchNorm statistics of the output come out of the same kernel.
  "dense_map": the map is materialised (fill + three row scatters into column slices) and convolved by csrc/conv_dense.hip - with
  bf16 operands in the throughput mode, as the fp32-grade three-term product in the fp32 parity mode; F.conv2d only as the last
  fallback for channel counts those kernels do not serve.
  Either way the output is only consumed at the M pillar sites, so BN + ReLU are applied to the gathered rows only.
* In the backward the gradient of the conv output is an affine function of the conv output plus M sparse rows, dY = k0 + k1*Y + rows,
  and the conv input gradient is only needed where the input is not background.  The background's share (input gradient summed over
  all other sites, weight gradient against the constant) is a closed form of 9 border-region sums (the "region algebra").  Per source
  stage one of three backward schedules, chosen by the forward and carried to the backward:
  "rulebook": dY once in the conv output's tile-compact layout (gdmae_decoder_dy), the input-gradient rows as an implicit GEMM over the
  stage's (site, tap) rulebook (gdmae_spconv), the weight gradient as nine gathered products in one grouped launch (gdmae_tap_dw);
  "block" (upsampling stride 2 / 4): the same, with the weight gradient on token blocks (gdmae_decoder_block_dw, csrc/decoder_blocks.hip);
  "taps" (GDMAE_DEC_BWD=taps, and whatever the tile path does not serve): the 9 shifted dY rows of the active sites are gathered
  (gdmae_conv3x3_grad_taps) and two library GEMMs give the input-gradient rows and the weight gradient.
  The M sparse rows, a2 * relu'(a2 y + b2) * dout, are an array only for "taps"; the other two form them where they are added
  (gdmae_decoder_dy_rows, gdmae_border_sums_rows), from the conv output that thread holds anyway.

Autograd: one hand-derived Function (DecoderHead) from the token-side deconvolution rows to the pillar rows.
"""
from __future__ import annotations

import os
from collections import namedtuple
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn.functional as F

from . import bn as gbn
from . import lib as L
from . import ops, packing
from . import plan as gplan
from . import timing

# conv_out backward of the tile path: "implicit" = tile-compact output gradient + implicit-GEMM input gradient + gathered grouped
# weight gradient (no tap matrix, no library GEMM); "taps" = the round-2 schedule (gdmae_conv3x3_grad_taps + two library GEMMs)
CONV_BWD = os.environ.get("GDMAE_DEC_BWD", "implicit")
# stages with an upsampling stride of 2 / 4 in the "implicit" backward: "1" = the weight gradient on token blocks (csrc/decoder_blocks.hip:
# each token's dY halo staged once, the Zd rows never written), "0" = the rulebook path for every stage (A/B runs)
BLOCK_BWD = os.environ.get("GDMAE_DEC_BLOCK", "1")
# "1" = the pillar rows of dY (a2 * relu' * dout) are formed inside gdmae_decoder_dy_rows / gdmae_border_sums_rows, which hold the conv
# output of the site anyway; "0" = gdmae_rows_bwd writes them as an (M, C2) fp32 array first (A/B runs).  The "taps" schedule reads the array.
DY_ROWS = os.environ.get("GDMAE_DEC_DY_ROWS", "1") != "0"
# "1" = the tile path gathers the pillar rows and writes their BatchNorm + ReLU in one launch; "0" = gather, then a second pass over the rows
GATHER_FUSED = os.environ.get("GDMAE_DEC_GATHER_FUSED", "1") != "0"
# tile convolution: "1" = leading source stages that are background over a tile's whole halo patch are not multiplied (the accumulators
# start from the pre-accumulators of gdmae_conv3x3_tiles_pack_pre, workgroups pair the tiles in class order; the same bits), "0" = every
# tile runs every phase from zero in ascending pairs (A/B runs), "ascending" = the skip on ascending pairs (what the pairing order is worth)
CT_SKIP = os.environ.get("GDMAE_CT_SKIP", "1")


# sparse_decoder(..., pre_conv_hook=callable): invoked once right before the decoder's tile convolution is launched (the one
# matrix-core-bound launch of the step) - the training loop issues the NEXT batch's geometry plan there, so that the plan's
# atomics-and-scatter kernels on the side stream run under it instead of under the memory-bound start of the forward (bench.py --plan-at
# conv).  The hook travels with the call (SPTBackboneMAE.prefetch_plan_under_decoder keeps it on the module until its forward), there is
# no process-global state.

def colstats(x2d: torch.Tensor):
    """(sum, sumsq) per column of a contiguous (R, C) fp32/bf16 device matrix, as float64 (C,) tensors."""
    R, C = x2d.shape
    assert x2d.is_contiguous() and x2d.dtype in (torch.float32, torch.bfloat16)
    out = torch.empty(2 * C, dtype=torch.float64, device=x2d.device)
    ws = torch.empty(L.load().gdmae_colstats_workspace_bytes(C), dtype=torch.uint8, device=x2d.device)
    L.call("gdmae_colstats", L.ptr(x2d), R, C, int(x2d.dtype == torch.bfloat16), L.ptr(out), L.ptr(ws), L.stream())
    return out[:C], out[C:]


def _gather_slice(table2d, idx, col0, ncol):
    es = table2d.element_size()
    out = torch.empty(idx.numel(), ncol, dtype=table2d.dtype, device=table2d.device)
    L.call("gdmae_gather_rows_strided", L.ptr(table2d), L.ptr(idx), idx.numel(), ncol * es, table2d.shape[1] * es,
           col0 * es, L.ptr(out), L.stream())
    return out


def _scatter_slice(src2d, idx, table2d, col0):
    es = table2d.element_size()
    src2d = src2d.contiguous()
    assert src2d.dtype == table2d.dtype
    L.call("gdmae_scatter_rows_strided", L.ptr(src2d), L.ptr(idx), idx.numel(), src2d.shape[1] * es,
           table2d.shape[1] * es, col0 * es, L.ptr(table2d), L.stream())


def _bf(t):
    return int(t.dtype == torch.bfloat16)


# S_k = sum of the output gradient over the sites s whose tap s+k lies inside the map, from the 9 region sums
# [all, row 0, row H-1, col 0, col W-1, corner(0,0), corner(0,W-1), corner(H-1,0), corner(H-1,W-1)]
_TAP_REGION = torch.zeros(9, 9, dtype=torch.float64)
for _ky in (-1, 0, 1):
    for _kx in (-1, 0, 1):
        _k = (_ky + 1) * 3 + (_kx + 1)
        _TAP_REGION[_k, 0] = 1
        if _ky:
            _TAP_REGION[_k, 1 if _ky < 0 else 2] = -1
        if _kx:
            _TAP_REGION[_k, 3 if _kx < 0 else 4] = -1
        if _ky and _kx:
            _TAP_REGION[_k, 5 + (0 if _ky < 0 else 2) + (0 if _kx < 0 else 1)] = 1


_REGION_CONSTS = {}


def _region_consts(dev, B, H, W):
    """Device copies of the tap/region matrix and the region site counts (cached: a host->device copy inside the
    backward would stall the host until the GPU has caught up)."""
    key = (dev, B, H, W)
    if key not in _REGION_CONSTS:
        R = B * H * W
        cnt = torch.tensor([R, B * W, B * W, B * H, B * H, B, B, B, B], dtype=torch.float64)
        _REGION_CONSTS[key] = (_TAP_REGION.to(dev), cnt.to(dev))
    return _REGION_CONSTS[key]


@dataclass(frozen=True, eq=False)
class TileConv:
    """What the tile convolution of a call reads besides the rows: the active-tile set and, per source stage, the cell -> token
    map and the upsampling stride."""
    tiles: gplan.DecoderTiles
    maps: list
    ups: list
    skip: str = "0"           # CT_SKIP as the caller read it: "0", "1" or "ascending"


@dataclass(frozen=True, eq=False)
class DecoderGeom:
    """The non-tensor description of one DecoderHead call: the (B, H, W) map, the eps of the stages' BatchNorm2d and of the output's,
    the compute dtype, and the tile convolution's geometry (None: the map is materialised)."""
    B: int
    H: int
    W: int
    eps1: float
    eps2: float
    cdt: torch.dtype
    tile_conv: Optional[TileConv] = None


# What either forward schedule hands to the driver:
#   y2                 conv output: tile-compact (n_act * 64, C2) or dense (R, C2)
#   yrows              (M, C2) conv output at the pillar sites
#   stats2, ab2, mv2   f64 mean | rstd, f32 a | b, f32 mean | biased var of the output BatchNorm2d
#   Z                  (R, Cin) materialised map (dense_map; None on tiles)
#   tile_slot, ybg     tile -> slot of y2 and the 9 border-class constants outside the tiles (tiles; None on dense_map)
#   bgz                (Cin,) value of every non-active site of the map
#   out                (M, C2) fp32 relu(a2 * yrows + b2) where the schedule wrote it with the gather (tiles, GATHER_FUSED), else None
_Forward = namedtuple("_Forward", "y2 yrows stats2 ab2 mv2 Z tile_slot ybg bgz out", defaults=(None,))


def _forward_tiles(geom, pre_conv_hook, conv_w, gamma2, beta2, pillar_cell, Ps, widths, ab_l, bn2):
    """own bf16-MFMA 3x3 convolution over the active tiles; the dense 384-channel map is never built"""
    B, H, W, cdt, tc = geom.B, geom.H, geom.W, geom.cdt, geom.tile_conv
    dt, k, dev = tc.tiles, len(Ps), Ps[0].device
    lib = L.load()
    Cin = sum(widths)
    C2 = 128
    Wp = torch.empty(lib.gdmae_conv3x3_tiles_packed_bytes(k), dtype=torch.uint8, device=dev)
    bgz = torch.empty(Cin, dtype=cdt, device=dev)
    ybg = torch.empty(9, C2, dtype=cdt, device=dev)
    a_l, b_l = [ab[:w] for ab, w in zip(ab_l, widths)], [ab[w:] for ab, w in zip(ab_l, widths)]
    # the path is the call's (TileConv.skip), and needs a tile set that came with its classes
    skip = tc.skip != "0" and k >= 2 and dt.tile_class is not None and dt.tile_order is not None
    pre = order = None
    if skip:
        pre = torch.empty(k - 1, C2, dtype=torch.float32, device=dev)
        L.call("gdmae_conv3x3_tiles_pack_pre", L.ptr(conv_w), C2, Cin, L.host_ptrs(b_l), k, L.ptr(Wp), L.ptr(bgz), L.ptr(ybg), L.ptr(pre),
               L.stream())
        order = dt.tile_order if tc.skip != "ascending" else torch.arange(dt.n_act, dtype=torch.int32, device=dev)
    else:
        L.call("gdmae_conv3x3_tiles_pack", L.ptr(conv_w), C2, Cin, L.host_ptrs(b_l), k, L.ptr(Wp), L.ptr(bgz), L.ptr(ybg),
               L.stream())
    y2 = torch.empty(max(dt.n_act, 1) * 64, C2, dtype=cdt, device=dev)
    stats2 = torch.empty(2 * C2, dtype=torch.float64, device=dev)
    ab2 = torch.empty(2 * C2, dtype=torch.float32, device=dev)
    mv2 = torch.empty(2 * C2, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.gdmae_conv3x3_tiles_workspace_bytes(dt.n_act), dtype=torch.uint8, device=dev)
    rm, rv, nb, mom = gbn.running_stats(bn2)
    flops = 2.0 * dt.n_act * 64 * C2 * 9 * Cin
    if pre_conv_hook is not None:        # work to issue (on another stream) right before the tile convolution
        pre_conv_hook()
    with timing.kernel("k_conv3x3_tiles", dt.n_act * 64 * (Cin + C2) * 2, flops,
                       {"dense_equivalent_TFLOPs_per_launch": round(2.0 * B * H * W * C2 * 9 * Cin / 1e12, 4), "active_tiles": dt.n_act}):
        L.call("gdmae_conv3x3_tiles_fwd_skip", L.host_ptrs([P.contiguous() for P in Ps]), L.host_ptrs(tc.maps), L.host_ptrs(a_l),
               L.host_ptrs(b_l), L.host_i32(tc.ups), k, L.ptr(Wp), L.ptr(ybg), L.ptr(dt.tile_list), dt.n_act, B, H, W,
               L.ptr(y2), L.ptr(gamma2), L.ptr(beta2), float(geom.eps2), mom, L.ptr(rm), L.ptr(rv), L.ptr(nb), L.ptr(stats2),
               L.ptr(ab2), L.ptr(mv2), L.ptr(dt.tile_class) if skip else None, L.ptr(order), L.ptr(pre), L.ptr(ws), L.stream())
    M = pillar_cell.numel()
    yrows = torch.empty(M, C2, dtype=cdt, device=dev)
    out = None
    if GATHER_FUSED:
        out = torch.empty(M, C2, dtype=torch.float32, device=dev)
        L.call("gdmae_tiles_gather_rows_affine_relu", L.ptr(y2), L.ptr(dt.tile_slot), L.ptr(ybg), L.ptr(pillar_cell), M, H, W, C2,
               L.ptr(ab2), L.ptr(ab2[C2:]), L.ptr(yrows), L.ptr(out), L.stream())
    else:
        L.call("gdmae_tiles_gather_rows", L.ptr(y2), L.ptr(dt.tile_slot), L.ptr(ybg), L.ptr(pillar_cell), M, H, W, C2, 2,
               L.ptr(yrows), L.stream())
    return _Forward(y2, yrows, stats2, ab2, mv2, None, dt.tile_slot, ybg, bgz, out)


def _forward_dense_map(geom, conv_w, gamma2, beta2, pillar_cell, sites, Ps, widths, ab_l, bn2):
    """the map materialised (fill + one row scatter per stage) in front of a dense convolution"""
    B, H, W, cdt = geom.B, geom.H, geom.W, geom.cdt
    R = B * H * W
    bgz = torch.relu(torch.cat([ab[w:] for ab, w in zip(ab_l, widths)])).to(cdt)   # value of every non-active site
    Z = torch.empty(R, sum(widths), dtype=cdt, device=Ps[0].device)
    L.call("gdmae_fill_rows", L.ptr(bgz), R, Z.shape[1], Z.element_size(), L.ptr(Z), L.stream())
    col = 0
    for P, st, ab, w in zip(Ps, sites, ab_l, widths):
        L.call("gdmae_rows_affine_relu_scatter", L.ptr(P), _bf(P), L.ptr(st), P.shape[0], w, L.ptr(ab), L.ptr(ab[w:]), L.ptr(Z), _bf(Z),
               Z.shape[1], col, L.stream())
        col += w
    # csrc/conv_dense.hip: bf16 operands in the throughput mode, the fp32-grade three-term form in the parity mode; F.conv2d for the
    # channel counts it does not serve
    from . import dense as gdense
    C2o = conv_w.shape[0]
    if cdt == torch.bfloat16 and Z.shape[1] % 64 == 0 and conv_w.dtype == torch.float32:
        y2 = gdense.Conv3x3Dense.apply(Z.view(B, H, W, -1).permute(0, 3, 1, 2), conv_w.detach(), None, 1, None).permute(0, 2, 3, 1)
    elif cdt == torch.float32 and Z.shape[1] % 64 == 0:
        y2 = gdense.conv3x3_f32_rows(Z.view(B, H, W, -1), conv_w.detach().float().contiguous(), None, 1)[..., :C2o]
    else:
        wc = ops.shadow(conv_w, cdt)
        with torch.autocast("cuda", enabled=False):
            y2 = F.conv2d(Z.view(B, H, W, -1).permute(0, 3, 1, 2), wc, None, 1, 1).permute(0, 2, 3, 1)
    if not y2.is_contiguous():
        y2 = y2.contiguous()
    y2 = y2.view(R, -1)
    stats2, ab2, mv2 = gbn.fold(y2, R, gamma2, beta2, geom.eps2, bn2)
    yrows = ops.gather_rows_raw(y2, pillar_cell)                       # (M, C2) conv outputs at the pillar sites
    return _Forward(y2, yrows, stats2, ab2, mv2, Z, None, None, bgz)


def _backward_schedule(geom, conv_w, sites, Ps, widths, fwd):
    """-> (region algebra through the native entry?, per source stage "block" / "rulebook" / "taps").  Decided here, by the forward,
    from the switches and the call; the backward only reads it."""
    C2 = fwd.y2.shape[1]
    native = conv_w.dtype == torch.float32 and conv_w.is_contiguous() and C2 % 8 == 0
    tc = geom.tile_conv
    if not (CONV_BWD == "implicit" and fwd.tile_slot is not None and fwd.y2.dtype == torch.bfloat16 and native and C2 == 128
            and all(w == 128 for w in widths) and tc is not None):
        return native, ["taps"] * len(widths)
    stage_bwd = []
    for P, st, u in zip(Ps, sites, tc.ups):
        n, u = P.shape[0], int(u)
        # workspace of 0 bytes: more tokens per slice than the block kernel serves
        block = (BLOCK_BWD != "0" and u in (2, 4) and P.dtype == torch.bfloat16 and P.is_contiguous() and st.numel() >= n
                 and int(L.load().gdmae_decoder_block_dw_workspace_bytes(n, u)) > 0)
        stage_bwd.append("block" if block else "rulebook")
    return native, stage_bwd


def _save(ctx, **named):
    """save_for_backward by name: every value is a tensor, None or a list of them; _saved gives them back under their names."""
    ctx.saved_names = [(name, len(v) if isinstance(v, (list, tuple)) else None) for name, v in named.items()]
    ctx.save_for_backward(*[t for v in named.values() for t in (v if isinstance(v, (list, tuple)) else (v,))])


def _saved(ctx) -> SimpleNamespace:
    sv, out, j = ctx.saved_tensors, SimpleNamespace(), 0
    for name, n in ctx.saved_names:
        setattr(out, name, sv[j] if n is None else sv[j:j + n])
        j += 1 if n is None else n
    return out


def _bn2_backward(s, dout, R, direct):
    """BatchNorm2d #2 (+ReLU) at the pillar rows: dY = k0 + k1*Y + rows[pillar sites], rows = a*dh (_pillar_rows).
    -> (dout (M, C2) fp32 contiguous, st2 f64[3 C2] column sums, k01 f32[2 C2], dgamma2, dbeta2)"""
    yrows, ab2 = s.yrows, s.ab2
    M, C2 = yrows.shape
    dev = yrows.device
    dout = dout.float().contiguous()
    st2 = torch.empty(3 * C2, dtype=torch.float64, device=dev)
    ws = torch.empty(L.load().gdmae_rows_bwd_stats_workspace_bytes(C2), dtype=torch.uint8, device=dev)
    L.call("gdmae_rows_bwd_stats", L.ptr(yrows), _bf(yrows), None, M, C2, L.ptr(ab2), L.ptr(ab2[C2:]), L.ptr(dout), 0, C2, 0,
           L.ptr(st2), L.ptr(ws), L.stream())
    dgamma2, dbeta2, k01 = gbn.bwd_coeffs(st2, 3, s.stats2, ab2, s.gamma2, R, None, direct)
    return dout, st2, k01, dgamma2, dbeta2


def _pillar_rows(s, dout):
    """rows (M, C2) fp32 = a2 * (a2 * yrows + b2 > 0 ? dout : 0), the sparse part of dY as an array (for the schedules that read one)"""
    yrows, ab2 = s.yrows, s.ab2
    M, C2 = yrows.shape
    zero = torch.zeros(2 * C2, dtype=torch.float32, device=yrows.device)
    rows = torch.empty(M, C2, dtype=torch.float32, device=yrows.device)
    L.call("gdmae_rows_bwd", L.ptr(yrows), _bf(yrows), None, M, C2, L.ptr(ab2), L.ptr(ab2[C2:]), L.ptr(zero), L.ptr(zero[C2:]),
           L.ptr(dout), 0, C2, 0, L.ptr(rows), 0, L.stream())
    return rows


def _region_sums(s, rows, dout, B, H, W):
    """(16, C2) f64 sums of Y (0..7) and of the pillar rows (8..15) over border rows / border columns / corners (regions 1..8 of
    _TAP_REGION; region 0, all sites, follows from the BatchNorm statistics).  rows None: the border pillars' rows are formed from dout."""
    y2 = s.y2
    C2 = y2.shape[1]
    reg = torch.empty(16, C2, dtype=torch.float64, device=y2.device)
    ws = torch.empty(L.load().gdmae_border_sums_workspace_bytes(B, C2), dtype=torch.uint8, device=y2.device)
    if rows is None:
        L.call("gdmae_border_sums_rows", L.ptr(y2), _bf(y2), L.ptr(s.tile_slot), L.ptr(s.ybg), L.ptr(dout), L.ptr(s.yrows), L.ptr(s.ab2),
               L.ptr(s.ab2[C2:]), L.ptr(s.pillar_cell), dout.shape[0], B, H, W, C2, L.ptr(reg), L.ptr(ws), L.stream())
    else:
        L.call("gdmae_border_sums", L.ptr(y2), _bf(y2), L.ptr(s.tile_slot), L.ptr(s.ybg), L.ptr(rows), L.ptr(s.pillar_cell),
               rows.shape[0], B, H, W, C2, L.ptr(reg), L.ptr(ws), L.stream())
    return reg


# The region algebra: S = tap_region @ (cnt k0 + regY k1 + regR) with region 0 = all sites (sum Y = mean * R, sum rows = a * sum dh),
# the column sums of dZ over ALL sites, the background part of the weight gradient and the per-tap weight in the compute dtype.
# -> S (9, C2) f64, tot (Cin,) f64, dWk (9, C2, Cin), Wd (9, C2, Cin) in cdt;  W_k[o, i] = conv_w[o, i, ky, kx], k = 3 ky + kx.

def region_algebra_native(stats2, ab2, st2, k01, reg, tap_region, cnt, R, conv_w, bgz, cdt):
    """gdmae_decoder_region_algebra: one call (three launches) instead of ~20 small torch ops; fp32 contiguous conv_w, C2 % 8 == 0"""
    C2, Cin, dev = conv_w.shape[0], bgz.numel(), conv_w.device
    S = torch.empty(9, C2, dtype=torch.float64, device=dev)
    tot = torch.empty(Cin, dtype=torch.float64, device=dev)
    dWk = torch.empty(9, C2, Cin, dtype=torch.float32, device=dev)
    Wd = torch.empty(9, C2, Cin, dtype=cdt, device=dev)
    ws = torch.empty(L.load().gdmae_decoder_region_workspace_bytes(C2, Cin), dtype=torch.uint8, device=dev)
    L.call("gdmae_decoder_region_algebra", L.ptr(stats2), L.ptr(ab2), L.ptr(st2), L.ptr(k01), L.ptr(reg),
           L.ptr(tap_region), L.ptr(cnt), float(R), C2, Cin, L.ptr(conv_w), L.ptr(bgz), _bf(Wd), L.ptr(S), L.ptr(tot),
           L.ptr(dWk), L.ptr(Wd), L.ptr(ws), L.stream())
    return S, tot, dWk, Wd


def region_algebra_torch(stats2, ab2, st2, k01, reg, tap_region, cnt, R, conv_w, bgz, cdt):
    """The same as plain tensor algebra, for any conv_w and on any device.  dWk is fp32 (an fp64 conv_w keeps its gradient in fp64)."""
    C2, Cin = conv_w.shape[0], bgz.numel()
    k0, k1 = k01[:C2].double(), k01[C2:].double()
    regY = torch.cat([(stats2[:C2] * R)[None], reg[:8]])
    regR = torch.cat([(ab2[:C2].double() * st2[:C2])[None], reg[8:]])
    regD = cnt[:, None] * k0[None, :] + regY * k1[None, :] + regR
    S = tap_region @ regD                                     # (9, C2)
    Wk = conv_w.permute(2, 3, 0, 1).reshape(9, C2, Cin)              # W_k[o, i], k = (ky+1)*3 + (kx+1)
    tot = torch.einsum('ko,koi->i', S, Wk.double()).contiguous()      # column sums of dZ over ALL sites
    dWk = (S[:, :, None] * bgz.double()[None, None, :]).to(torch.promote_types(torch.float32, conv_w.dtype))   # background part of dW
    Wd = Wk.to(cdt)
    return S, tot, dWk, Wd


def _stage_dx_spconv(b, i, col):
    """dZ rows of the stage's active sites: implicit GEMM over the rulebook (9 gathered dY rows per site)"""
    n, w, C2 = b.Ps[i].shape[0], b.widths[i], b.y2.shape[1]
    nbr = b.tiles.nbr[i]
    assert nbr.shape[0] == n, (nbr.shape, n)
    dX = torch.empty(n, w, dtype=b.cdt, device=b.y2.device)
    L.call("gdmae_spconv", L.ptr(b.dYc), 0, L.ptr(nbr), b.packed.data_ptr() + i * 9 * w * C2 * 2, n, C2, w, L.ptr(dX), 8, L.stream())
    return dX


def _stage_grads_block(b, i, col):
    """input gradient over the rulebook; weight gradient on token blocks, added into b.dWk: the same sums (bit for bit) as
    _stage_grads_rulebook with the halo of a token's u x u sites read once per channel quarter; Zd stays in LDS"""
    dX = _stage_dx_spconv(b, i, col)
    P, ab, w, u = b.Ps[i], b.ab_l[i], b.widths[i], int(b.ups[i])
    n = P.shape[0]
    ws = torch.empty(int(L.load().gdmae_decoder_block_dw_workspace_bytes(n, u)), dtype=torch.uint8, device=P.device)
    L.call("gdmae_decoder_block_dw", L.ptr(P), L.ptr(ab), L.ptr(ab[w:]), L.ptr(b.bgz[col:col + w]), L.ptr(b.sites[i]), n, u, L.ptr(b.dYc),
           L.ptr(b.tile_slot), b.H, b.W, L.ptr(b.dWk), b.bgz.numel(), col, L.ptr(ws), L.stream())
    return dX, None


def _stage_grads_rulebook(b, i, col):
    """input gradient over the rulebook; weight gradient dWk[k][co][col + ci] += sum_t dY[site_t - k][co] * Zd[t][ci], nine taps in
    one grouped launch, added into b.dWk"""
    dX = _stage_dx_spconv(b, i, col)
    P, ab, w, C2 = b.Ps[i], b.ab_l[i], b.widths[i], b.y2.shape[1]
    n = P.shape[0]
    n_pad = int(L.load().gdmae_tap_dw_rows(n, w, C2))
    Zd = torch.empty(n_pad, w, dtype=b.cdt, device=P.device)
    L.call("gdmae_rows_affine_relu_sub", L.ptr(P), _bf(P), None, n, w, L.ptr(ab), L.ptr(ab[w:]), L.ptr(b.bgz[col:col + w]), L.ptr(Zd),
           _bf(Zd), w, 0, L.stream())
    ws = torch.empty(L.load().gdmae_tap_dw_workspace_bytes(n, w, C2), dtype=torch.uint8, device=P.device)
    L.call("gdmae_tap_dw", L.ptr(Zd), n, n_pad, w, L.ptr(b.dYc), L.ptr(b.tiles.nbr[i]), C2, L.ptr(b.dWk), b.bgz.numel(), col, L.ptr(ws),
           L.stream())
    return dX, None


def _stage_grads_taps(b, i, col):
    """the round-2 schedule: the 9 shifted dY rows of the active sites gathered, two library GEMMs; -> dX, dW rows (9*C2, w) fp32"""
    P, ab, w, C2, cdt = b.Ps[i], b.ab_l[i], b.widths[i], b.y2.shape[1], b.cdt
    n, dev = P.shape[0], P.device
    G = torch.empty(n, 9 * C2, dtype=cdt, device=dev)
    with timing.kernel("k_conv_grad_taps", 2.0 * n * 9 * C2 * G.element_size()):
        L.call("gdmae_conv3x3_grad_taps", L.ptr(b.y2), _bf(b.y2), L.ptr(b.tile_slot), L.ptr(b.ybg), L.ptr(b.k01), L.ptr(b.k01[C2:]),
               L.ptr(b.rows), L.ptr(b.cell2pillar), L.ptr(b.sites[i]), n, b.H, b.W, C2, L.ptr(G), L.stream())
    dX = ops.mm(G, b.Wd[:, :, col:col + w].reshape(9 * C2, w))      # dZ rows of this stage's active sites
    bg = b.bgz[col:col + w]
    if b.Z is not None:
        Zd = _gather_slice(b.Z, b.sites[i], col, w) - bg
    else:                       # the map was never built (tiles: 128-wide stages, bg in the compute dtype): redo BN + ReLU of the rows
        Zd = torch.empty(n, w, dtype=cdt, device=dev)
        L.call("gdmae_rows_affine_relu_sub", L.ptr(P), _bf(P), None, n, w, L.ptr(ab), L.ptr(ab[w:]), L.ptr(bg), L.ptr(Zd),
               _bf(Zd), w, 0, L.stream())
    return dX, ops.splitk_tn(G, Zd)


_STAGE_GRADS = {"block": _stage_grads_block, "rulebook": _stage_grads_rulebook, "taps": _stage_grads_taps}


def _stage_bn_backward(b, i, col, dX, R, direct):
    """BatchNorm2d (+ReLU) of source stage i at its active rows: dX -> (dP, dgamma, dbeta); b.tot carries the other sites' share"""
    P, ab, w = b.Ps[i], b.ab_l[i], b.widths[i]
    n = P.shape[0]
    ws = torch.empty(L.load().gdmae_rows_bwd_stats_workspace_bytes(w), dtype=torch.uint8, device=P.device)
    L.call("gdmae_rows_bwd_stats", L.ptr(P), _bf(P), None, n, w, L.ptr(ab), L.ptr(ab[w:]), L.ptr(dX), _bf(dX), w, 0,
           None, L.ptr(ws), L.stream())
    dgamma, dbeta, c01 = gbn.bwd_coeffs((ws, L.load().gdmae_rows_bwd_stats_rows(n)), 3, b.stats_l[i], ab, b.gammas[i], R,
                                        b.tot[col:col + w], direct)
    dP = torch.empty_like(P)
    L.call("gdmae_rows_bwd", L.ptr(P), _bf(P), None, n, w, L.ptr(ab), L.ptr(ab[w:]), L.ptr(c01), L.ptr(c01[w:]), L.ptr(dX),
           _bf(dX), w, 0, L.ptr(dP), _bf(dP), L.stream())
    return dP, dgamma, dbeta


class DecoderHead(torch.autograd.Function):
    """The whole generative-decoder head on the token rows (reference spt_backbone_mae.py:30-52,125-135):
    ConvTranspose2d(k=s) outputs P_i of the active sites -> BatchNorm2d(train)+ReLU of the (implicit) dense maps ->
    channel concat Z (R, sum C_i) channels-last -> 3x3 conv_out (tile convolution, or a dense convolution of the materialised map) ->
    BatchNorm2d(train)+ReLU evaluated only at the pillar sites.

    forward(geom, pre_conv_hook, conv_w, gamma2, beta2, pillar_cell, cell2pillar, bn_mods, sites_0, P_0, gamma_0, beta_0, sites_1, ...)
      geom: DecoderGeom.  pre_conv_hook: None or a callable invoked once right before the tile convolution is launched; it is not
      kept.  Every non-active site of map i is zero before its BatchNorm, so the batch statistics over all R sites are column sums
      of P_i and every other site holds the constant background relu(beta - gamma*mean*rstd).
      Returns (out (M, C2) fp32, Y [conv output, tile-compact or (R, C2)], mean2, var2, mean_0, var_0, ..., ybg [the 9 border-class
      constants of a tile-compact Y, else None]); all but out non-differentiable, Y and ybg for expand_dense.
      The forward also decides the backward's schedule per source stage (_backward_schedule) and carries it on ctx.
    backward: hand-derived.  The conv output gradient is dY = k0 + k1*Y + rows-at-pillar-sites (BatchNorm2d chain rule), which is
      dense - but the input gradient is only needed at the active sites of each stage (everything else is the shared background whose
      gradient is a border-corrected closed form), and the weight gradient splits into background x region-sums plus active-site
      rows: _bn2_backward, _region_sums + the region algebra, then per stage _STAGE_GRADS[schedule] and _stage_bn_backward.  dY on all
      sites and dZ are never materialised."""

    @staticmethod
    def forward(ctx, geom, pre_conv_hook, conv_w, gamma2, beta2, pillar_cell, cell2pillar, bn_mods, *args):
        R = geom.B * geom.H * geom.W
        k = len(args) // 4
        sites, Ps, gammas, betas = args[0::4], args[1::4], args[2::4], args[3::4]
        widths = [int(P.shape[1]) for P in Ps]
        bns = list(bn_mods) if bn_mods is not None else [None] * (k + 1)
        ab_l, stats_l, mv_out = [], [], []
        for i in range(k):
            stats, ab, mv = gbn.fold(Ps[i].contiguous(), R, gammas[i], betas[i], geom.eps1, bns[i])
            ab_l.append(ab), stats_l.append(stats)
            mv_out += [mv[:widths[i]], mv[widths[i]:]]
        use_tiles = (geom.tile_conv is not None and geom.cdt == torch.bfloat16 and all(w == 128 for w in widths) and conv_w.shape[0] == 128
                     and conv_w.dtype == torch.float32 and conv_w.is_contiguous() and all(P.dtype == torch.bfloat16 for P in Ps))
        if use_tiles:
            f = _forward_tiles(geom, pre_conv_hook, conv_w, gamma2, beta2, pillar_cell, Ps, widths, ab_l, bns[k])
        else:
            f = _forward_dense_map(geom, conv_w, gamma2, beta2, pillar_cell, sites, Ps, widths, ab_l, bns[k])
        M, C2 = f.yrows.shape
        out = f.out
        if out is None:
            out = torch.empty(M, C2, dtype=torch.float32, device=f.yrows.device)
            L.call("gdmae_rows_affine_relu_scatter", L.ptr(f.yrows), _bf(f.yrows), None, M, C2, L.ptr(f.ab2), L.ptr(f.ab2[C2:]), L.ptr(out), 0,
                   C2, 0, L.stream())
        _save(ctx, sites=sites, Ps=Ps, ab_l=ab_l, stats_l=stats_l, gammas=[g.detach() for g in gammas], Z=f.Z, y2=f.y2, bgz=f.bgz,
              yrows=f.yrows, ab2=f.ab2, stats2=f.stats2, pillar_cell=pillar_cell, cell2pillar=cell2pillar, gamma2=gamma2.detach(),
              conv_w=conv_w.detach(), tile_slot=f.tile_slot, ybg=f.ybg)
        ctx.geom, ctx.widths = geom, widths
        ctx.native_region, ctx.stage_bwd = _backward_schedule(geom, conv_w, sites, Ps, widths, f)
        # the pillar rows of dY stay unwritten when no stage reads them as an array ("taps" does, through gdmae_conv3x3_grad_taps)
        ctx.dy_rows = DY_ROWS and C2 % 8 == 0 and all(sb != "taps" for sb in ctx.stage_bwd)
        ctx.direct = [gbn.direct_pair(g, be) for g, be in zip(gammas, betas)] + [gbn.direct_pair(gamma2, beta2)]
        ctx.direct_w = ops.direct_grad(conv_w)
        ctx.conv_param = conv_w        # the parameter object itself: the packed images of the backward are registered on its identity
        mean2, var2 = f.mv2[:C2], f.mv2[C2:]
        ctx.mark_non_differentiable(f.y2, mean2, var2, *mv_out, *([] if f.ybg is None else [f.ybg]))
        ctx.set_materialize_grads(False)      # no zero tensors for the unused gradients of those outputs
        return (out, f.y2, mean2, var2, *mv_out, f.ybg)

    @staticmethod
    def backward(ctx, dout, *_):
        geom, widths, stage_bwd = ctx.geom, ctx.widths, ctx.stage_bwd
        B, H, W = geom.B, geom.H, geom.W
        R, k = B * H * W, len(widths)
        b = _saved(ctx)                      # the saved tensors by name; the steps below add what they share
        b.H, b.W, b.cdt, b.widths = H, W, geom.cdt, widths
        dout, st2, b.k01, dgamma2, dbeta2 = _bn2_backward(b, dout, R, ctx.direct[k])
        b.rows = None if ctx.dy_rows else _pillar_rows(b, dout)
        reg = _region_sums(b, b.rows, dout, B, H, W)
        tap_region, cnt = _region_consts(reg.device, B, H, W)
        algebra = region_algebra_native if ctx.native_region else region_algebra_torch
        S, b.tot, b.dWk, b.Wd = algebra(b.stats2, b.ab2, st2, b.k01, reg, tap_region, cnt, R, b.conv_w, b.bgz, geom.cdt)
        if stage_bwd[0] != "taps":
            # the one test left to the backward: a weight that no flat optimizer owns is packed on the spot, and in the forward that
            # launch would come earlier
            b.packed = packing.decoder_conv_packed(ctx.conv_param, widths, ctx.direct_w is not None)
            if b.packed is None:
                stage_bwd = ["taps"] * k
                if b.rows is None:
                    b.rows = _pillar_rows(b, dout)
            else:
                # the output gradient ONCE in Y's tile-compact layout, rulebooks of the (active site, tap) rows
                b.tiles, b.ups = geom.tile_conv.tiles, geom.tile_conv.ups
                if b.tiles.nbr is None:
                    b.tiles.nbr = gplan.decoder_site_rulebooks(b.tiles, b.sites, b.ups)
                C2 = b.y2.shape[1]
                b.dYc = torch.empty_like(b.y2)
                if b.rows is None:
                    L.call("gdmae_decoder_dy_rows", L.ptr(b.y2), L.ptr(b.tiles.tile_list), b.tiles.n_act, L.ptr(b.k01), L.ptr(b.k01[C2:]),
                           L.ptr(dout), L.ptr(b.ab2), L.ptr(b.ab2[C2:]), L.ptr(b.cell2pillar), H, W, C2, L.ptr(b.dYc), L.stream())
                else:
                    L.call("gdmae_decoder_dy", L.ptr(b.y2), L.ptr(b.tiles.tile_list), b.tiles.n_act, L.ptr(b.k01), L.ptr(b.k01[C2:]),
                           L.ptr(b.rows), L.ptr(b.cell2pillar), H, W, C2, L.ptr(b.dYc), L.stream())
        grads = [None] * 8
        dW_rows = []
        col = 0
        for i, w in enumerate(widths):
            dX, dW = _STAGE_GRADS[stage_bwd[i]](b, i, col)
            if dW is not None:
                dW_rows.append(dW)
            grads += [None, *_stage_bn_backward(b, i, col, dX, R, ctx.direct[i])]
            col += w
        dWk = b.dWk
        if dW_rows:
            dWk = dWk + torch.cat(dW_rows, dim=1).view(dWk.shape)
        dW = dWk.permute(1, 2, 0).reshape(b.conv_w.shape[0], b.conv_w.shape[1], 3, 3)
        if ctx.direct_w is not None:
            ctx.direct_w.add_(dW)
        else:
            grads[2] = dW.to(b.conv_w.dtype)
        grads[3], grads[4] = dgamma2, dbeta2
        return tuple(grads)


class DeconvRowsFn(torch.autograd.Function):
    """P (n * s*s, cout) = rows of ConvTranspose2d(k = s, stride s, no bias) at the active tokens (csrc/rows_gemm.hip): x (n, cin)
    bf16 token rows, weight (cin, cout, s, s) fp32 owned by a flat optimizer (its gradient is accumulated there directly).  Replaces
    the weight permute + cast and the three library GEMMs (forward, input gradient, split-K weight gradient) of a deblock."""

    @staticmethod
    def forward(ctx, x, weight, direct):
        cin, cout, s, _ = weight.shape
        n = x.shape[0]
        dev = x.device
        x = x.contiguous()
        nb = L.load().gdmae_deconv_rows_packed_bytes(cin, cout, s)
        pf = torch.empty(nb, dtype=torch.uint8, device=dev)
        pb = torch.empty(nb, dtype=torch.uint8, device=dev)
        L.call("gdmae_deconv_rows_pack", L.ptr(weight), cin, cout, s, L.ptr(pf), L.ptr(pb), L.stream())
        P = torch.empty(n * s * s, cout, dtype=torch.bfloat16, device=dev)
        L.call("gdmae_deconv_rows_fwd", L.ptr(x), n, cin, cout, s, L.ptr(pf), L.ptr(P), L.stream())
        ctx.save_for_backward(x, pb)
        ctx.meta = (cin, cout, s, direct)
        return P

    @staticmethod
    def backward(ctx, dP):
        x, pb = ctx.saved_tensors
        cin, cout, s, direct = ctx.meta
        n = x.shape[0]
        dP = dP.contiguous()
        if dP.dtype != torch.bfloat16:
            dP = dP.to(torch.bfloat16)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(n, cin, dtype=torch.bfloat16, device=x.device)
            L.call("gdmae_deconv_rows_bwd_input", L.ptr(dP), n, cin, cout, s, L.ptr(pb), L.ptr(dx), L.stream())
        ws = torch.empty(L.load().gdmae_deconv_rows_dw_workspace_bytes(n, cin, cout, s), dtype=torch.uint8, device=x.device)
        L.call("gdmae_deconv_rows_bwd_weight", L.ptr(x), L.ptr(dP), n, cin, cout, s, L.ptr(direct), L.ptr(ws), L.stream())
        return dx, None, None


DECONV_ROWS = os.environ.get("GDMAE_DECONV_ROWS", "1") != "0"     # False: weight permute + library GEMMs (A/B reference)


def deconv_rows(x, deconv):
    """Token rows of a ConvTranspose2d(k = s, stride s, no bias) block: -> (n * s*s, cout), row (token, dy * s + dx)."""
    w = deconv.weight
    s = int(deconv.stride[0])
    cin, cout = w.shape[0], w.shape[1]
    direct = ops.direct_grad(w)
    if (DECONV_ROWS and x.is_cuda and torch.is_autocast_enabled() and x.dtype == torch.bfloat16 and direct is not None and w.dtype == torch.float32
            and w.is_contiguous() and cin in (128, 256) and cout == 128 and s in (1, 2, 4) and x.shape[0] > 0):
        return DeconvRowsFn.apply(x, w, direct)
    wmat = w.permute(0, 2, 3, 1).reshape(cin, s * s * cout)                  # columns ordered (dy, dx, c)
    return ops.linear(x, wmat.t()).view(-1, cout)


class PredHeadFn(torch.autograd.Function):
    """x W^T + b (fp32-accurate forward, bf16-operand backward) for the prediction head nn.Linear(128 -> 48) on the fp32 decoder rows of all pillars (csrc/rows_gemm.hip
    k_pred_*; reference spt_backbone_mae.py:52,74): no cast passes, no unaligned library GEMMs."""

    @staticmethod
    def forward(ctx, x, weight, bias, direct):
        n, n_out = x.shape[0], weight.shape[0]
        x = x.contiguous()
        packed = torch.empty(L.load().gdmae_pred_head_packed_bytes(), dtype=torch.uint8, device=x.device)
        L.call("gdmae_pred_head_pack", L.ptr(weight), None if bias is None else L.ptr(bias), weight.shape[1], n_out, L.ptr(packed), L.stream())
        xb = torch.empty(n, x.shape[1], dtype=torch.bfloat16, device=x.device)      # the rounded operand rows: operand of the weight gradient
        # fp32-accurate result (three-term split-bf16 product, fp32 bias): the Chamfer kernel squares these offsets, and a bf16-rounded
        # output biases the loss by 1 - 4e-4 relative; an fp32 output also receives the loss's fp32 gradient without a cast in between
        y = torch.empty(n, n_out, dtype=torch.float32, device=x.device)
        L.call("gdmae_pred_head_fwd", L.ptr(x), n, n_out, L.ptr(packed), None, L.ptr(xb), L.ptr(y), L.stream())
        ctx.save_for_backward(xb, packed)
        ctx.meta = (n_out, direct, weight.shape, None if bias is None else bias.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, packed = ctx.saved_tensors
        n_out, direct, wshape, bshape = ctx.meta
        n = x.shape[0]
        dy = dy.contiguous()
        if dy.dtype not in (torch.bfloat16, torch.float32):
            dy = dy.float()
        f32 = dy.dtype == torch.float32                   # rounded inside the input-gradient launch (no cast pass)
        dyb = torch.empty(dy.shape, dtype=torch.bfloat16, device=x.device) if f32 else None
        dx = torch.empty(x.shape, dtype=torch.float32, device=x.device) if ctx.needs_input_grad[0] else None
        if direct is not None:
            dW, db = direct
            ret = (None, None)
        else:
            dW = torch.zeros(wshape, dtype=torch.float32, device=x.device)
            db = None if bshape is None else torch.zeros(bshape, dtype=torch.float32, device=x.device)
            ret = (dW, db)
        ws = torch.empty(L.load().gdmae_pred_head_bwd_workspace_bytes(n), dtype=torch.uint8, device=x.device)
        scale = ops.LAZY_SCALE.pop(dy.data_ptr(), None) if f32 else None         # (upstream gradient, 1 / sum of weights) of the Chamfer mean
        if scale is None and ops.LAZY_SCALE:
            raise RuntimeError("an unscaled Chamfer gradient was handed over (ops.LAZY_SCALE) but did not arrive here as the same tensor")
        L.call("gdmae_pred_head_bwd", L.ptr(dy), int(f32), None if dyb is None else L.ptr(dyb), None if scale is None else L.ptr(scale[0]),
               None if scale is None else L.ptr(scale[1]), L.ptr(x), n, n_out, L.ptr(packed),
               None if dx is None else L.ptr(dx), L.ptr(dW), None if db is None else L.ptr(db), L.ptr(ws), L.stream())
        return (dx, *ret, None)


def pred_head(x, linear):
    """``linear`` (nn.Linear 128 -> n_out) applied to fp32 rows under autocast: -> (n, n_out) fp32 values accurate to fp32 on the fused path
    (bf16 from the library path)."""
    w, b = linear.weight, linear.bias
    if (DECONV_ROWS and x.is_cuda and torch.is_autocast_enabled() and x.dtype == torch.float32 and w.dtype == torch.float32 and w.is_contiguous()
            and w.shape[1] == 128 and 8 <= w.shape[0] <= 64 and w.shape[0] % 8 == 0 and x.shape[0] > 0):
        dw, db = ops.direct_grad(w), (ops.direct_grad(b) if b is not None else None)
        direct = (dw, db) if (dw is not None and (b is None or db is not None)) else None
        y = PredHeadFn.apply(x, w, b, direct)
        y._gd_pred_head = True                 # its backward applies the scalars of a mean on load (ops.ChamferLoss lazy_scale)
        return y
    return ops.linear(x, w, b)


def upsampled_sites(stage_plan, s: int, Y: int, X: int) -> torch.Tensor:
    """(n_tok * s*s,) int32 full-resolution cell of every (token, dy, dx) of a stride-s stage (prepared with the geometry
    plan when the stage's stride matches)."""
    if s == 1:
        return stage_plan.tok_cell
    pre = getattr(stage_plan, "_up_sites", None)
    if pre is not None and pre[0] == s and stage_plan.Y * s == Y and stage_plan.X * s == X:
        return pre[1]
    return gplan.upsample_cells(stage_plan.tok_cell, stage_plan.Y, stage_plan.X, s).reshape(-1).contiguous()


def expand_dense(y2, ybg, tiles, a2, b2, B, Y, X):
    """relu(a2 * conv output + b2) on all sites as the reference's dense (B, C2, Y, X) spatial_features.  ``y2``, ``ybg``: the conv
    output and the border-class constants that ONE DecoderHead call returned (tile-compact on ``tiles``, or dense and None)."""
    R = B * Y * X
    C2 = y2.shape[1]
    # a tile-compact Y is the one that came with border-class constants.  Its row count says nothing: with every tile active on a map
    # of whole tiles it has R rows too, in tile order
    compact = ybg is not None
    assert y2.shape[0] == (max(tiles.n_act, 1) * 64 if compact else R), (y2.shape, R, compact)
    if compact and y2.dtype == torch.bfloat16 and C2 % 8 == 0:
        # tile-compact conv output -> the reference's dense map in one pass (expand + BatchNorm affine + ReLU)
        dmap = torch.empty(R, C2, dtype=torch.float32, device=y2.device)
        L.call("gdmae_tiles_to_dense_affine_relu", L.ptr(y2), L.ptr(tiles.tile_slot), L.ptr(ybg), B, Y, X, C2,
               L.ptr(a2), L.ptr(b2), L.ptr(dmap), L.stream())
        return dmap.view(B, Y, X, -1).permute(0, 3, 1, 2)
    if compact:
        yd = torch.empty(R, C2, dtype=y2.dtype, device=y2.device)
        L.call("gdmae_tiles_to_dense", L.ptr(y2), L.ptr(tiles.tile_slot), L.ptr(ybg), B, Y, X, C2, y2.element_size(),
               L.ptr(yd), L.stream())
        y2 = yd
    return torch.relu(y2.float() * a2 + b2).view(B, Y, X, -1).permute(0, 3, 1, 2)


def sparse_decoder(model_cfg, deblocks, conv_out, hidden, pillar_cell, cell2pillar, B, Y, X, want_dense=False, conv_impl='tiles', pre_conv_hook=None):
    """hidden: list of SparseConvTensor per stage.  Returns (features at the pillar sites (M, C) fp32,
    dense spatial_features (B, C, Y, X) or None)."""
    args, bns = [], []
    cdt = torch.bfloat16 if torch.is_autocast_enabled() else torch.float32
    src_idx = [int(src[-1]) - 1 for src in model_cfg.FEATURES_SOURCE]
    tile_conv = None
    if cdt == torch.bfloat16 and conv_impl == 'tiles':
        ep = hidden[0]._plan
        tile_conv = TileConv(gplan.decoder_tiles(ep, src_idx, Y, X), [hidden[i].stage_plan.map for i in src_idx],
                             [Y // hidden[i].stage_plan.Y for i in src_idx], CT_SKIP)
    for i, src in enumerate(model_cfg.FEATURES_SOURCE):
        h = hidden[int(src[-1]) - 1]
        sp = h.stage_plan
        deconv, bn = deblocks[i][0], deblocks[i][1]
        s = int(deconv.stride[0])
        assert deconv.kernel_size == (s, s) and sp.Y * s == Y and sp.X * s == X and deconv.bias is None
        P = deconv_rows(h.features, deconv)                                      # (n_tok * s*s, cout)
        args += [upsampled_sites(sp, s, Y, X), P, bn.weight, bn.bias]
        bns.append(bn)
    conv, bn2 = conv_out[0], conv_out[1]
    outs = DecoderHead.apply(DecoderGeom(B, Y, X, bns[0].eps, bn2.eps, cdt, tile_conv), pre_conv_hook, conv.weight, bn2.weight, bn2.bias,
                             pillar_cell, cell2pillar, tuple(bns) + (bn2,), *args)
    out, y2, mean2, var2 = outs[:4]
    dense = None
    if want_dense:
        with torch.no_grad():
            a2 = (bn2.weight * torch.rsqrt(var2 + bn2.eps)).float().contiguous()
            b2 = (bn2.bias - a2 * mean2).float().contiguous()
            dense = expand_dense(y2, outs[-1], None if tile_conv is None else tile_conv.tiles, a2, b2, B, Y, X)
    return out, dense
