"""Decoder conv_out backward on token blocks (csrc/decoder_blocks.hip) through the C ABI, on crafted geometry built with the plan's own
helpers (decoder_tiles -> tile set + rulebook, upsample_cells -> the stage's sites).

gdmae_decoder_block_dw replaces gdmae_rows_affine_relu_sub + gdmae_tap_dw for source stages with an upsampling stride u = 2 / 4:

    dWk[k][co][ci] = sum_t dY[nbr[t, k]][co] * Zd[t][ci]        Zd = bf16(bf16(relu(a P + b)) - bg)

Reference: the fp64 product of the SAME bf16 operands (the Zd rows gdmae_rows_affine_relu_sub writes, the dY rows through the rulebook).
Error = |got - want|_F / |want|_F per tap.  The bound is 2 x the worst error of the rulebook path (gdmae_rows_affine_relu_sub +
gdmae_tap_dw) over all cases and taps, measured with this same test body (PARENT_WORST; the factor 2 covers a different but still
fixed summation order).  Two consecutive runs must give the same bits.  The kernel keeps the rulebook path's slices, chunk order and
reduction, so its result is also required to EQUAL that path's, bit for bit, in every case.

Measured (MI355X): see profiles/r10_decoder_conv_backward.txt, section 5."""
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

# worst relative Frobenius error per tap of the rulebook path (rows_affine_relu_sub + tap_dw) over CASES, against the fp64 product
PARENT_WORST = 1.880e-7

C = 128


def _cells(kind, B, Ys, Xs, u, gen):
    """coarse cells ((b Ys + y) Xs + x) of the tokens, in token order"""
    if kind == "one":
        return [(0 * Ys + Ys // 2) * Xs + 1]
    if kind == "corners":                       # halo rows outside the map on two sides, in every batch item
        return [(b * Ys + y) * Xs + x for b in range(B) for y in (0, Ys - 1) for x in (0, Xs - 1)]
    if kind == "adjacent":                      # two tokens on either side of the 8 x 8 tile boundary at fine x = 8 (and y = 8)
        cx = 8 // u
        return [(0 * Ys + 1) * Xs + cx - 1, (0 * Ys + 1) * Xs + cx, ((B - 1) * Ys + cx - 1) * Xs + 0, ((B - 1) * Ys + cx) * Xs + 0]
    n = int(kind)
    return sorted(torch.randperm(B * Ys * Xs, generator=gen)[:n].tolist())


# (u, B, H = W, tokens): every combination the kernel treats differently at the smallest sizes - 3 x 3 tiles with a partial last
# tile (20) and whole tiles (24), one token, corners, neighbours across a tile boundary, token counts that are no multiple of the
# chunk (4 tokens at u = 4, 16 at u = 2) - and one map per stride with several chunks per slice (9 at u = 4, 6 at u = 2)
CASES = [(4, 1, 20, "one"), (2, 1, 24, "one"), (4, 1, 20, "corners"), (2, 2, 20, "corners"), (4, 2, 24, "corners"), (2, 1, 24, "corners"),
         (4, 1, 24, "adjacent"), (2, 2, 20, "adjacent"), (4, 1, 20, "13"), (2, 2, 24, "13"), (4, 2, 20, "37"), (2, 1, 20, "37"),
         (4, 2, 24, "37"), (2, 2, 24, "37"), (4, 1, 24, "36"), (2, 2, 24, "288"), (4, 2, 192, "2300"), (2, 2, 96, "2650")]


def _id(c):
    return "u%d_B%d_H%d_%s" % c


@functools.lru_cache(maxsize=None)
def _case(u, B, H, kind):
    """geometry + operands of one case on the GPU, the fp64 reference and the rulebook path's result (computed once, never modified)"""
    from gdmae_hip import lib as L
    from gdmae_hip import plan as gplan
    d = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1000 * u + 100 * B + H + len(kind))
    W = H
    Ys, Xs = H // u, W // u
    tok = torch.tensor(_cells(kind, B, Ys, Xs, u, gen), dtype=torch.int32)
    ntok = tok.numel()
    cmap = torch.full((B * Ys * Xs,), -1, dtype=torch.int32)
    cmap[tok.long()] = torch.arange(ntok, dtype=torch.int32)
    sp = types.SimpleNamespace(map=cmap.to(d), B=B, Y=Ys, X=Xs, tok_cell=tok.to(d), n_tok=ntok, _up_sites=None)
    ep = types.SimpleNamespace(dec_tiles=None, stages=[sp])
    dt = gplan.decoder_tiles(ep, (0,), H, W)
    sites = gplan.upsample_cells(sp.tok_cell, Ys, Xs, u).reshape(-1).contiguous()
    nbr = dt.nbr[0].contiguous()
    n = sites.numel()
    assert nbr.shape == (n, 9) and n == ntok * u * u
    P = torch.randn(n, C, generator=gen).bfloat16().to(d)
    a = (torch.rand(C, generator=gen) + 0.5).to(d)
    b = (torch.randn(C, generator=gen) * 0.5).to(d)
    bg = torch.relu(b).bfloat16()
    dY = torch.randn(dt.n_act * 64, C, generator=gen).bfloat16().to(d)
    lib = L.load()
    # the rulebook path: Zd rows, then the nine gathered products
    n_pad = int(lib.gdmae_tap_dw_rows(n, C, C))
    Zd = torch.zeros(n_pad, C, dtype=torch.bfloat16, device=d)
    L.call("gdmae_rows_affine_relu_sub", L.ptr(P), 1, None, n, C, L.ptr(a), L.ptr(b), L.ptr(bg), L.ptr(Zd), 1, C, 0, L.stream())
    parent = torch.zeros(9, C, C, device=d)
    ws = torch.empty(lib.gdmae_tap_dw_workspace_bytes(n, C, C), dtype=torch.uint8, device=d)
    L.call("gdmae_tap_dw", L.ptr(Zd), n, n_pad, C, L.ptr(dY), L.ptr(nbr), C, L.ptr(parent), C, 0, L.ptr(ws), L.stream())
    # fp64 product of the same bf16 operands
    z = Zd[:n].double()
    want = torch.empty(9, C, C, dtype=torch.float64, device=d)
    for k in range(9):
        j = nbr[:, k].long()
        g = dY[j.clamp(min=0)].double() * (j >= 0).double()[:, None]
        want[k] = g.t() @ z
    torch.cuda.synchronize()
    return types.SimpleNamespace(u=u, B=B, H=H, W=W, n=n, dt=dt, sites=sites, nbr=nbr, P=P, a=a, b=b, bg=bg, dY=dY, want=want, parent=parent)


def _block_dw(c, ld_out=C, m_off=0, fill=0.0):
    from gdmae_hip import lib as L
    d = c.P.device
    out = torch.full((9, C, ld_out), fill, device=d)
    ws = torch.empty(L.load().gdmae_decoder_block_dw_workspace_bytes(c.n, c.u), dtype=torch.uint8, device=d)
    L.call("gdmae_decoder_block_dw", L.ptr(c.P), L.ptr(c.a), L.ptr(c.b), L.ptr(c.bg), L.ptr(c.sites), c.n, c.u, L.ptr(c.dY),
           L.ptr(c.dt.tile_slot), c.H, c.W, L.ptr(out), ld_out, m_off, L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    return out


def _tap_errors(got, want):
    return [float((got[k].double() - want[k]).norm()) / max(float(want[k].norm()), 1e-30) for k in range(9)]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_block_weight_gradient_against_fp64(case):
    c = _case(*case)
    got = _block_dw(c)
    e_new, e_par = _tap_errors(got, c.want), _tap_errors(c.parent, c.want)
    print("[decoder block dw %s] n %d  worst tap error: rulebook path %.3e  block kernel %.3e" % (_id(case), c.n, max(e_par), max(e_new)))
    assert max(e_new) <= 2 * PARENT_WORST, (e_new, PARENT_WORST)
    assert torch.equal(got, c.parent), "not the rulebook path's bits (same slices, same chunk order, same reduction)"
    assert torch.equal(got, _block_dw(c)), "two runs on the same inputs differ"


def test_block_weight_gradient_adds_into_its_columns_only():
    """out[k][co][m_off + ci] += ...: a (9, 128, 384) gradient with the stage at column 128, prefilled"""
    c = _case(4, 2, 24, "37")
    got = _block_dw(c, ld_out=3 * C, m_off=C, fill=0.5)
    assert bool((got[:, :, :C] == 0.5).all()) and bool((got[:, :, 2 * C:] == 0.5).all())
    assert torch.equal(got[:, :, C:2 * C], 0.5 + _block_dw(c))


def test_no_rows_is_no_launch():
    from gdmae_hip import lib as L
    for u in (2, 4):
        assert L.load().gdmae_decoder_block_dw(None, None, None, None, None, 0, u, None, None, 24, 24, None, C, 0, None, None) == 0


def _head_geometry():
    """B = 2, 24 x 24, three source stages u = 1 / 2 / 4 with 150 / 37 / 13 tokens; pillars = the tokens of the first stage"""
    d = torch.device("cuda:0")
    B, H, W = 2, 24, 24
    gen = torch.Generator().manual_seed(5)
    stages = []
    for u, ntok in ((1, 150), (2, 37), (4, 13)):
        Ys, Xs = H // u, W // u
        tok = torch.randperm(B * Ys * Xs, generator=gen)[:ntok].sort().values.int()
        cmap = torch.full((B * Ys * Xs,), -1, dtype=torch.int32)
        cmap[tok.long()] = torch.arange(ntok, dtype=torch.int32)
        stages.append(types.SimpleNamespace(map=cmap.to(d), B=B, Y=Ys, X=Xs, tok_cell=tok.to(d), n_tok=ntok, _up_sites=None))
    return (B, H, W, stages, stages[0].tok_cell, stages[0].map)


def _decoder_head(geo, seed=11):
    """one DecoderHead forward on the crafted stages: -> (outputs, leaves [conv_w, g2, b2, (P, g, b) per stage], tile set, an upstream
    gradient for outputs[0])"""
    from gdmae_hip import decoder as gdec
    from gdmae_hip import plan as gplan
    d = torch.device("cuda:0")
    B, H, W, stages, pillar_cell, cell2pillar = geo
    gen = torch.Generator().manual_seed(seed)
    ep = types.SimpleNamespace(dec_tiles=None, stages=stages)
    dt = gplan.decoder_tiles(ep, (0, 1, 2), H, W)
    ups = [H // sp.Y for sp in stages]
    conv_w = (torch.randn(C, 3 * C, 3, 3, generator=gen) * 0.05).to(d).requires_grad_()
    g2, b2 = (torch.rand(C, generator=gen) + 0.5).to(d).requires_grad_(), (torch.randn(C, generator=gen) * 0.3).to(d).requires_grad_()
    args, leaves = [], [conv_w, g2, b2]
    for sp, u in zip(stages, ups):
        sites = sp.tok_cell if u == 1 else gplan.upsample_cells(sp.tok_cell, sp.Y, sp.X, u).reshape(-1).contiguous()
        P = torch.randn(sites.numel(), C, generator=gen).bfloat16().to(d).requires_grad_()
        g, b = (torch.rand(C, generator=gen) + 0.5).to(d).requires_grad_(), (torch.randn(C, generator=gen) * 0.3).to(d).requires_grad_()
        args += [sites, P, g, b]
        leaves += [P, g, b]
    up = torch.randn(pillar_cell.numel(), C, generator=gen).to(d)
    geom = gdec.DecoderGeom(B, H, W, 1e-3, 1e-3, torch.bfloat16, gdec.TileConv(dt, [sp.map for sp in stages], ups))
    outs = gdec.DecoderHead.apply(geom, None, conv_w, g2, b2, pillar_cell, cell2pillar, None, *args)
    return outs, leaves, dt, up


def _decoder_head_grads(mode, geo, mode_after_forward=None):
    """one DecoderHead forward + backward on crafted stages (u = 1, 2, 4) with gdmae_hip.decoder.BLOCK_BWD = mode (and, if given,
    = mode_after_forward between the forward and the backward)"""
    from gdmae_hip import decoder as gdec
    old = gdec.BLOCK_BWD
    gdec.BLOCK_BWD = mode
    try:
        outs, leaves, _, up = _decoder_head(geo)
        if mode_after_forward is not None:
            gdec.BLOCK_BWD = mode_after_forward
        (outs[0] * up).sum().backward()
    finally:
        gdec.BLOCK_BWD = old
    torch.cuda.synchronize()
    return [t.grad.clone() for t in leaves]


def test_decoder_head_backward_same_gradients_on_both_paths():
    """DecoderHead.backward with the block kernels (default) and with the rulebook path for every stage (GDMAE_DEC_BLOCK=0): dP, dgamma,
    dbeta of every stage and of the output BatchNorm bit-equal; the conv weight gradient bit-equal in the u = 1 stage's columns and
    within the bound of the C-ABI test per tap in the others."""
    geo = _head_geometry()
    new, ref = _decoder_head_grads("1", geo), _decoder_head_grads("0", geo)
    assert torch.equal(new[1], ref[1]) and torch.equal(new[2], ref[2]), "dgamma2 / dbeta2"
    for i in range(3):
        for j, what in enumerate(("dP", "dgamma", "dbeta")):
            assert torch.equal(new[3 + 3 * i + j], ref[3 + 3 * i + j]), (what, i)
    dw_new, dw_ref = new[0], ref[0]                           # (128, 384, 3, 3)
    assert torch.equal(dw_new[:, :C], dw_ref[:, :C]), "conv weight gradient, u = 1 columns"
    worst = 0.0
    for i in (1, 2):
        for k in range(9):
            a, b = dw_new[:, i * C:(i + 1) * C, k // 3, k % 3].double(), dw_ref[:, i * C:(i + 1) * C, k // 3, k % 3].double()
            worst = max(worst, float((a - b).norm()) / max(float(b.norm()), 1e-30))
    print("[decoder head backward] conv weight gradient, block vs rulebook path, worst tap: %.3e" % worst)
    assert worst <= 2 * PARENT_WORST, worst
    assert torch.equal(dw_new, dw_ref), "conv weight gradient: the two paths add the same products in the same order"


def test_backward_schedule_is_the_one_the_forward_chose():
    """gdmae_hip.decoder.BLOCK_BWD set to "0" after the forward and before backward(): the gradients are those of a run that never
    touched it (bit for bit) - the forward decided the schedule and the backward consults no switch."""
    geo = _head_geometry()
    ref, got = _decoder_head_grads("1", geo), _decoder_head_grads("1", geo, mode_after_forward="0")
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(a, b), i


def test_border_constants_belong_to_their_call():
    """The dense expansion of head A's outputs is the same (bit for bit) before and after another head B, with another conv weight and
    other BatchNorm parameters, has run: ybg travels with the call's outputs, not with the process."""
    from gdmae_hip import decoder as gdec
    geo = _head_geometry()
    B, H, W = geo[:3]
    a2 = (torch.rand(C, generator=torch.Generator().manual_seed(3)) + 0.5).cuda()
    b2 = torch.randn(C, generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad():
        outs_a, _, dt, _ = _decoder_head(geo, seed=11)
        first = gdec.expand_dense(outs_a[1], outs_a[-1], dt, a2, b2, B, H, W).clone()
        outs_b = _decoder_head(geo, seed=23)[0]
        assert not torch.equal(outs_b[-1], outs_a[-1]), "head B must have other border constants for this test to mean anything"
        again = gdec.expand_dense(outs_a[1], outs_a[-1], dt, a2, b2, B, H, W)
    torch.cuda.synchronize()
    assert first.shape == (B, C, H, W) and torch.equal(first, again)
