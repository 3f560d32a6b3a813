"""The decoder head's region algebra (gdmae_hip.decoder.region_algebra_torch / region_algebra_native): the closed form that turns the
9 border-region sums of the conv output gradient dY = k0 + k1 Y + rows into the per-tap sums S, the column sums ``tot`` of the
conv input gradient over all sites and the background part dWk of the weight gradient.

CPU: on a map that holds the constant ``bgz`` at EVERY site the background part is the whole gradient, so the pure function is checked
against autograd through F.conv2d in fp64: dWk == w.grad and tot == Z.grad summed over the sites, to 1e-12 of the largest reference
magnitude (fp64 sums of at most a few thousand terms; measured <= 7e-16 on the shapes below).  The degenerate maps (H = 1: row 0 and
row H-1 are the same row) check the inclusion-exclusion of the regions.

GPU: the native entry against the pure function on the same device inputs.  Wd is one rounding of the same fp32 value: bit-equal.
S and tot are fp64 sums in a different order: within (n_terms + 16) 2^-52 sum|terms|, n_terms = 9 (S), 9 C2 (tot).  dWk is the fp32
rounding of S bg: within one fp32 rounding of it plus S's bound times |bg|."""
import pytest
import torch
import torch.nn.functional as F

F64 = torch.float64


def _region_sums(t):
    """(B, C, H, W) -> (9, C): [all, row 0, row H-1, col 0, col W-1, corner(0,0), corner(0,W-1), corner(H-1,0), corner(H-1,W-1)]"""
    return torch.stack([t.sum((0, 2, 3)), t[:, :, 0].sum((0, 2)), t[:, :, -1].sum((0, 2)), t[:, :, :, 0].sum((0, 2)),
                        t[:, :, :, -1].sum((0, 2)), t[:, :, 0, 0].sum(0), t[:, :, 0, -1].sum(0), t[:, :, -1, 0].sum(0),
                        t[:, :, -1, -1].sum(0)])


def _inputs(B, H, W, C2, Cin, affine, gen, dev="cpu"):
    """the function's arguments for dY = k0 + k1 Y + rows on a (B, H, W) map, and dY itself; all fp64"""
    R = B * H * W
    rows = torch.randn(B, C2, H, W, dtype=F64, generator=gen)
    Y = torch.randn(B, C2, H, W, dtype=F64, generator=gen)
    k0, k1 = (torch.randn(2, C2, dtype=F64, generator=gen) if affine else torch.zeros(2, C2, dtype=F64))
    dY = k0[None, :, None, None] + k1[None, :, None, None] * Y + rows
    regY, regR = _region_sums(Y), _region_sums(rows)
    stats2 = torch.cat([regY[0] / R, torch.ones(C2, dtype=F64)])             # mean | rstd: sum Y over all sites = mean * R
    ab2 = torch.cat([torch.ones(C2, dtype=F64), torch.zeros(C2, dtype=F64)])     # a = 1 and st2[:C2] = sum of the rows over all sites
    st2 = torch.cat([regR[0], torch.zeros(2 * C2, dtype=F64)])
    reg = torch.cat([regY[1:], regR[1:]])
    cnt = torch.tensor([R, B * W, B * W, B * H, B * H, B, B, B, B], dtype=F64)
    w = torch.randn(C2, Cin, 3, 3, dtype=F64, generator=gen)
    bgz = torch.rand(Cin, dtype=F64, generator=gen)
    args = dict(stats2=stats2, ab2=ab2, st2=st2, k01=torch.cat([k0, k1]), reg=reg, cnt=cnt, conv_w=w, bgz=bgz)
    return {k: v.to(dev) for k, v in args.items()}, dY


@pytest.mark.parametrize("affine", [False, True], ids=["rows_only", "k0_k1"])
@pytest.mark.parametrize("shape", [(2, 5, 7, 8, 16), (3, 2, 2, 16, 24), (1, 1, 4, 8, 8), (1, 3, 1, 8, 8), (1, 1, 1, 8, 8)], ids=str)
def test_pure_region_algebra_against_autograd_on_a_constant_map(shape, affine):
    from gdmae_hip import decoder as gdec
    B, H, W, C2, Cin = shape
    gen = torch.Generator().manual_seed(7 + sum(shape))
    a, dY = _inputs(B, H, W, C2, Cin, affine, gen)
    w = a["conv_w"].clone().requires_grad_()
    Z = a["bgz"][None, :, None, None].expand(B, Cin, H, W).clone().requires_grad_()
    (F.conv2d(Z, w, padding=1) * dY).sum().backward()
    S, tot, dWk, Wd = gdec.region_algebra_torch(a["stats2"], a["ab2"], a["st2"], a["k01"], a["reg"], gdec._TAP_REGION, a["cnt"],
                                                B * H * W, a["conv_w"], a["bgz"], F64)
    assert dWk.dtype == F64 and tot.dtype == F64 and S.shape == (9, C2)
    want_w, want_tot = w.grad, Z.grad.sum((0, 2, 3))
    e_w = float((dWk.permute(1, 2, 0).reshape(C2, Cin, 3, 3) - want_w).abs().max()) / float(want_w.abs().max())
    e_t = float((tot - want_tot).abs().max()) / float(want_tot.abs().max())
    print("[region algebra %s %s] dW %.2e  tot %.2e of the largest reference magnitude" % (shape, "k0 k1" if affine else "rows", e_w, e_t))
    assert e_w <= 1e-12 and e_t <= 1e-12, (e_w, e_t)
    assert torch.equal(Wd, a["conv_w"].permute(2, 3, 0, 1).reshape(9, C2, Cin))


@pytest.mark.gpu
@pytest.mark.parametrize("cdt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C2,Cin", [(128, 384), (8, 24)])
def test_native_region_algebra_against_the_pure_function(C2, Cin, cdt):
    from gdmae_hip import decoder as gdec
    B, H, W = 2, 5, 7
    R = B * H * W
    d = torch.device("cuda:0")
    a, _ = _inputs(B, H, W, C2, Cin, True, torch.Generator().manual_seed(C2 + Cin), d)
    # the dtypes of the head: fp32 a | b, k0 | k1 and weight, the background in the compute dtype
    a.update(ab2=a["ab2"].float(), k01=a["k01"].float(), conv_w=(a["conv_w"] * 0.05).float().contiguous(), bgz=a["bgz"].to(cdt))
    tap_region, cnt = gdec._region_consts(d, B, H, W)
    args = (a["stats2"], a["ab2"], a["st2"], a["k01"], a["reg"], tap_region, cnt, R, a["conv_w"], a["bgz"], cdt)
    S, tot, dWk, Wd = gdec.region_algebra_native(*args)
    S_r, tot_r, dWk_r, Wd_r = gdec.region_algebra_torch(*args)
    torch.cuda.synchronize()
    assert torch.equal(Wd, Wd_r) and Wd.dtype == cdt
    u64, u32 = 2.0 ** -52, 2.0 ** -24
    k0, k1 = a["k01"][:C2].double(), a["k01"][C2:].double()
    regY = torch.cat([(a["stats2"][:C2] * R)[None], a["reg"][:8]])
    regR = torch.cat([(a["ab2"][:C2].double() * a["st2"][:C2])[None], a["reg"][8:]])
    bound_S = (9 + 16) * u64 * (tap_region.abs() @ ((cnt[:, None] * k0).abs() + (regY * k1).abs() + regR.abs()))           # (9, C2)
    Wk = a["conv_w"].permute(2, 3, 0, 1).reshape(9, C2, Cin).double()
    bound_tot = (9 * C2 + 16) * u64 * torch.einsum('ko,koi->i', S_r.abs(), Wk.abs())
    bg = a["bgz"].double()
    bound_dW = u32 * (S_r[:, :, None] * bg).abs() + bound_S[:, :, None] * bg.abs()
    e_S, e_tot, e_dW = (S - S_r).abs(), (tot - tot_r).abs(), (dWk.double() - S_r[:, :, None] * bg).abs()
    print("[native region algebra C2 %d Cin %d %s] worst error / bound: S %.3f  tot %.3f  dWk %.3f" % (
        C2, Cin, cdt, float((e_S / bound_S).max()), float((e_tot / bound_tot).max()), float((e_dW / bound_dW).max())))
    assert bool((e_S <= bound_S).all()) and bool((e_tot <= bound_tot).all()) and bool((e_dW <= bound_dW).all())
