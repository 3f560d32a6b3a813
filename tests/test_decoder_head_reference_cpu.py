"""tests/decoder_head_reference.py checked on its own, without a GPU: its forward and gradients against torch.nn modules in float64 on the
dense map, backward_at against plain autograd, the edges its cases must reach, and the POWER of the bounds tests/test_decoder_head_gpu.py
derives from it - every mutation of the backward (decoder_head_reference.MUTATIONS: a dropped corner or edge term of the closed form,
pillar rows lost on a border row, relu' of the background, one (site, tap) pair, the partial tile, the running variance's count) moves
at least one asserted tensor by >= 5 x its GPU bound, in every case where it applies.  That is a condition on the cases (geometry and
seed), not a measurement of any kernel."""
import pytest
import torch

import decoder_head_reference as R

C = R.C
POWER = 5.0
RUNNING_RTOL = 1e-4


def _modules(c):
    bns = [torch.nn.BatchNorm2d(C, eps=R.EPS1 if i < 3 else R.EPS2, momentum=R.MOMENTUM).double() for i in range(4)]
    conv = torch.nn.Conv2d(3 * C, C, 3, padding=1, bias=False).double()
    with torch.no_grad():
        for i, bn in enumerate(bns):
            bn.weight.copy_(c.gamma[i] if i < 3 else c.gamma2)
            bn.bias.copy_(c.beta[i] if i < 3 else c.beta2)
            bn.running_mean.copy_(c.rm0[i])
            bn.running_var.copy_(c.rv0[i])
        conv.weight.copy_(c.conv_w)
    return bns, conv


@pytest.mark.parametrize("name", R.CASES)
def test_reference_equals_torch_modules_in_float64(name):
    c, ex = R.make_case(name), R.exact(name)
    bns, conv = _modules(c)
    Ps = [p.clone().requires_grad_() for p in c.P]
    maps = []
    for i, (sites, P) in enumerate(zip(c.sites, Ps)):
        x = torch.zeros(c.R, C, dtype=torch.float64).index_copy(0, sites, P)
        maps.append(torch.relu(bns[i](x.view(c.B, c.H, c.W, C).permute(0, 3, 1, 2))))
    dense = torch.relu(bns[3](conv(torch.cat(maps, 1)))).permute(0, 2, 3, 1).reshape(c.R, C)
    out = dense[c.pillar_cell]
    (out * c.up).sum().backward()
    tight = dict(rtol=1e-10, atol=1e-12)
    assert torch.allclose(out, ex["out"], **tight) and torch.allclose(dense, ex["dense"], **tight)
    for i, bn in enumerate(bns):
        assert torch.allclose(bn.running_mean, ex["running_mean%d" % i], **tight), i
        assert torch.allclose(bn.running_var, ex["running_var%d" % i], **tight), i
        assert int(bn.num_batches_tracked) == ex["num_batches_tracked"] == 1
    want = {"dW": conv.weight.grad, "dgamma2": bns[3].weight.grad, "dbeta2": bns[3].bias.grad}
    for i in range(3):
        want.update({"dP%d" % i: Ps[i].grad, "dgamma%d" % i: bns[i].weight.grad, "dbeta%d" % i: bns[i].bias.grad})
    worst = R.metrics(ex, want)
    assert max(worst.values()) < 1e-10, max(worst.items(), key=lambda kv: kv[1])


@pytest.mark.parametrize("name", R.CASES)
def test_backward_at_the_own_output_is_plain_autograd_and_follows_a_given_one(name):
    c, ex = R.make_case(name), R.exact(name)
    at = R.backward_at(c, ex["Y"])
    assert max(R.metrics(at, ex).values()) < 1e-12
    # a perturbed Y: the forward tensors follow it, and the gradients are those of a head whose convolution has that output
    Yp = ex["Y"] + 0.01 * torch.randn(ex["Y"].shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    at = R.backward_at(c, Yp)
    assert torch.equal(at["Y"], Yp) and torch.allclose(at["mean2"], Yp.mean(0), rtol=1e-12, atol=1e-14)
    moved = R.metrics(at, ex)
    assert moved["dbeta0"] > 1e-4 and moved["out"] > 1e-4


def test_cases_reach_the_edges():
    cs = {n: R.make_case(n) for n in R.CASES}
    assert all(c.H % 4 == 0 and c.W % 4 == 0 for c in cs.values())
    assert sum(c.H != c.W for c in cs.values()) >= 5 and {c.B for c in cs.values()} == {1, 2}
    for n in ("A", "F"):
        assert cs[n].H % 8 and cs[n].W % 8, "a partial last tile on both axes"
    assert all(cs[n].H % 8 == 0 and cs[n].W % 8 == 0 for n in ("B", "C", "D", "E"))
    assert [t.numel() for t in cs["F"].tok] == [1, 1, 1] and cs["B"].tok[2].numel() == 1 and cs["F"].M == 1 < 64
    # token counts that are no multiple of the block kernel's chunk (16 tokens at u = 2, 4 at u = 4: 64 sites)
    assert any(c.tok[1].numel() % 16 for c in cs.values()) and any(c.tok[2].numel() % 4 for c in cs.values())
    for n, c in cs.items():
        ex = R.exact(n)
        for i in range(3):
            pos, zero = ex["bg_signs%d" % i]
            assert pos >= 16 and zero >= 16, "background channels of both signs in every stage"
    # D: no token on the border; pillars in NON-ACTIVE tiles at sites of each of the 9 border classes
    d = cs["D"]
    allsites = torch.cat(d.sites)
    assert bool((R.site_class(d, allsites) == 4).all())
    off = ~R.active_tiles(d)[R.tile_of(d, d.pillar_cell)]
    assert set(R.site_class(d, d.pillar_cell[off]).tolist()) == set(range(9))
    # E: tokens only along row 0 and column W - 1, on both sides of a tile boundary; no pillar on an active site
    e = cs["E"]
    for u, t in zip(e.ups, e.tok):
        y, x = (t // (e.W // u)) % (e.H // u), t % (e.W // u)
        assert bool(((y == 0) | (x == e.W // u - 1)).all())
    x0 = e.sites[0][(e.sites[0] // e.W) % e.H == 0] % e.W
    assert {7, 8} <= set(x0.tolist())
    act = torch.zeros(e.R, dtype=torch.bool)
    act[torch.cat(e.sites)] = True
    assert not bool(act[e.pillar_cell].any())
    # A, C: tokens in all four coarse corners of every stage, a pillar on each edge
    for n in ("A", "C"):
        c = cs[n]
        for s in c.sites:
            assert {0, 2, 6, 8} <= set(R.site_class(c, s).tolist())
        assert {1, 3, 5, 7} <= set(R.site_class(c, c.pillar_cell).tolist())
    assert set(R.site_class(cs["B"], cs["B"].pillar_cell).tolist()) == set(range(9))


def _applies(c, m):
    if m == "m6":
        return c.W % 8 != 0
    if m == "m3":
        return bool(((c.pillar_cell // c.W) % c.H == c.H - 1).any())
    return True


@pytest.mark.parametrize("name", R.CASES)
def test_every_mutation_lands_outside_the_gpu_bounds(name):
    c, ex = R.make_case(name), R.exact(name)
    bound = R.bounds(name, "bf16")              # the wider of the two routes' bounds (fp32: 10 x d_ref of ~1e-6)
    assert all(R.bounds(name, "fp32")[k] <= v for k, v in bound.items())
    applied = 0
    for m in R.MUTATIONS:
        if not _applies(c, m):
            continue
        applied += 1
        mu = R.run(c, mutation=m)
        if m == "m7":
            ratio, which = max((R.close_ratio(mu["running_var%d" % i], ex["running_var%d" % i], RUNNING_RTOL, 0.0), "running_var%d" % i)
                               for i in range(3))
        else:
            assert all(torch.equal(mu[k], ex[k]) for k in R.FORWARD), "m1 - m6 change the backward only"
            moved = R.metrics(mu, ex, names=R.GRADS + ("dW",))
            ratio, which = max((moved[k] / bound[k], k) for k in moved)
        print("[decoder head reference %s] %s (%s): %s moves by %.1f x its GPU bound" % (name, m, R.MUTATIONS[m], which, ratio))
        assert ratio >= POWER, (m, which, ratio)
    assert applied >= 5
    assert _applies(c, "m6") == (name in ("A", "F")) and (_applies(c, "m3") or name not in ("A", "B", "C", "D", "F"))


def test_d_ref_is_of_the_size_the_rounding_predicts():
    """bf16 rounding is 2^-9 relative per element: after a few independent roundings a relative L2 of a few 1e-3; fp32: a few 1e-7 to
    1e-6.  A d_ref far outside would mean the emulation rounds something it should not (or nothing at all)."""
    for name in R.CASES:
        b, f = R.d_ref(name, "bf16"), R.d_ref(name, "fp32")
        assert all(2e-4 < v < 3e-2 for v in b.values()), (name, min(b.items(), key=lambda kv: kv[1]), max(b.items(), key=lambda kv: kv[1]))
        assert all(2e-8 < v < 2e-5 for v in f.values()), (name, min(f.items(), key=lambda kv: kv[1]), max(f.items(), key=lambda kv: kv[1]))
