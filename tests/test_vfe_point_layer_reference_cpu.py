"""Conditions on the float64 reference of the first DynVFE point layer (tests/vfe_point_layer_reference.py) that must hold before
anything runs on a GPU: it is the oracle's DynVFE layer and autograd's BatchNorm backward; its bounds are tight against |z| (the
cancellation case far_tight is held to its own, looser figure, on record), leave few ReLU signs undecided, leave none within 4 d_z of
zero in the small backward cases; and every wrong variant a kernel change could plausibly produce lands outside them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import vfe_point_layer_reference as R
from oracle import gdmae_oracle as orc

F64 = torch.float64


def _fw(case, F):
    return R.scene_forward(case, F)


# ====================================================================================================== the reference is right
@pytest.mark.parametrize("F", [3, 4, 5])
def test_forward_is_the_oracle_layer(F):
    """decoration: centre and raw columns bit-equal to orc.dyn_vfe, the cluster columns to the few ulps of |xyz| by which the oracle's
    fp32 sequential pillar mean differs from the fp64 mean rounded once (pillars of <= 8 points: 8 additions + 1 division);
    BatchNorm + ReLU on the SAME fp32 features: orc.batch_norm_train within d_z, running statistics within their bounds;
    the pillar maximum of the whole oracle layer within d_z plus what the mean's ulps do to z."""
    s, fw = R.scene("edges_129", F), _fw("edges_129", F)
    sd = {"vfe.dvfe_mlps.0.0.weight": s.W, "vfe.dvfe_mlps.0.1.weight": s.gamma, "vfe.dvfe_mlps.0.1.bias": s.beta}
    vf, mean, deco = orc.dyn_vfe(s.points, s.point_coords, s.inverse32.long(), s.M, sd, R.LO + (38.4, 38.4, 3.0), R.VS)
    f = R.decorate(s.points, s.point_coords, s.inverse32, s.pillar_mean)
    assert torch.equal(f, R.scene_features(s)[s.perm]), "the two layouts decorate the same rows differently"
    assert torch.equal(deco[:, :3 + F], f[:, :3 + F])
    d_clu = 10 * R.U * float(s.points[:, 1:4].abs().max())
    assert float((deco[:, 3 + F:] - f[:, 3 + F:]).abs().max()) <= d_clu
    assert float((mean - s.pillar_mean).abs().max()) <= d_clu
    # the same fp32 rows through the oracle's BatchNorm
    fpm = R.scene_features(s)
    run = {"mean": s.rm0.clone(), "var": s.rv0.clone(), "n": 7}
    y = torch.relu(orc.batch_norm_train(TF.linear(fpm, s.W), s.gamma, s.beta, run))
    assert R.worst_ratio(y, fw.y, fw.d_z) <= 1.0
    assert R.worst_ratio(run["mean"], fw.rm, fw.d_rm) <= 1.0 and R.worst_ratio(run["var"], fw.rv, fw.d_rv) <= 1.0 and run["n"] == 8
    # the whole oracle layer, pillar maximum included
    ymax = torch.stack([fw.y[a:b].max(0).values for a, b in zip(s.pt_off[:-1].tolist(), s.pt_off[1:].tolist())])
    dmax = torch.stack([fw.d_z[a:b].max(0).values for a, b in zip(s.pt_off[:-1].tolist(), s.pt_off[1:].tolist())])
    dmax = dmax + 1.5 * fw.a.abs() * s.W.double()[:, 3 + F:].abs().sum(1) * d_clu       # 1.5: the statistics move with the rows
    assert R.worst_ratio(vf, ymax, dmax) <= 1.0


@pytest.mark.parametrize("case", ["one_tile", "edges_33", "crowded"])
@pytest.mark.parametrize("F", [3, 4, 5])
def test_backward_is_autograd_through_batchnorm(case, F):
    s, fw = R.scene(case, F), _fw(case, F)
    W, gamma, beta = (t.double().requires_grad_() for t in (s.W, s.gamma, s.beta))
    h = fw.f @ W.t()
    y = torch.relu((h - h.mean(0)) / torch.sqrt(h.var(0, unbiased=False) + R.EPS) * gamma + beta)
    assert torch.allclose(y, fw.y, rtol=1e-12, atol=1e-12)
    (y * s.g32.double()).sum().backward()
    bw = R.backward(fw, fw.stats, fw.ab, s.gamma, s.g32)
    for name, got, want in (("dW", bw.dW, W.grad), ("dgamma", bw.dgamma, gamma.grad), ("dbeta", bw.dbeta, beta.grad)):
        assert float((got - want).abs().max()) <= 1e-10 * float(want.abs().max()) + 1e-13, name


def test_single_point_scene():
    """N = 1: the variance is exactly 0, z = beta, the unbiased factor is guarded and dW is zero up to cancellation"""
    s, fw = R.scene("single", 4), _fw("single", 4)
    assert s.N == 1 and float(fw.var.abs().max()) == 0.0 and torch.allclose(fw.z[0], s.beta.double(), atol=1e-9)
    assert torch.allclose(fw.rv, s.rv0.double() * (1 - R.MOM))
    bw = R.backward(fw, fw.stats, fw.ab, s.gamma, s.g32)
    assert float(bw.dW.abs().max()) <= 1e-9 * float((fw.a * s.g32.double().abs().max() * fw.f.abs().max()).max())


# ====================================================================================================== the bounds are a net
@pytest.mark.parametrize("case,F", [(c, F) for c in R.CASES for F in (3, 4, 5) if (c, F) != ("deep", 3)])      # deep: F = 4 and 5 only
def test_bounds_are_tight_and_leave_few_signs_open(case, F):
    fw = _fw(case, F)
    ratio = float(fw.d_z.max() / fw.z.abs().max())
    share = float((fw.z.abs() <= fw.d_z).double().mean())
    print(f"{case} F={F}: max d_z / max|z| {ratio:.3e}, ambiguous share {share:.3e}")
    if case == "far_tight":
        # mean^2 / var of the absolute x and y columns is ~ (25.6 m / 0.9 m)^2: d_var carries 2 |mean| d_mean and E[h^2] >> var.
        # Evaluated for the reference alone: 2.7e-3 .. 4.8e-3 over F = 3, 4, 5 - the price of the one-pass variance, kept on record.
        assert 1e-3 < ratio <= 1e-2
    else:
        assert ratio <= 1e-3
    assert share <= 1e-3
    if case in R.BWD_SMALL:
        assert int((fw.z.abs() <= 4 * fw.d_z).sum()) == 0, "pick another scene seed (vfe_point_layer_reference.SEEDS)"


def _exceeds(got, ref, bound):
    return bool(((got - ref).abs() > bound).any())


def _y(f, s, **kw):
    return R.bn_relu(f.double() @ s.W.double().t(), s.gamma.double(), s.beta.double(), **kw)


@pytest.mark.parametrize("F", [3, 4, 5])
def test_bounds_reject_wrong_forwards(F):
    """each wrong variant, computed in float64, leaves the bound of y in the case named (and the statistics' where it changes them)"""
    for case in ("tiny", "crowded"):                         # unbiased instead of biased variance
        s, fw = R.scene(case, F), _fw(case, F)
        assert _exceeds(_y(fw.f, s, unbiased=True), fw.y, fw.d_z), case
        assert _exceeds(fw.var * s.N / (s.N - 1), fw.var, fw.d_var), case
    for case in ("one_tile", "crowded", "far_tight"):
        s, fw = R.scene(case, F), _fw(case, F)
        # centre without + 0.5: a constant per feature column, which BatchNorm removes from y (and from every gradient: sum dx = 0) -
        # it shows in the statistics the call returns (mean, b, the running mean) and in gdmae_decorate_points
        m = (R.scene_features(s, half=0.0).double() @ s.W.double().t()).mean(0)
        assert _exceeds(m, fw.mean, fw.d_mean) and _exceeds(s.beta.double() - fw.a * m, fw.b, fw.d_b), (case, "centre without + 0.5")
        assert _exceeds(_y(R.scene_features(s, mean_roll=1), s), fw.y, fw.d_z), (case, "cluster offset of pillar p + 1")
    for case in ("edges_33", "crowded"):                     # rows r and r + 4 of a tile swapped; the last W column dropped
        s, fw = R.scene(case, F), _fw(case, F)
        y = fw.y.clone()
        r = next(r for r in range(28) if not torch.equal(fw.f[r], fw.f[r + 4]))       # (rows of a repeated-point pillar are equal)
        y[[r, r + 4]] = y[[r + 4, r]]
        assert _exceeds(y, fw.y, fw.d_z), case
        if F != 4:                                           # odd D: the padded K column of the last MFMA step
            Wd = s.W.double().clone()
            Wd[:, -1] = 0
            assert _exceeds(R.bn_relu(fw.f @ Wd.t(), s.gamma.double(), s.beta.double()), fw.y, fw.d_z), case
            assert _exceeds(((fw.f @ Wd.t()) ** 2).mean(0) - fw.mean ** 2, fw.var, fw.d_var), case   # (its column sums to ~ 0: not the mean)
    for n in (31, 32, 33, 127, 128, 129):                    # row N - 1 copied over row N - 2
        fw = _fw(f"edges_{n}", F)
        y = fw.y.clone()
        y[n - 2] = y[n - 1]
        assert _exceeds(y, fw.y, fw.d_z), n


@pytest.mark.parametrize("F", [4, 5])
def test_bounds_reject_a_lost_tile_of_the_third_pass(F):
    """tile 8 200 lies in a third or later pass whatever grid (<= 1 024 workgroups of 4 tiles) is launched: its 32 rows taken as zero
    rows by the statistics pass move mean and variance out of their bounds; written as relu(b) by the apply pass they leave d_z"""
    s, fw = R.scene("deep", F), _fw("deep", F)
    t = 8200
    assert t >= 2 * 4 * 1024 and (t + 1) * 32 <= s.N
    rows = slice(32 * t, 32 * t + 32)
    h = fw.h[rows]
    mean = fw.mean - h.sum(0) / s.N
    var = (fw.var + fw.mean ** 2) - (h * h).sum(0) / s.N - mean ** 2
    assert _exceeds(mean, fw.mean, fw.d_mean) and _exceeds(var, fw.var, fw.d_var)
    assert _exceeds(torch.relu(fw.b).expand(32, -1), fw.y[rows], fw.d_z[rows])


@pytest.mark.parametrize("case", ["edges_33", "crowded"])
@pytest.mark.parametrize("F", [3, 4, 5])
def test_bounds_reject_wrong_backwards(case, F):
    s, fw = R.scene(case, F), _fw(case, F)
    bw = R.backward(fw, fw.stats, fw.ab, s.gamma, s.g32)
    m = R.backward(fw, fw.stats, fw.ab, s.gamma, s.g32, mask=fw.h > 0)             # ReLU mask from h > 0
    assert _exceeds(m.dW, bw.dW, bw.d_dW) and _exceeds(m.dgamma, bw.dgamma, bw.d_dgamma) and _exceeds(m.dbeta, bw.dbeta, bw.d_dbeta)
    m = R.backward(fw, fw.stats, fw.ab, s.gamma, s.g32, drop_c0=True)              # c0 left out of dx
    assert _exceeds(m.dW, bw.dW, bw.d_dW)
    if F != 4:                                                                     # the last feature column dropped from dW
        assert bool((bw.dW[:, -1].abs() > bw.d_dW[:, -1]).any())
    # the bounds themselves stay small against the gradients
    for name in ("dW", "dgamma", "dbeta"):
        assert float(getattr(bw, "d_" + name).max()) <= 1e-3 * float(getattr(bw, name).abs().max()), name
