"""tests/optimizer_reference.py is what tests/test_optimizer_step_gpu.py measures the HIP optimizer step against; this file checks
the reference itself, on the CPU:
  * step_f64 equals torch.optim.Adam in float64 with the manual decay and clip_grad_norm_ (independent of the oracle) and
    oracle.optim_oracle.AdamOneCycle on the golden optimizer.npz trajectory;
  * bounds() is sound: step_f32 (float32, the oracle's operation order) lies inside it on every crafted case;
  * bounds() is sharp enough: each wrong variant in MUTATIONS lands at least 5 x outside it on at least one crafted case;
  * FlatAdamOneCycle's segment list: adjacent optimised ranges merge, more than 64 disjoint ones raise.
"""
import os

import numpy as np
import pytest
import torch

import optimizer_reference as R
from gdmae_hip import configs, optim
from oracle import optim_oracle as oo

Z = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "optimizer.npz")))

# the crafted calls the soundness and mutation checks run on: every parameter set on every small segment list, and on one list
# with a segment beyond 1 048 576 elements
SMALL = [(name, ps.name) for name in ("odd", "touching", "empties", "64") for ps in R.PARAM_SETS]
LARGE = [("short-long", ps.name) for ps in R.PARAM_SETS]


def _case(lst, ps_name):
    n, seg = R.SEGMENT_LISTS[lst]
    return R.case(n, ps_name, tuple(seg))


def _ratio(got, ref, bound):
    """worst |got - ref| / bound; a difference where the bound is zero counts as infinitely far out, a NaN as no evidence"""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    d = np.where(np.isnan(d), 0.0, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d > 0, np.inf, 0.0))
    return float(q.max())


def test_step_f64_equals_torch_adam_with_manual_decay_and_clip():
    for ps in R.PARAM_SETS:
        if ps.total is None:
            continue
        k = ps.kw
        rng = np.random.default_rng(5)
        n = 257
        p, g, m, v = rng.normal(size=n), rng.normal(size=n), rng.normal(size=n) * 0.1, rng.uniform(0.01, 1.0, n)
        f = lambda x: float(np.float32(x))
        sq = float((g * g).sum())
        ref = R.step_f64(p, g, m, v, [(0, n)], **{**k, "sq_norm": sq})
        tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
        adam = torch.optim.Adam([tp], lr=f(k["lr"]), betas=(f(k["beta1"]), f(k["beta2"])), eps=f(k["eps"]), weight_decay=0)
        adam.state[tp] = {"step": torch.tensor(float(k["t"] - 1)), "exp_avg": torch.from_numpy(m.copy()),
                          "exp_avg_sq": torch.from_numpy(v.copy())}
        tp.grad = torch.from_numpy(g * f(k["grad_scale"]))                  # the averaged gradient
        torch.nn.utils.clip_grad_norm_([tp], f(k["max_norm"]))
        with torch.no_grad():
            tp.mul_(1 - f(k["wd"]) * f(k["lr"]))
        adam.step()
        st = adam.state[tp]
        for a, b in zip(ref, (tp.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy())):
            assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), ps.name


def test_step_f64_follows_the_golden_trajectory_like_the_oracle():
    shapes = [tuple(int(v) for v in s if v > 0) for s in Z["shapes"]]
    n = sum(int(np.prod(s)) for s in shapes)
    p, m, v = Z["init"][:n].astype(np.float64), np.zeros(n), np.zeros(n)
    ps = [torch.from_numpy(Z["init"][:n].copy()).requires_grad_(True)]
    opt = oo.AdamOneCycle(ps, wd=0.01)
    for t in range(3):
        lr, b1 = oo.one_cycle(t, 100, 0.003, [0.95, 0.85], 10, 0.4)
        g = Z["grads"][t][:n].astype(np.float64)
        p, m, v = R.step_f64(p, g, m, v, [(0, n)], lr=lr, beta1=b1, beta2=0.99, eps=1e-8, wd=0.01, t=t + 1, max_norm=10.0,
                             grad_scale=1.0, sq_norm=float((g * g).sum()))
        ps[0].grad = torch.from_numpy(Z["grads"][t][:n].copy())
        opt.step(lr, b1)
        assert np.abs(p - Z["traj"][t][:n]).max() <= 2e-6 * np.abs(Z["traj"][t]).max()
        assert np.abs(p - ps[0].detach().numpy()).max() <= 2e-6 * np.abs(Z["traj"][t]).max()


@pytest.mark.parametrize("lst,ps_name", SMALL + LARGE)
def test_float32_step_lies_inside_the_bounds(lst, ps_name):
    """the condition that bounds() is sound"""
    c = _case(lst, ps_name)
    got = R.step_f32(c.p, c.g, c.m, c.v, c.segments, **c.ps.kw)
    for name, a, r, b, x in zip("pmv", got, c.ref, c.bounds, (c.p, c.m, c.v)):
        assert np.isfinite(r).all() and np.isfinite(a).all(), name
        assert np.array_equal(a[~c.inside], x[~c.inside]) and np.array_equal(r[~c.inside], x[~c.inside].astype(np.float64))
        q = _ratio(a, r, b)
        print(f"{lst} {ps_name} {name}: float32 / bound {q:.3f}")
        assert q <= 1.0, (name, q)


def test_reference_touches_exactly_the_segments_and_updates_below_one_ulp_survive():
    c = _case("odd", "t1000-lrend")
    # lr at the end of the schedule: the step is below one ulp of most O(1) parameters, the float64 reference still moves them
    big = c.inside & (np.abs(c.p) >= 1.0) & (c.g != 0)
    assert big.sum() > 100 and (np.abs(c.ref[0][big] - c.p[big].astype(np.float64)) < np.spacing(np.abs(c.p[big]))).mean() > 0.9
    assert (c.ref[0][big] != c.p[big]).all()
    z = c.inside & (c.g == 0)
    k = c.ps.kw
    assert z.any() and np.array_equal(c.ref[0][z], c.p[z].astype(np.float64) * (1.0 - float(np.float32(k["wd"])) * float(np.float32(k["lr"]))))
    assert not c.ref[1][z].any() and not c.ref[2][z].any()


@pytest.mark.parametrize("key", sorted(k for k, v in R.MUTATIONS.items() if v[1] == "step"))
def test_each_wrong_step_lands_five_times_outside_the_bounds(key):
    what, _, fn = R.MUTATIONS[key]
    worst, where = 0.0, None
    for lst, ps_name in (LARGE if key == "g" else SMALL):
        c = _case(lst, ps_name)
        got = fn(c.p, c.g, c.m, c.v, c.segments, **c.ps.kw)
        q = max(_ratio(a, r, b) for a, r, b in zip(got, c.ref, c.bounds))
        if q > worst:
            worst, where = q, (lst, ps_name)
    print(f"mutation {key} ({what}): {worst:.3g} x the bound on {where}")
    assert worst >= 5.0, (key, what, worst)


def test_shadow_rounding_reference_and_its_truncating_variant():
    x = R.SHADOW_EDGE_BITS.view(np.float32)
    assert np.array_equal(R.bf16_bits(x), R.SHADOW_EDGE_EXPECT)
    assert np.array_equal(torch.from_numpy(x.copy()).bfloat16().view(torch.int16).numpy().view(np.uint16), R.SHADOW_EDGE_EXPECT)
    c = _case("odd", "t2-clip-gs8")
    p32 = c.ref[0].astype(np.float32)
    assert np.array_equal(torch.from_numpy(p32).bfloat16().view(torch.int16).numpy().view(np.uint16), R.bf16_bits(p32))
    _, kind, trunc = R.MUTATIONS["h"]
    assert kind == "shadow" and (trunc(p32) != R.bf16_bits(p32)).mean() > 0.25        # differs in bits on about half the elements
    assert (trunc(x) != R.SHADOW_EDGE_EXPECT).any()


def test_norm_chain_and_planted_indices():
    assert R.NORM_CHAIN < 64
    assert R.planted_indices(1) == [0] and R.planted_indices(4) == [0, 3] and R.planted_indices(5) == [0, 3, 4]
    assert R.planted_indices(4194305) == [0, 1048576, 2097152, 3145728, 4194303, 4194304]
    assert len(R.planted_indices(9000003)) == 9 + 3 and R.planted_indices(9000003)[-3:] == [8999999, 9000000, 9000002]


class _Mixed(torch.nn.Module):
    """a direct parameter on a module that also has a child: the reference's leaf-module rule leaves it frozen"""

    def __init__(self, k):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(k))
        self.lin = torch.nn.Linear(2, 2)


def _model(kinds):
    net = torch.nn.Module()
    for i, kind in enumerate(kinds):
        setattr(net, f"c{i}", _Mixed(3) if kind == "mixed" else torch.nn.Linear(3, 2))
    return net


def test_more_than_64_disjoint_optimised_ranges_raise():
    top = lambda name: name.split(".")[0]
    with pytest.raises(ValueError, match="65 disjoint"):
        optim.FlatAdamOneCycle(_model(["mixed"] * 65), configs.optimization_cfg(), total_steps=10, bucket_of=top)
    opt = optim.FlatAdamOneCycle(_model(["mixed"] * 64), configs.optimization_cfg(), total_steps=10, bucket_of=top)
    assert len(opt.segments) == 128 and len(opt.frozen) == 64


def test_adjacent_optimised_ranges_merge_into_one_segment():
    top = lambda name: name.split(".")[0]
    # buckets: c0 (8 optimised), c1 (8 optimised), c2 (6 optimised + 3 frozen), c3 (8 optimised)
    opt = optim.FlatAdamOneCycle(_model(["leaf", "leaf", "mixed", "leaf"]), configs.optimization_cfg(), total_steps=10, bucket_of=top)
    assert [b for b, _, _ in opt.buckets] == ["c0", "c1", "c2", "c3"]
    assert opt.segments == [0, 22, 25, 33] and opt.n == 33 and opt.n_opt == 30
    assert [tuple(p.shape) for p in opt.frozen] == [(3,)]
