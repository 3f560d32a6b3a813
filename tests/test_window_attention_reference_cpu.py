"""The attention reference of tests/window_attention_reference.py against the oracle, and the input conditions that
tests/test_window_attention_gpu.py relies on - asserted here, on the CPU, so that the crafted inputs cannot drift unnoticed."""
import numpy as np
import pytest
import torch

import window_attention_reference as war
from oracle import gdmae_oracle as orc


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("tau", [0.37, war.TAU_MIN, 0.004])
def test_reference_equals_oracle(tau):
    """``orc.cosine_window_attention`` computes q, k, v from one input row; to hand it the given ``qk`` / ``v`` its input is the row
    [q | k | v] (width 3 d, 3 H heads of the same head dim), ``pos`` is zero, ``out_proj`` the identity and ``in_proj`` the block
    permutations that make its q = [q|k|v], k = [k|v|q], v = [v|q|k]: heads do not mix, so its first d output columns are the
    attention of (q, k, v) and, with a loss on those columns only, the gradient of its input row is [dq | dk | dv]."""
    d, H = 64, 4
    w = war.build_windows("edges")
    p = war.plan_fields(w)
    g = torch.Generator().manual_seed(3)
    n = w["n"]
    qk = torch.randn(n, 2 * d, generator=g, dtype=torch.float64)
    v = torch.randn(n, d, generator=g, dtype=torch.float64)
    dout = torch.randn(n, d, generator=g, dtype=torch.float64)
    out, dqk, dv, dtau = war.evaluate(torch.float64, qk, v, dout, tau, w, H)

    D = 3 * d
    eye = torch.eye(d, dtype=torch.float64)
    blk = lambda order: torch.cat([torch.cat([eye if c == o else torch.zeros_like(eye) for c in range(3)], 1) for o in order], 0)   # noqa: E731
    pfx = "a."
    sd = {pfx + "in_proj_weight": torch.cat([blk((0, 1, 2)), blk((1, 2, 0)), blk((2, 0, 1))], 0),
          pfx + "in_proj_bias": torch.zeros(3 * D, dtype=torch.float64),
          pfx + "out_proj.weight": torch.eye(D, dtype=torch.float64), pfx + "out_proj.bias": torch.zeros(D, dtype=torch.float64),
          pfx + "tau": torch.full((1, 1, 1), tau, dtype=torch.float64).requires_grad_(True)}
    x = torch.cat([qk, v], 1).requires_grad_(True)
    # unreferenced rows have level -1: the oracle's partition leaves them out of every window and returns zero rows for them
    part = {"level": torch.from_numpy(p["tok_level"]), "slot": torch.from_numpy(p["tok_slot"]),
            "num_win": {lv: int(nw) for lv, nw in enumerate(w["n_win"])}}
    di = {lv: {"max_tokens": T, "drop_range": [0, 0]} for lv, T in enumerate(w["max_tokens"])}
    oo = orc.cosine_window_attention(x, torch.zeros(n, D, dtype=torch.float64), part, di, sd, pfx, 3 * H, tau_min=war.TAU_MIN)
    oo[:, :d].backward(dout)
    assert _rel(out, oo[:, :d].detach()) < 1e-12
    assert _rel(dqk, x.grad[:, :2 * d]) < 1e-12
    assert _rel(dv, x.grad[:, 2 * d:]) < 1e-12
    got_tau = float(sd[pfx + "tau"].grad.reshape(()))
    if tau < war.TAU_MIN:
        assert float(dtau) == 0.0 and got_tau == 0.0
    else:
        assert float(dtau) != 0.0 and abs(float(dtau) - got_tau) <= 1e-12 * abs(got_tau)
    assert float(out[w["unref"]].abs().max()) == 0.0 and float(dqk[w["unref"]].abs().max()) == 0.0


@pytest.mark.parametrize("name", list(war.WINDOW_LISTS))
def test_window_lists(name):
    """Every list names each referenced row exactly once, leaves row 0, the last row and two middle rows out, stores its windows
    level by level within the level's capacity, ascending token rows inside a window, and stays under 1000 rows."""
    w = war.build_windows(name)
    n = w["n"]
    assert n < 1000
    count = np.bincount(w["csr"], minlength=n)
    ref_rows = np.setdiff1d(np.arange(n), w["unref"])
    assert (count[ref_rows] == 1).all() and (count[w["unref"]] == 0).all()
    assert len(w["unref"]) == 4 and w["unref"][0] == 0 and w["unref"][-1] == n - 1 and 0 < w["unref"][1] < w["unref"][2] < n - 1
    assert int(w["win_len"].sum()) == len(w["csr"]) == n - 4 and len(w["win_len"]) == sum(w["n_win"])
    assert np.array_equal(w["win_start"], np.concatenate([[0], np.cumsum(w["win_len"])[:-1]]))
    assert (np.diff(w["level_of_win"]) >= 0).all()
    for i, (s, k) in enumerate(zip(w["win_start"], w["win_len"])):
        assert 1 <= k <= w["max_tokens"][w["level_of_win"][i]]
        assert (np.diff(w["csr"][s:s + k]) > 0).all()
    p = war.plan_fields(w)
    assert (p["tok_level"][w["unref"]] == -1).all() and (p["tok_level"][ref_rows] >= 0).all()
    assert sum(p["n_tok"]) == n - 4


def test_shipped_boundaries_are_in_the_edges_list():
    """DROP_INFO of the shipped configs is [0, 16) / [16, 32) / [32, ...): a 16-token window is a T = 32 window, a 32-token window
    a T = 64 window."""
    from gdmae_hip import configs
    lv = configs._drop_info()["train"]
    level_of = lambda k: next(int(i) for i, e in lv.items() if e["drop_range"][0] <= k < e["drop_range"][1])   # noqa: E731
    mt, lens = war.WINDOW_LISTS["edges"]
    assert mt == [lv[str(i)]["max_tokens"] for i in range(3)] == [16, 32, 64]
    assert level_of(16) == 1 and 16 in lens[1] and level_of(32) == 2 and 32 in lens[2]
    assert war.WINDOW_LISTS["reordered"][0] == [64, 16, 32]
    assert war.WINDOW_LISTS["no64-3lv"][1][2] == [] and len(war.WINDOW_LISTS["no64-2lv"][0]) == 2


@pytest.mark.parametrize("d,H", war.SHAPES)
@pytest.mark.parametrize("name", list(war.WINDOW_LISTS))
def test_inputs_and_yardstick(name, d, H):
    """No head slice of q or k is near zero unless the zero-norm edit put it there, and the float32 yardstick and the float64
    reference are finite for every tau."""
    dh = d // H
    for bf16 in (False, True):
        w, qk, v, dout = war.make_inputs(name, d, H, bf16)
        norms = qk.view(w["n"], 2 * H, dh).norm(dim=-1)
        assert float(norms.min()) > 1e-3
        for tau in war.TAUS:
            _, _, _, _, ref, y, f32, _ = war.cached_reference(name, d, H, tau, bf16)
            for t in ref + f32:
                assert bool(torch.isfinite(t).all())
            assert all(np.isfinite(y)) and max(y) < 1e-3, y


def test_zero_norm_edit():
    """The edit zeroes exactly one q slice and one k slice per level, in two different rows of one window; the edited query's head-0
    output is the plain mean of the window's v slices; the edited rows' gradients are finite and of the order 1 / eps."""
    for d, H in war.SHAPES:
        dh = d // H
        w, qk, v, dout, ref, _, f32, edits = war.cached_reference("edges", d, H, 0.2, True, zero_norm=True)
        w0, qk0, _, _ = war.make_inputs("edges", d, H, True)
        assert len(edits) == 3 and int((qk != qk0).any(dim=1).sum()) == 6
        norms = qk.view(w["n"], 2 * H, dh).norm(dim=-1)
        assert int((norms == 0).sum()) == 6 and float(norms[norms > 0].min()) > 1e-3
        out, dqk = ref[0], ref[1]
        for wi, rq, rk in edits:
            s, k = int(w["win_start"][wi]), int(w["win_len"][wi])
            rows = w["csr"][s:s + k]
            assert rq in rows and rk in rows and rq != rk
            mean = v[rows, :dh].double().mean(0)
            assert float((out[rq, :dh] - mean).abs().max()) <= 1e-12 * float(mean.abs().max())
            assert float(dqk[rq, :dh].abs().max()) > 1e9 and float(dqk[rk, d + 3 * dh:d + 4 * dh].abs().max()) > 1e9
        for t in ref + f32:
            assert bool(torch.isfinite(t).all())


@pytest.mark.parametrize("name", ["edges", "only16-five"])
def test_below_the_clamp_equals_the_clamp(name):
    """tau = 0.004 < tau_min: out, dqk and dv equal the evaluation at tau = tau_min exactly and dtau is 0; at tau = tau_min itself
    the clamp's gradient passes."""
    d, H = 128, 8
    at = war.cached_reference(name, d, H, war.TAU_MIN, False)[4]
    below = war.cached_reference(name, d, H, 0.004, False)[4]
    for a, b in zip(at[:3], below[:3]):
        assert torch.equal(a, b)
    assert float(below[3]) == 0.0 and float(at[3]) != 0.0
