"""The encoder stage through its real entry point (``gdmae_hip.encoder.encoder_stage`` -> ``EncoderStageFn`` ->
gdmae_encoder_stage_fwd / _bwd) against a float64 reference, output by output, gradient by gradient and layer by layer.

Layer path 1 runs the fused launches of csrc/layer_fused.hip (k_layer_fwd, k_layer_bwd_ffn, k_layer_bwd_in, k_ln2_bwd_top and
the tails that ride along); path 0 the launch-per-product sequence of csrc/encoder_layer.hip.  The parameters are owned by a
``FlatAdamOneCycle`` and the stage runs under bf16 autocast, as in the bench step.

The window plans are synthetic (random token permutation, every window-length edge of the three occupancy levels), the row
counts are picked at the row-tile and 2048-row padding edges, and the reference reads exactly the operands the kernels read:
bf16-rounded weights and biases, fp32 LayerNorm weights and tau, bf16-representable inputs.  Everything left is kernel error.

``test_reference_equals_oracle`` (CPU) pins the reference to ``oracle.gdmae_oracle.encoder_layer``, which the goldens pin to
the upstream model."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import gdmae_oracle as orc

NHEAD = 8
TAU_MIN = 0.01                     # LAYER_CFG.tau_min of the shipped configs (and the oracle's default)
LEVEL_T = (16, 32, 64)             # DROP_INFO max_tokens per occupancy level
EDGE_LENGTHS = (1, 16, 17, 32, 33, 64)
N_POS = 64                         # pos_table rows: the cells of an 8 x 8 window


def _ref_threads():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))


# ------------------------------------------------------------------------------------------------------------------------
# synthetic window plans
# ------------------------------------------------------------------------------------------------------------------------
def _level(length):
    return 0 if length <= 16 else (1 if length <= 32 else 2)


def synth_plan_arrays(n, seed):
    """Host arrays of one window partition of n tokens: the window lengths hold every edge length that fits (1, 16, 17, 32, 33,
    64) and random lengths within the planner's level bounds (1-16, 17-32, 33-64) for the rest; windows are stored level by
    level, as the planner emits them, and a window's tokens are scattered rows of a random permutation (ascending inside the
    window, the planner's canonical order).  A level without windows stays in the plan with n_win = 0, as for a sparse frame."""
    rng = np.random.default_rng(seed)
    edges = list(EDGE_LENGTHS)
    rng.shuffle(edges)
    lens, left = [], n
    for e in edges:
        if e <= left:
            lens.append(e)
            left -= e
    while left > 0:
        k = int(rng.integers(1, min(64, left) + 1))
        lens.append(k)
        left -= k
    rng.shuffle(lens)
    lens = [k for lv in range(3) for k in lens if _level(k) == lv]
    perm = rng.permutation(n)
    win_len = np.array(lens, dtype=np.int64)
    win_start = np.concatenate([[0], np.cumsum(win_len)[:-1]]).astype(np.int64)
    csr = np.empty(n, dtype=np.int64)
    tok_win = np.empty(n, dtype=np.int64)
    tok_level = np.empty(n, dtype=np.int64)
    tok_slot = np.empty(n, dtype=np.int64)
    tok_pos = np.empty(n, dtype=np.int64)
    n_win = [sum(1 for k in lens if _level(k) == lv) for lv in range(3)]
    local = [0, 0, 0]
    for w, (s, k) in enumerate(zip(win_start, win_len)):
        lv = _level(int(k))
        toks = np.sort(perm[s:s + k])
        csr[s:s + k] = toks
        tok_win[toks] = w
        tok_level[toks] = lv
        tok_slot[toks] = local[lv] * LEVEL_T[lv] + np.arange(k)
        tok_pos[toks] = rng.choice(N_POS, size=int(k), replace=False)      # distinct cells inside a window
        local[lv] += 1
    return dict(n=n, csr=csr, win_start=win_start, win_len=win_len, tok_win=tok_win, tok_level=tok_level, tok_slot=tok_slot,
                tok_pos=tok_pos, n_win=n_win, n_tok=[int(win_len[[_level(int(k)) == lv for k in win_len]].sum()) for lv in range(3)])


def to_window_plan(p, device):
    from gdmae_hip.plan import WindowPlan
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32).to(device)   # noqa: E731
    return WindowPlan(i32(p["tok_win"]), i32(p["tok_level"]), i32(p["tok_slot"]), i32(p["tok_pos"]), i32(p["csr"]),
                      i32(p["win_start"]), i32(p["win_len"]), list(p["n_win"]), list(p["n_tok"]), list(LEVEL_T))


def oracle_part(p):
    """The oracle's window partition dict (``orc.window_partition`` output fields the encoder layer reads)."""
    return {"level": torch.from_numpy(p["tok_level"]), "slot": torch.from_numpy(p["tok_slot"]),
            "num_win": {lv: int(p["n_win"][lv]) for lv in range(3)}}


ORACLE_DROP_INFO = {lv: {"max_tokens": LEVEL_T[lv], "drop_range": [0, 0]} for lv in range(3)}


def _level_index(p):
    """Per level: (window ids, (nW, T) token rows padded with row 0, (nW, T) live mask)."""
    out = []
    base = 0
    for lv in range(3):
        nw, T = p["n_win"][lv], LEVEL_T[lv]
        if nw == 0:
            continue
        wid = np.arange(base, base + nw)
        idx = np.zeros((nw, T), dtype=np.int64)
        live = np.zeros((nw, T), dtype=bool)
        for r, w in enumerate(wid):
            s, k = p["win_start"][w], p["win_len"][w]
            idx[r, :k] = p["csr"][s:s + k]
            live[r, :k] = True
        out.append((torch.from_numpy(wid), torch.from_numpy(idx), torch.from_numpy(live)))
        base += nw
    return out


# ------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ------------------------------------------------------------------------------------------------------------------------
PNAMES = ("Win", "bin", "tau", "Wo", "bo", "W1", "b1", "W2", "b2", "g1", "be1", "g2", "be2")   # = gdmae_hip.encoder._plist order


def ref_layer(x, pos, levels, p, tau_w, eps=1e-5):
    """Post-norm cosine-attention encoder layer over CSR windows: q = k = x + pos, v = x, per-head L2 normalisation, logits /
    clamp(tau_w, TAU_MIN) with one tau leaf per window, padded keys masked, LN(x + attn), erf-GELU FFN, LN(x1 + ffn)."""
    n, d = x.shape
    dh = d // NHEAD
    qk_in = x + pos
    q = F.linear(qk_in, p["Win"][:d], p["bin"][:d])
    k = F.linear(qk_in, p["Win"][d:2 * d], p["bin"][d:2 * d])
    v = F.linear(x, p["Win"][2 * d:], p["bin"][2 * d:])
    o = torch.zeros_like(x)
    for wid, idx, live in levels:
        nw, T = idx.shape
        heads = lambda t: t[idx].view(nw, T, NHEAD, dh).transpose(1, 2)   # noqa: E731
        qw, kw, vw = F.normalize(heads(q), dim=-1), F.normalize(heads(k), dim=-1), heads(v)
        logit = qw @ kw.transpose(-2, -1) / tau_w[wid].clamp(min=TAU_MIN).view(nw, 1, 1, 1)
        logit = logit.masked_fill(~live.view(nw, 1, 1, T), float("-inf"))
        ow = (logit.softmax(-1) @ vw).transpose(1, 2).reshape(nw, T, d)
        o = o.index_copy(0, idx[live], ow[live])
    x1 = F.layer_norm(x + F.linear(o, p["Wo"], p["bo"]), (d,), p["g1"], p["be1"], eps)
    f = F.linear(F.gelu(F.linear(x1, p["W1"], p["b1"])), p["W2"], p["b2"])
    return F.layer_norm(x1 + f, (d,), p["g2"], p["be2"], eps)


def ref_stage(x, dy, pos_table, plans, params, residual):
    """fp64 forward + autograd backward of the stage (layer i uses plans[i % 2]).  Returns out, dx, per layer a dict of the 13
    parameter gradients (``tau`` = sum of the per-window leaves) and ``tau_S`` = sum_w |dL/dtau_w| (the condition scale of dtau)."""
    x = x.detach().double().requires_grad_(True)
    leaves = [{k: v.detach().double().requires_grad_(True) for k, v in p.items() if k != "tau"} for p in params]
    taus = []
    y = x
    for i, (p, lp) in enumerate(zip(params, leaves)):
        pl = plans[i % 2]
        tau_w = torch.full((len(pl["win_len"]),), float(p["tau"].reshape(-1)[0]), dtype=torch.float64, requires_grad=True)
        taus.append(tau_w)
        y = ref_layer(y, pos_table.double()[torch.from_numpy(pl["tok_pos"])], pl["levels"], lp, tau_w)
    out = x + y if residual else y
    out.backward(dy.double())
    grads = []
    for lp, tau_w in zip(leaves, taus):
        g = {k: v.grad for k, v in lp.items()}
        g["tau"] = tau_w.grad.sum()
        g["tau_S"] = float(tau_w.grad.abs().sum())
        grads.append(g)
    return out.detach(), x.grad, grads


def test_reference_equals_oracle():
    """The reference above against oracle.gdmae_oracle.encoder_layer (the padded-window dataflow of the upstream model), two
    chained layers on the two shifts of a synthetic plan, forward and backward, fp64; the second layer's tau is below tau_min."""
    _ref_threads()
    n, d = 301, 32
    plans = [synth_plan_arrays(n, 11), synth_plan_arrays(n, 12)]
    for pl in plans:
        pl["levels"] = _level_index(pl)
    gen = torch.Generator().manual_seed(5)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=gen, dtype=torch.float64) * scale)   # noqa: E731
    params = []
    for tau in (0.6, 0.004):
        params.append({"Win": rnd(3 * d, d, scale=d ** -0.5), "bin": rnd(3 * d, scale=0.1), "tau": torch.tensor([tau], dtype=torch.float64),
                       "Wo": rnd(d, d, scale=d ** -0.5), "bo": rnd(d, scale=0.1), "W1": rnd(2 * d, d, scale=d ** -0.5),
                       "b1": rnd(2 * d, scale=0.1), "W2": rnd(d, 2 * d, scale=(2 * d) ** -0.5), "b2": rnd(d, scale=0.1),
                       "g1": 1 + rnd(d, scale=0.2), "be1": rnd(d, scale=0.1), "g2": 1 + rnd(d, scale=0.2), "be2": rnd(d, scale=0.1)})
    pos_table = rnd(N_POS, d)
    x, dy = rnd(n, d), rnd(n, d)
    for residual in (False, True):
        out, dx, grads = ref_stage(x, dy, pos_table, plans, params, residual)
        # the oracle, same operands
        names = {"Win": "win_attn.self_attn.in_proj_weight", "bin": "win_attn.self_attn.in_proj_bias", "tau": "win_attn.self_attn.tau",
                 "Wo": "win_attn.self_attn.out_proj.weight", "bo": "win_attn.self_attn.out_proj.bias", "W1": "linear1.weight",
                 "b1": "linear1.bias", "W2": "linear2.weight", "b2": "linear2.bias", "g1": "norm1.weight", "be1": "norm1.bias",
                 "g2": "norm2.weight", "be2": "norm2.bias"}
        sd = {}
        for i, p in enumerate(params):
            for k, v in p.items():
                sd[f"l{i}.{names[k]}"] = v.clone().requires_grad_(True)
        xo = x.clone().requires_grad_(True)
        y = xo
        for i in range(len(params)):
            pl = plans[i % 2]
            y = orc.encoder_layer(y, pos_table[torch.from_numpy(pl["tok_pos"])], oracle_part(pl), ORACLE_DROP_INFO, sd, f"l{i}.", NHEAD)
        oo = xo + y if residual else y
        oo.backward(dy)
        rel = lambda a, b: float((a - b).norm() / b.norm())   # noqa: E731
        assert rel(out, oo.detach()) < 1e-12
        assert rel(dx, xo.grad) < 1e-12
        for i, g in enumerate(grads):
            for k in PNAMES:
                ro = sd[f"l{i}.{names[k]}"].grad.reshape(g[k].shape)
                if k == "tau":
                    assert abs(float(g[k] - ro)) <= 1e-12 * max(g["tau_S"], 1e-300) or (float(ro) == 0 and float(g[k]) == 0), (i, k)
                else:
                    assert rel(g[k], ro) < 1e-12, (i, k, rel(g[k], ro))
        assert float(grads[1]["tau"]) == 0.0 and grads[1]["tau_S"] == 0.0       # tau < tau_min: clamped, no gradient
        assert grads[0]["tau_S"] > 0


# ------------------------------------------------------------------------------------------------------------------------
# GPU: the stage against the reference
# ------------------------------------------------------------------------------------------------------------------------
# (d, n, layers, residual, tau, layer paths).  d = 128 runs the 64-row tiles of layer_fused.hip, d = 256 the 32-row tiles;
# n = 65 / 33 end in a partial row tile, 2048 fills the 2048-row padding exactly, 2049 leaves 2047 padding rows; L = 3 is the
# odd parity of the ln2[i & 1] ping-pong; tau = 0.004 < tau_min.
CASES = [
    (128, 1, 1, False, 0.6, (1, 0)),
    (128, 65, 2, True, 0.6, (1, 0)),
    (128, 2048, 3, False, 0.6, (1,)),
    (128, 2049, 2, True, 0.6, (1, 0)),
    (128, 2049, 1, False, 0.004, (1, 0)),
    (128, 5003, 4, True, 0.6, (1,)),
    (256, 1, 2, True, 0.6, (1,)),
    (256, 33, 1, False, 0.6, (1, 0)),
    (256, 2048, 2, True, 0.6, (1,)),
    (256, 2049, 3, True, 0.6, (1, 0)),
    (256, 4411, 4, False, 0.6, (1, 0)),
    (256, 5987, 2, True, 0.004, (1,)),
]
RUNS = [(c, path) for c in CASES for path in c[5]]

# Bounds = 2 x the largest error measured on an MI355X over the runs of one layer path and one tau regime (measured value in the
# comment).  y / dx: relative L2 of the tensor and the worst row (row error / max(row norm, 5 % of the RMS row norm)); weight
# gradients: relative L2; biases, dgamma, dbeta: relative L2 and max element error / max |ref|; tau: |dtau - ref| / S with
# S = sum_w |dL/dtau_w| (dtau is a sum of cancelling per-window terms), the absolute |dtau| where S = 0.
# Path 1 carries the residual stream between the layers in bf16, path 0 in fp32: path 1's errors are the larger.
# At tau = tau_min the logits are cosines / 0.01: the bf16 rounding of the q / k operands (2^-9 relative) moves them by ~0.2 and the
# softmax with them.  The fp64 reference with only that operand rounding injected shows the same errors as the kernels (dx relative
# L2 4.1e-2 at d = 128 and 6.3e-2 at d = 256; kernels 4.1e-2 and 6.8e-2), so those runs have bounds of their own.
BOUNDS = {
    (1, "tau"): {   # 10 runs
        "y.l2": 0.0088,    # 4.39e-03
        "y.row": 0.015,    # 7.68e-03
        "dx.l2": 0.01,     # 5.06e-03
        "dx.row": 0.018,   # 8.87e-03
        "Win.l2": 0.012,   # 6.15e-03
        "bin.l2": 0.012,   # 5.89e-03
        "bin.max": 0.015,  # 7.48e-03
        "tau.S": 0.0089,   # 4.43e-03
        "Wo.l2": 0.012,    # 5.95e-03
        "bo.l2": 0.011,    # 5.57e-03
        "bo.max": 0.013,   # 6.72e-03
        "W1.l2": 0.012,    # 5.98e-03
        "b1.l2": 0.011,    # 5.52e-03
        "b1.max": 0.014,   # 7.00e-03
        "W2.l2": 0.012,    # 5.93e-03
        "b2.l2": 0.011,    # 5.25e-03
        "b2.max": 0.012,   # 6.24e-03
        "g1.l2": 0.01,     # 5.01e-03
        "g1.max": 0.014,   # 6.94e-03
        "be1.l2": 0.011,   # 5.29e-03
        "be1.max": 0.012,  # 6.07e-03
        "g2.l2": 0.011,    # 5.38e-03
        "g2.max": 0.015,   # 7.67e-03
        "be2.l2": 0.0099,  # 4.97e-03
        "be2.max": 0.011,  # 5.51e-03
    },
    (1, "tau_min"): {   # 2 runs
        "y.l2": 0.011,     # 5.36e-03
        "y.row": 0.044,    # 2.22e-02
        "dx.l2": 0.14,     # 6.75e-02
        "dx.row": 0.77,    # 3.87e-01
        "Win.l2": 0.16,    # 7.93e-02
        "bin.l2": 0.15,    # 7.29e-02
        "bin.max": 0.2,    # 9.95e-02
        "tau.S": 0.0,      # 0 (dtau is exactly 0 below tau_min)
        "Wo.l2": 0.12,     # 5.94e-02
        "bo.l2": 0.13,     # 6.52e-02
        "bo.max": 0.1,     # 5.13e-02
        "W1.l2": 0.12,     # 5.87e-02
        "b1.l2": 0.13,     # 6.38e-02
        "b1.max": 0.14,    # 7.24e-02
        "W2.l2": 0.12,     # 5.91e-02
        "b2.l2": 0.13,     # 6.54e-02
        "b2.max": 0.11,    # 5.32e-02
        "g1.l2": 0.11,     # 5.47e-02
        "g1.max": 0.11,    # 5.34e-02
        "be1.l2": 0.13,    # 6.53e-02
        "be1.max": 0.11,   # 5.59e-02
        "g2.l2": 0.12,     # 6.23e-02
        "g2.max": 0.12,    # 6.16e-02
        "be2.l2": 0.12,    # 6.10e-02
        "be2.max": 0.11,   # 5.27e-02
    },
    (0, "tau"): {   # 6 runs
        "y.l2": 0.0037,    # 1.83e-03
        "y.row": 0.0047,   # 2.35e-03
        "dx.l2": 0.0045,   # 2.23e-03
        "dx.row": 0.006,   # 3.02e-03
        "Win.l2": 0.0081,  # 4.05e-03
        "bin.l2": 0.0057,  # 2.83e-03
        "bin.max": 0.0063, # 3.13e-03
        "tau.S": 0.011,    # 5.35e-03
        "Wo.l2": 0.0065,   # 3.26e-03
        "bo.l2": 0.0035,   # 1.77e-03
        "bo.max": 0.0031,  # 1.54e-03
        "W1.l2": 0.0079,   # 3.93e-03
        "b1.l2": 0.0069,   # 3.47e-03
        "b1.max": 0.0089,  # 4.43e-03
        "W2.l2": 0.008,    # 4.02e-03
        "b2.l2": 0.0038,   # 1.88e-03
        "b2.max": 0.003,   # 1.48e-03
        "g1.l2": 0.0036,   # 1.78e-03
        "g1.max": 0.0037,  # 1.84e-03
        "be1.l2": 0.0039,  # 1.96e-03
        "be1.max": 0.0035, # 1.73e-03
        "g2.l2": 0.0038,   # 1.89e-03
        "g2.max": 0.0035,  # 1.74e-03
        "be2.l2": 0.0036,  # 1.82e-03
        "be2.max": 0.0032, # 1.61e-03
    },
    (0, "tau_min"): {   # 1 run
        "y.l2": 0.0097,   # 4.86e-03
        "y.row": 0.041,   # 2.03e-02
        "dx.l2": 0.083,   # 4.14e-02
        "dx.row": 0.29,   # 1.45e-01
        "Win.l2": 0.092,  # 4.59e-02
        "bin.l2": 0.091,  # 4.55e-02
        "bin.max": 0.088, # 4.39e-02
        "tau.S": 0.0,     # 0 (dtau is exactly 0 below tau_min)
        "Wo.l2": 0.027,   # 1.33e-02
        "bo.l2": 0.0026,  # 1.31e-03
        "bo.max": 0.0019, # 9.47e-04
        "W1.l2": 0.013,   # 6.67e-03
        "b1.l2": 0.0088,  # 4.39e-03
        "b1.max": 0.0061, # 3.06e-03
        "W2.l2": 0.012,   # 6.18e-03
        "b2.l2": 0.0014,  # 7.19e-04
        "b2.max": 0.0015, # 7.41e-04
        "g1.l2": 0.01,    # 5.18e-03
        "g1.max": 0.012,  # 6.17e-03
        "be1.l2": 0.0023, # 1.13e-03
        "be1.max": 0.0016, # 8.13e-04
        "g2.l2": 0.011,   # 5.44e-03
        "g2.max": 0.013,  # 6.53e-03
        "be2.l2": 7.6e-08, # 3.79e-08
        "be2.max": 9.6e-08, # 4.82e-08
    },
}


def _case_id(r):
    (d, n, nl, residual, tau, _), path = r
    return f"d{d}-n{n}-L{nl}-{'res' if residual else 'nores'}{'-tausmall' if tau < TAU_MIN else ''}-path{path}"


def _setup(case):
    """CPU-seeded module (so that every call builds the same parameters), plans, pos table, x, dy; reference operands."""
    from torch import nn
    from gdmae_hip.encoder import _plist
    from pcdet.models.model_utils.sst_basic_block import EncoderLayer
    d, n, nl, residual, tau, _ = case
    seed = d * 100003 + n * 7 + nl
    torch.manual_seed(seed)
    block = nn.Module()        # encoder_stage reads block.encoder_list only: any depth, layer k on plan k % 2
    block.encoder_list = nn.ModuleList([EncoderLayer(d, NHEAD, 2 * d, 0.0, "gelu", layer_cfg={"cosine": True, "tau_min": TAU_MIN})
                                        for _ in range(nl)])
    with torch.no_grad():
        for layer in block.encoder_list:
            sa = layer.win_attn.self_attn
            sa.tau.fill_(tau)
            sa.in_proj_bias.normal_(0, 0.1)
            sa.out_proj.bias.normal_(0, 0.1)
            for nm in (layer.norm1, layer.norm2):
                nm.weight.uniform_(0.5, 1.5)
                nm.bias.normal_(0, 0.1)
    plans = [synth_plan_arrays(n, seed + 1), synth_plan_arrays(n, seed + 2)]
    assert n < 2 or not np.array_equal(plans[0]["tok_pos"], plans[1]["tok_pos"])
    assert n < 2 or not (np.array_equal(plans[0]["win_len"], plans[1]["win_len"]) and np.array_equal(plans[0]["csr"], plans[1]["csr"]))
    for pl in plans:
        pl["levels"] = _level_index(pl)
    g = torch.Generator().manual_seed(seed + 3)
    pos_table = torch.rand(N_POS, d, generator=g) * 2 - 1
    x = torch.randn(n, d, generator=g).bfloat16().float()            # bf16-representable
    dy = torch.randn(n, d, generator=g).bfloat16().float()
    params = []
    for layer in block.encoder_list:
        p = {}
        for k, t in zip(PNAMES, _plist(layer)):
            t = t.detach()
            p[k] = t.bfloat16().float() if k in ("Win", "bin", "Wo", "bo", "W1", "b1", "W2", "b2") else t.clone()
        params.append(p)
    return block, plans, pos_table, x, dy, params


_REF = {}


def _reference(case):
    key = case[:5]
    if key not in _REF:
        _ref_threads()
        block, plans, pos_table, x, dy, params = _setup(case)
        _REF[key] = ref_stage(x, dy, pos_table, plans, params, case[3])
    return _REF[key]


def _poison(nbytes, dev):
    """Fill the caching allocator's free memory with NaN: the buffers the stage takes with torch.empty then start as NaN, so a read
    of a row nobody wrote turns the results non-finite."""
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    t = torch.full(((nbytes + 3) // 4,), float("nan"), dtype=torch.float32, device=dev)
    del t


def _run_stage(case, path, dev, steps=2, path_before_backward=None):
    """``steps`` identical steps of the stage under layer path ``path``; ``path_before_backward``: gdmae_encoder_set_layer_path is
    called with it between each forward and its backward."""
    from gdmae_hip import configs, optim
    from gdmae_hip import encoder as genc
    from gdmae_hip import lib as glib
    from torch import nn
    d, n, nl, residual = case[:4]
    block, plans, pos_table, x, dy, _ = _setup(case)
    model = nn.Module()
    model.block = block
    model.to(dev).train()
    opt = optim.FlatAdamOneCycle(model, configs.optimization_cfg(), total_steps=10)
    wplans = [to_window_plan(pl, dev) for pl in plans]
    pos_dev = pos_table.to(dev)
    xdt = torch.bfloat16 if residual else torch.float32      # residual: the bf16 block input of the bench (folded residual on path 1)
    sb, fb, bb = genc._layer_bytes(n, d, 2 * d, NHEAD, 1)
    poison = nl * sb + fb + bb + 4 * n * d * 4 + (64 << 20)
    results = []
    try:
        for _ in range(steps):
            glib.call("gdmae_encoder_set_layer_path", path)
            opt.zero_grad()
            xi = x.to(dev, xdt).requires_grad_(True)
            g = dy.to(dev, xdt)
            _poison(poison, dev)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = genc.encoder_stage([block], xi, pos_dev, wplans, residual=residual)
            assert out.grad_fn.meta[8] == (path == 1), "the stage did not take the requested layer path"
            _poison(poison, dev)
            if path_before_backward is not None:
                glib.call("gdmae_encoder_set_layer_path", path_before_backward)
            out.backward(g)
            torch.cuda.synchronize(dev)
            results.append((out.detach().clone(), xi.grad.detach().clone(), opt.flat_grad.clone(),
                            [{k: t.grad.detach().clone() for k, t in zip(PNAMES, genc._plist(layer))} for layer in block.encoder_list]))
    finally:
        glib.call("gdmae_encoder_set_layer_path", -1)
    return results


def _rel_l2(got, ref):
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def _row_err(got, ref):
    rn = ref.norm(dim=1)
    floor = 0.05 * float(rn.pow(2).mean().sqrt())
    return float(((got - ref).norm(dim=1) / rn.clamp_min(max(floor, 1e-30))).max())


def _max_el(got, ref):
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _errors(results, ref):
    """Every checked quantity of one run: {name: (error, where)}, the worst over the layers for the parameter gradients."""
    out, dx, _, grads = results
    r_out, r_dx, r_grads = ref
    out, dx = out.double().cpu(), dx.double().cpu()
    err = {"y.l2": (_rel_l2(out, r_out), ""), "y.row": (_row_err(out, r_out), ""),
           "dx.l2": (_rel_l2(dx, r_dx), ""), "dx.row": (_row_err(dx, r_dx), "")}

    def put(key, v, where):
        if key not in err or v > err[key][0]:
            err[key] = (v, where)

    for i, (g, rg) in enumerate(zip(grads, r_grads)):
        for k in PNAMES:
            got = g[k].double().cpu().reshape(rg[k].shape)
            if k == "tau":
                # S = 0 (one-token windows only, or tau < tau_min): the absolute value of a gradient that must vanish
                put("tau.S", abs(float(got - rg[k])) / (rg["tau_S"] if rg["tau_S"] > 0 else 1.0), f"layer {i}")
                continue
            put(f"{k}.l2", _rel_l2(got, rg[k]), f"layer {i}")
            if not k.startswith("W"):
                put(f"{k}.max", _max_el(got, rg[k]), f"layer {i}")
    return err


@pytest.mark.gpu
@pytest.mark.parametrize("run", RUNS, ids=[_case_id(r) for r in RUNS])
def test_encoder_stage_matches_fp64_reference(run):
    """Stage output, dx and the 13 gradients of every layer against the fp64 reference, with NaN-poisoned stage buffers (no read of
    an unwritten padding row), twice (bit-identical results)."""
    case, path = run
    dev = torch.device("cuda:0")
    res = _run_stage(case, path, dev)
    ref = _reference(case)
    (o1, dx1, fg1, _), (o2, dx2, fg2, _) = res
    for name, t in (("y", o1), ("dx", dx1), ("flat gradient", fg1)):
        assert bool(torch.isfinite(t).all()), f"{name} holds non-finite values (a read of an unwritten buffer row)"
    assert torch.equal(o1, o2) and torch.equal(dx1, dx2) and torch.equal(fg1, fg2), "two identical steps differ"
    if case[4] < TAU_MIN:
        for i, g in enumerate(res[0][3]):
            assert float(g["tau"].reshape(-1)[0]) == 0.0, f"layer {i}: dtau must be exactly 0 with tau < tau_min"
    err = _errors(res[0], ref)
    print("MEASURE " + json.dumps({"id": _case_id(run), "path": path, "err": {k: v[0] for k, v in err.items()}}))
    bound = BOUNDS[(path, "tau_min" if case[4] <= TAU_MIN else "tau")]
    assert set(bound) == set(err)
    bad = [f"{k} = {v:.3e} > {bound[k]:.1e} ({w})" for k, (v, w) in err.items() if not v <= bound[k]]
    assert not bad, "; ".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("path", [1, 0])
@pytest.mark.parametrize("d,n", [(128, 70), (256, 33)], ids=["d128-n70", "d256-n33"])
def test_backward_follows_the_path_of_its_forward(d, n, path):
    """The layer path belongs to the call: the stage asks gdmae_encoder_stage_fused once, before its forward, and hands the answer
    to both directions in the arguments.  A gdmae_encoder_set_layer_path call between a forward and its backward (forward under 1,
    then 0; and forward under 0, then 1) therefore changes nothing: output, dx and the flat gradient of a two-layer stage are
    bit-equal to the same step without the call.  n = 70 at d = 128 is past one 64-row tile, n = 33 at d = 256 past one 32-row
    tile, both far below the 2048-row padding."""
    dev = torch.device("cuda:0")
    case = (d, n, 2, False, 0.6, ())
    (o0, dx0, fg0, _), = _run_stage(case, path, dev, steps=1)
    (o1, dx1, fg1, _), = _run_stage(case, path, dev, steps=1, path_before_backward=1 - path)
    for name, t in (("y", o0), ("dx", dx0), ("flat gradient", fg0)):
        assert bool(torch.isfinite(t).all()), f"{name} holds non-finite values"
    assert float(fg0.abs().max()) > 0.0
    assert torch.equal(o0, o1), "the output depends on a path set after the forward"
    assert torch.equal(dx0, dx1), "dx depends on a path set between forward and backward"
    assert torch.equal(fg0, fg1), "the flat gradient depends on a path set between forward and backward"
