"""Plain-torch reference of the windowed cosine attention on the kernels' own arguments (``qk``, ``v``, ``tau``, window CSR), the
crafted window lists the attention tests run on, and the float32 CPU evaluation they use as yardstick.  No GPU, no project code.

    q^ = q / max(|q|, 1e-12), k^ likewise, per head;  out = softmax(q^ k^T / clamp(tau, tau_min)) v  inside every window,

rows that no window names stay zero.  ``test_window_attention_reference_cpu.py`` pins ``reference`` to
``oracle.gdmae_oracle.cosine_window_attention``."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

TAU_MIN = float(np.float32(0.01))          # LAYER_CFG.tau_min as the kernels get it: a C float
# the project's two regimes, exactly the clamp (its gradient passes), below the clamp - as the float32 values the kernels read
TAUS = tuple(float(np.float32(t)) for t in (0.2, 0.37, 0.01, 0.004))
TAU_IDS = ("tau0.2", "tau0.37", "taumin", "tau0.004")
SHAPES = ((128, 8), (256, 8), (128, 4))    # (d, H): head dim 16, head dim 32, and one that does not have eight heads

T16_EDGES = [1, 1, 1, 1, 15, 16, 8, 8, 5, 4, 4, 3, 2, 9, 7, 14, 16, 16, 1]    # 19 windows (tail group of 3), groups packing to 16 and 17
T32_EDGES = [16, 17, 31, 32, 1]            # 16 @ T = 32: the shipped boundary [16, 32)
T64_EDGES = [32, 33, 63, 64, 1, 31]        # 32 @ T = 64: the shipped boundary [32, ...), the second 32-row tile all padding

# name -> (max_tokens per level, window lengths per level), levels in the order they are passed
WINDOW_LISTS = {
    "edges": ([16, 32, 64], [T16_EDGES, T32_EDGES, T64_EDGES]),
    "no64-3lv": ([16, 32, 64], [T16_EDGES, T32_EDGES, []]),
    "no64-2lv": ([16, 32], [T16_EDGES, T32_EDGES]),
    "only16-one": ([16], [[1]]),
    "only16-five": ([16], [[3, 16, 1, 9, 12]]),
    "only32": ([32], [[16, 32, 1, 17, 25]]),
    "only64": ([64], [[64]]),
    "16+64": ([16, 64], [[16, 1, 7, 15, 2], [32, 64, 33, 1]]),
    "reordered": ([64, 16, 32], [T64_EDGES, T16_EDGES, T32_EDGES]),
}


def build_windows(name):
    """Host arrays of one crafted window list: ``csr``, ``win_start``, ``win_len`` (int64), ``n_win`` and ``max_tokens`` per level,
    ``n`` token rows, ``unref`` = the rows no window names (row 0, the last row and two in the middle), ``level_of_win``.  Windows
    are stored level by level; a window's tokens are scattered rows of a seeded permutation, ascending inside the window (the
    planner's canonical order)."""
    max_tokens, level_lens = WINDOW_LISTS[name]
    lens = [k for ll in level_lens for k in ll]
    for T, ll in zip(max_tokens, level_lens):
        assert all(1 <= k <= T for k in ll)
    n_ref = sum(lens)
    n = n_ref + 4
    unref = np.array(sorted({0, n // 3, (2 * n) // 3, n - 1}), dtype=np.int64)
    assert len(unref) == 4
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    rows = np.setdiff1d(np.arange(n), unref)
    perm = rows[rng.permutation(n_ref)]
    win_len = np.array(lens, dtype=np.int64)
    win_start = np.concatenate([[0], np.cumsum(win_len)[:-1]]).astype(np.int64)
    csr = np.empty(n_ref, dtype=np.int64)
    for s, k in zip(win_start, win_len):
        csr[s:s + k] = np.sort(perm[s:s + k])
    level_of_win = np.array([lv for lv, ll in enumerate(level_lens) for _ in ll], dtype=np.int64)
    return dict(name=name, n=n, csr=csr, win_start=win_start, win_len=win_len, n_win=[len(ll) for ll in level_lens],
                max_tokens=list(max_tokens), unref=unref, level_of_win=level_of_win)


def plan_fields(w):
    """Per-token fields of the partition (``tok_win``, ``tok_level``, ``tok_slot``, ``n_tok`` per level); -1 on unreferenced rows."""
    tok_win = np.full(w["n"], -1, dtype=np.int64)
    tok_level = np.full(w["n"], -1, dtype=np.int64)
    tok_slot = np.full(w["n"], -1, dtype=np.int64)
    local = [0] * len(w["n_win"])
    n_tok = [0] * len(w["n_win"])
    for i, (s, k) in enumerate(zip(w["win_start"], w["win_len"])):
        lv = int(w["level_of_win"][i])
        toks = w["csr"][s:s + k]
        tok_win[toks] = i
        tok_level[toks] = lv
        tok_slot[toks] = local[lv] * w["max_tokens"][lv] + np.arange(k)
        local[lv] += 1
        n_tok[lv] += int(k)
    return dict(tok_win=tok_win, tok_level=tok_level, tok_slot=tok_slot, n_tok=n_tok)


def reference(qk, v, tau, csr, win_start, win_len, H, tau_min):
    """out (n, d) in the dtype of ``qk``; differentiable in ``qk``, ``v`` and ``tau`` (a tensor).  ``csr`` / ``win_start`` /
    ``win_len``: integer sequences (numpy or lists).  Windows of similar length go through one batched product, padded keys masked with -inf."""
    n, d = v.shape
    dh = d // H
    out = torch.zeros_like(v)
    tau_c = tau.reshape(()).clamp(min=tau_min)
    csr = np.asarray(csr, dtype=np.int64)
    buckets = {}                                     # batch width -> windows; the width is a batching detail, not a level
    for s, k in zip(win_start, win_len):
        buckets.setdefault(next(b for b in (1, 4, 16, 32, 64, 1 << 30) if k <= b), []).append((int(s), int(k)))
    for _, wins in sorted(buckets.items()):
        nw, K = len(wins), max(k for _, k in wins)
        idx = np.zeros((nw, K), dtype=np.int64)      # slots past a window's length read row 0 and are masked below
        live = np.zeros((nw, K), dtype=bool)
        for r, (s, k) in enumerate(wins):
            idx[r, :k] = csr[s:s + k]
            live[r, :k] = True
        idx, live = torch.from_numpy(idx), torch.from_numpy(live)
        heads = lambda t: t[idx.reshape(-1)].view(nw, K, H, dh).transpose(1, 2)       # noqa: E731  (nw, H, K, dh)
        qh = F.normalize(heads(qk[:, :d]), dim=-1, eps=1e-12)
        kh = F.normalize(heads(qk[:, d:]), dim=-1, eps=1e-12)
        logit = (qh @ kh.transpose(-2, -1) / tau_c).masked_fill(~live.view(nw, 1, 1, K), float("-inf"))
        o = (logit.softmax(-1) @ heads(v)).transpose(1, 2).reshape(nw, K, d)
        out = out.index_copy(0, idx[live], o[live])
    return out


def evaluate(dtype, qk, v, dout, tau, w, H, tau_min=TAU_MIN):
    """Reference forward and autograd backward in ``dtype`` (float64, or float32: the yardstick) on the CPU.  Returns
    (out, dqk, dv, dtau), dtau a 0-dim tensor."""
    qk = qk.detach().to("cpu", dtype).requires_grad_(True)
    v = v.detach().to("cpu", dtype).requires_grad_(True)
    t = torch.tensor(float(tau), dtype=dtype, requires_grad=True)
    out = reference(qk, v, t, w["csr"], w["win_start"], w["win_len"], H, tau_min)
    out.backward(dout.detach().to("cpu", dtype))
    return out.detach(), qk.grad, v.grad, t.grad.reshape(())


def make_inputs(name, d, H, bf16):
    """Seeded float32 ``qk`` (n, 2d), ``v`` and ``dout`` (n, d) of one (window list, shape); ``bf16``: bf16-representable."""
    w = build_windows(name)
    g = torch.Generator().manual_seed(zlib.crc32(f"{name}/{d}/{H}".encode()))
    qk = torch.randn(w["n"], 2 * d, generator=g)
    v = torch.randn(w["n"], d, generator=g)
    dout = torch.randn(w["n"], d, generator=g)
    if bf16:
        qk, v, dout = (t.bfloat16().float() for t in (qk, v, dout))
    return w, qk, v, dout


# the zero-norm edit (``edges`` list): per level one window, the first token's q slice of head 0 and the last token's k slice of head 3
ZERO_WINDOWS = {16: 4, 32: 1, 64: 1}       # window index inside its level: the 15-, 17- and 33-token windows
ZERO_Q_HEAD, ZERO_K_HEAD = 0, 3


def zero_norm_edit(w, qk, d, H):
    """Returns (edited qk, [(window index, q row, k row)]) for the windows of ZERO_WINDOWS."""
    dh = d // H
    qk = qk.clone()
    edits = []
    for lv, T in enumerate(w["max_tokens"]):
        wi = sum(w["n_win"][:lv]) + ZERO_WINDOWS[T]
        s, k = int(w["win_start"][wi]), int(w["win_len"][wi])
        assert k >= 2
        rq, rk = int(w["csr"][s]), int(w["csr"][s + k - 1])
        qk[rq, ZERO_Q_HEAD * dh:(ZERO_Q_HEAD + 1) * dh] = 0
        qk[rk, d + ZERO_K_HEAD * dh:d + (ZERO_K_HEAD + 1) * dh] = 0
        edits.append((wi, rq, rk))
    return qk, edits


_CACHE = {}


def cached_reference(name, d, H, tau, bf16, zero_norm=False):
    """(w, qk, v, dout, ref64, y, f32, edits): inputs, the float64 reference (out, dqk, dv, dtau), the yardstick y = per tensor
    max |float32 CPU evaluation - float64| / max |float64| over the referenced rows, and that float32 evaluation.  Computed once per
    key and shared; callers do not modify it."""
    key = (name, d, H, float(tau), bool(bf16), bool(zero_norm))
    if key not in _CACHE:
        torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
        w, qk, v, dout = make_inputs(name, d, H, bf16)
        edits = []
        if zero_norm:
            qk, edits = zero_norm_edit(w, qk, d, H)
        ref = evaluate(torch.float64, qk, v, dout, tau, w, H)
        f32 = evaluate(torch.float32, qk, v, dout, tau, w, H)
        y = tuple(float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300)) for a, b in zip(f32[:3], ref[:3]))
        _CACHE[key] = (w, qk, v, dout, ref, y, f32, edits)
    return _CACHE[key]
