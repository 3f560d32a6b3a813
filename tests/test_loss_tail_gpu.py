"""The loss tail of the pre-training step through the C ABI against tests/loss_tail_reference.py at the kernels' edges:
gdmae_random_mask (csrc/mask.hip), gdmae_group_gt_points and gdmae_chamfer (csrc/chamfer.hip), gdmae_weighted_mean_finish
(csrc/attention.hip) and ops.ChamferLoss on top of them.

Every kernel call is made twice into buffers pre-filled with a sentinel (NaN, -7 for integers) and the two results must be
bit-equal.  Mask, len_keep, point ids and targets are exact.  The Chamfer tolerances are the reference's own derived bounds (operation
counts next to TERM_STEPS / DPRED_STEPS in loss_tail_reference.py) times the factor 2 allowed over them; nothing is measured from the
kernels.  tests/test_loss_tail_reference_cpu.py asserts the input properties these bounds rest on."""
import functools

import numpy as np
import pytest
import torch

import loss_tail_reference as R

pytestmark = pytest.mark.gpu
SLACK = 2.0               # over the derived bound and no more


def dev():
    return torch.device("cuda:0")


def _d(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(dev())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _twice(fn):
    """run a kernel call twice into fresh sentinel-filled buffers: bit-equal results, returned once"""
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y)), "two calls on the same input differ"
    return a


# ----------------------------------------------------------------------------------------------
# gdmae_random_mask
# ----------------------------------------------------------------------------------------------
def _mask_call(noise, off, keep_frac):
    from gdmae_hip import lib as L
    n_d, off_d = _d(noise), _d(off)

    def run():
        mask = torch.full((max(len(noise), 1),), float("nan"), device=dev())
        lk = torch.full((len(off) - 1,), -7, dtype=torch.int32, device=dev())
        L.call("gdmae_random_mask", L.ptr(n_d), L.ptr(off_d), len(off) - 1, float(keep_frac), L.ptr(mask), L.ptr(lk), L.stream())
        return mask[:len(noise)].cpu().numpy(), lk.cpu().numpy()
    return _twice(run)


@pytest.mark.parametrize("launch", list(R.MASK_LAUNCHES))
@pytest.mark.parametrize("kind", R.MASK_KINDS)
def test_random_mask(launch, kind):
    """Cached and uncached body (L on both sides of 16 * 1024, and 40000), samples of unequal length and an empty one in one launch,
    distinct / coarse / all-equal / mixed-sign noise.  No input holds -0.0: the kernel's key orders it before +0.0, a stable argsort
    does not, and torch.rand never produces it."""
    lengths = R.MASK_LAUNCHES[launch]
    noise, off = R.mask_noise(kind, lengths)
    for kf in R.MASK_KEEP_FRACS:
        mask, lk = _mask_call(noise, off, kf)
        exp, lens = R.random_mask(noise, off, kf)
        assert lk.tolist() == lens, (kf, lk.tolist(), lens)
        bad = np.flatnonzero(_bits(mask) != _bits(exp))
        assert bad.size == 0, (kf, bad[:8], np.searchsorted(off, bad[:8], side="right") - 1)
    if launch == "hundred":
        assert _mask_call(noise, off, 0.71)[1][0] == int(100 * 0.71)
        assert _mask_call(noise, off, 0.57)[1][0] == int(100 * 0.57) == 56         # 100 * 0.57 is below 57 in doubles


# ----------------------------------------------------------------------------------------------
# gdmae_group_gt_points
# ----------------------------------------------------------------------------------------------
def _group_call(sc, n_cols, K, want_index=True):
    from gdmae_hip import lib as L
    pts, off, csr, vc = _d(sc["points"]), _d(sc["pt_off"]), _d(sc["csr"]), _d(sc["voxel_coords"])
    M = sc["M"]

    def run():
        gt = torch.full((M, K, 3), float("nan"), device=dev())
        gi = torch.full((M, K), -7, dtype=torch.int32, device=dev()) if want_index else None
        L.call("gdmae_group_gt_points", L.ptr(pts), n_cols, L.ptr(off), L.ptr(csr), L.ptr(vc), M, K, L.host_f32(sc["lo"]),
               L.host_f32(sc["vs"]), L.ptr(gt), L.ptr(gi), L.stream())
        return (gt.cpu().numpy(), gi.cpu().numpy()) if want_index else (gt.cpu().numpy(),)
    return _twice(run)


def _check_group(sc, n_cols, K):
    gt, gi = _group_call(sc, n_cols, K)
    gt_ref, gi_ref = R.group_gt(sc["points"], n_cols, sc["pt_off"], sc["csr"], sc["voxel_coords"], K, sc["lo"], sc["vs"])
    assert np.array_equal(gi, gi_ref), np.argwhere(gi != gi_ref)[:4]
    bad = np.argwhere(_bits(gt) != _bits(gt_ref))
    assert bad.size == 0, (bad[:4], np.diff(sc["pt_off"])[bad[:4, 0]])
    (gt_only,) = _group_call(sc, n_cols, K, want_index=False)              # gidx = NULL
    assert np.array_equal(_bits(gt_only), _bits(gt_ref))


@pytest.mark.parametrize("n_cols", [4, 5, 6])
@pytest.mark.parametrize("K", [64, 16, 100])
def test_group_gt_points(K, n_cols):
    """cnt = 1, 2, K - 1, K, K + 1, 5 K, 63, 64, 65 with csr a random permutation of each pillar's list; K = 16 leaves lanes idle,
    K = 100 gives lanes two slots; negative range origin, cell (0, 0) and the last cell of a 470 x 470 grid, batch indices 0..2."""
    _check_group(R.gt_scene(K, n_cols), n_cols, K)


def test_group_gt_points_past_the_grid_cap():
    _check_group(R.gt_scene_many(), 4, 64)


# ----------------------------------------------------------------------------------------------
# gdmae_chamfer + gdmae_weighted_mean_finish
# ----------------------------------------------------------------------------------------------
def _chamfer_call(pred, gt, w):
    from gdmae_hip import lib as L
    M, P1, _ = pred.shape
    p_d, g_d, w_d = _d(pred), _d(gt), _d(w)

    def run():
        term = torch.full((M,), float("nan"), device=dev())
        dpred = torch.full((M, P1, 3), float("nan"), device=dev())
        L.call("gdmae_chamfer", L.ptr(p_d), L.ptr(g_d), L.ptr(w_d), M, P1, gt.shape[1], L.ptr(term), L.ptr(dpred), L.stream())
        return term.cpu().numpy(), dpred.cpu().numpy()
    return _twice(run)


def _finish_call(term, w, offset=False):
    """offset: both arrays are passed as views one float into their buffers - no 16-byte alignment, the kernel's scalar path"""
    from gdmae_hip import lib as L
    n = len(term)
    o = 1 if offset else 0
    t_d, w_d = torch.zeros(n + o, device=dev()), torch.zeros(n + o, device=dev())
    t_d[o:] = _d(term)
    w_d[o:] = _d(w)
    tv, wv = t_d[o:], w_d[o:]
    assert (tv.data_ptr() % 16 == 4 and wv.data_ptr() % 16 == 4) if offset else (tv.data_ptr() % 16 == 0 and wv.data_ptr() % 16 == 0)

    def run():
        out = torch.full((2,), float("nan"), device=dev())
        L.call("gdmae_weighted_mean_finish", L.ptr(tv), L.ptr(wv), n, L.ptr(out), L.stream())
        return (out.cpu().numpy(),)
    return _twice(run)[0]


def _check_finish(out, term32, w):
    loss, inv, loss_bound, inv_rel = R.mean_finish(term32, w)
    assert abs(float(out[1]) - inv) <= inv_rel * inv, (float(out[1]), inv)
    assert abs(float(out[0]) - loss) <= loss_bound, (float(out[0]), loss, loss_bound)


def _check_chamfer_dyadic(pred, gt, w, what, ref=None):
    """term and dpred within the reference's bound; arg-minima agree without exception (exact distances: a different minimiser
    shows as a gradient error far outside the bound); zero-weight pillars exactly 0; then the finish on the kernel's own terms."""
    ref = ref if ref is not None else R.chamfer(pred, gt, w)
    term, dpred = _chamfer_call(pred, gt, w)
    assert np.isfinite(term).all() and np.isfinite(dpred).all(), f"{what}: unwritten output"
    z = w == 0
    assert np.all(_bits(term[z]) == 0) and np.all(_bits(dpred[z]) == 0), f"{what}: zero-weight pillars must be exactly +0"
    et = np.abs(term - ref.term)
    bad = np.flatnonzero(et > SLACK * ref.term_bound)
    assert bad.size == 0, (what, "term", bad[:6], et[bad[:6]], ref.term_bound[bad[:6]])
    ed = np.abs(dpred - ref.dpred)
    bad = np.argwhere(ed > SLACK * ref.dpred_bound)
    assert bad.size == 0, (what, "dpred", len(bad), bad[:6].tolist(), ed[tuple(bad[:6].T)], ref.dpred_bound[tuple(bad[:6].T)])
    out = _finish_call(term, w)
    _check_finish(out, term, w)
    # the chain kernel terms -> loss against the float64 loss: the terms' bounds, scaled, on top of the finish's own
    _, inv, fb, _ = R.mean_finish(term, w)
    assert abs(float(out[0]) - ref.loss) <= SLACK * ref.term_bound.sum() * inv + fb + R.U * abs(ref.loss), what
    return term, dpred, out


@functools.lru_cache(maxsize=4)
def _inputs(kind, M, P1, P2):
    pred, gt = R.chamfer_dyadic(kind, M, P1, P2)
    w = R.chamfer_weights(M, seed=1, runs=M == R.CHAMFER_M_MANY)
    return pred, gt, w


@functools.lru_cache(maxsize=2)
def _inputs_ref(kind, M, P1, P2):
    """the reference of a standard input set: computed once, shared, never modified"""
    return R.chamfer(*_inputs(kind, M, P1, P2))


@pytest.mark.parametrize("kind", ["fine", "coarse"])
@pytest.mark.parametrize("P1,P2", R.CHAMFER_FAST + R.CHAMFER_GENERIC)
def test_chamfer_dyadic(P1, P2, kind):
    """(16, *) is the fast path (row minima folded over lane quads: P2 = 1, 2, 3 leave quads partly or wholly empty), the others the
    generic kernel (P1 = 1, 15 / 17 around the switch, 64 = the declared maximum).  "coarse" holds exact ties between distinct points,
    duplicated predictions / ground-truth points, an all-equal ground truth and d = +0; weights are 0, 1, 0.5, 2^-10 and 3."""
    pred, gt, w = _inputs(kind, R.CHAMFER_M, P1, P2)
    _check_chamfer_dyadic(pred, gt, w, (kind, P1, P2), _inputs_ref(kind, R.CHAMFER_M, P1, P2))


@pytest.mark.parametrize("kind", ["fine", "coarse"])
@pytest.mark.parametrize("P1,P2", R.CHAMFER_MANY)
def test_chamfer_grid_stride_loop(P1, P2, kind):
    """M = 4 * 8192 + 5: the launch is capped at 8192 workgroups, waves 0 - 4 walk a second pillar over the same LDS rows: live after
    live, zero-weight after live, live after the early `continue` of a zero-weight one."""
    pred, gt, w = _inputs(kind, R.CHAMFER_M_MANY, P1, P2)
    _check_chamfer_dyadic(pred, gt, w, (kind, P1, P2, "many"), _inputs_ref(kind, R.CHAMFER_M_MANY, P1, P2))


@pytest.mark.parametrize("P1,P2", [(16, 64), (3, 5)])
def test_chamfer_all_zero_and_single_weight(P1, P2):
    pred, gt, _ = _inputs("coarse", R.CHAMFER_M, P1, P2)
    w0 = np.zeros(R.CHAMFER_M, np.float32)
    term, dpred = _chamfer_call(pred, gt, w0)
    assert np.all(_bits(term) == 0) and np.all(_bits(dpred) == 0)
    out = _finish_call(term, w0)
    assert _bits(out).tolist() == [0, 0], "loss == 0 and inv == 0 when no weight is positive"
    for m, v in ((0, 3.0), (R.CHAMFER_M - 1, 2.0 ** -10), (77, 0.5)):          # exactly one positive weight
        w1 = w0.copy()
        w1[m] = v
        term, dpred, out = _check_chamfer_dyadic(pred, gt, w1, (P1, P2, "single", m))
        assert np.count_nonzero(term) <= 1 and np.all(dpred[np.arange(R.CHAMFER_M) != m] == 0)
        assert float(out[1]) == np.float32(1.0) / np.float32(v)


@pytest.mark.parametrize("P1,P2", R.CHAMFER_RANDOM)
def test_chamfer_random(P1, P2):
    """randn inputs of test_chamfer_matches_oracle (same seed), against the float64 reference: loss within 1e-5 relative, gradient
    within 1e-5 of the largest reference gradient outside the near ties (relative gap below 1e-5 between the two best distances;
    at most 0.1 % of rows and of columns, asserted on the CPU: this seed has none)."""
    pred, gt, w = R.chamfer_random(777, P1, P2)
    ref = R.chamfer(pred, gt, w)
    term, dpred = _chamfer_call(pred, gt, w)
    out = _finish_call(term, w)
    assert abs(float(out[0]) - ref.loss) <= 1e-5 * abs(ref.loss)
    rows, cols, skip = R.near_tie_points(ref, 1e-5)
    assert rows.sum() <= 1e-3 * rows.size and cols.sum() <= 1e-3 * cols.size
    g, g_ref = dpred.astype(np.float64) * float(out[1]), ref.dpred * ref.inv
    err = np.abs(g - g_ref).max(-1)
    assert err[~skip].max() <= 1e-5 * np.abs(g_ref).max(), (err[~skip].max(), np.abs(g_ref).max())
    assert np.all(_bits(term[w == 0]) == 0) and np.all(_bits(dpred[w == 0]) == 0)


@functools.lru_cache(maxsize=None)
def _finish_inputs():
    return R.finish_inputs()


@pytest.mark.parametrize("n", R.FINISH_N)
def test_weighted_mean_finish(n):
    """n around the 16-byte vector width (1, 3, 4, 5) and the 4 x 1024-vector sweep (4095, 4096, 4097 floats and 16384 + 5), on the
    reference's own terms rounded to fp32; once more through pointers that are not 16-byte aligned (scalar path)."""
    term, w = _finish_inputs()
    term, w = term[:n], w[:n]
    _check_finish(_finish_call(term, w), term, w)
    _check_finish(_finish_call(term, w, offset=True), term, w)
    z = _finish_call(term, np.zeros(n, np.float32), offset=n % 2 == 1)
    assert _bits(z).tolist() == [0, 0]


# ----------------------------------------------------------------------------------------------
# ops.ChamferLoss
# ----------------------------------------------------------------------------------------------
def _bf16_ordinal(t):
    """bf16 values as integers whose difference counts representable values in between"""
    b = t.detach().cpu().contiguous().view(torch.int16).numpy().astype(np.int64) & 0xFFFF
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def test_chamfer_loss_op_scaling_paths():
    """Upstream gradient 3 through ops.ChamferLoss: fp32 (scaled), bf16 (scaled and cast in one pass) and the lazy hand-over."""
    from gdmae_hip import ops
    P1, P2 = 16, 64
    pred, gt, w = _inputs("coarse", R.CHAMFER_M, P1, P2)          # multiples of 1 / 2 in [-2, 2]: exact in bf16 too
    ref = _inputs_ref("coarse", R.CHAMFER_M, P1, P2)
    assert R.weights_sum_exact(w)
    _, dpred_k = _chamfer_call(pred, gt, w)
    term_k, _ = _chamfer_call(pred, gt, w)
    inv_k = np.float32(_finish_call(term_k, w)[1])
    gt_d, w_d = _d(gt), _d(w)
    # fp32: dpred * (3 * inv).  inv: one rounding (the weights' sum is exact), 3 * inv one, the product one -> 3 u relative
    pg = _d(pred).requires_grad_(True)
    loss = ops.ChamferLoss.apply(pg, gt_d, w_d)
    (loss * 3).backward()
    assert abs(float(loss.detach()) - ref.loss) <= SLACK * ref.term_bound.sum() * ref.inv + R.mean_finish(term_k, w)[2] + R.U * abs(ref.loss)
    g_ref = ref.dpred * (3 * ref.inv)
    bound = SLACK * ref.dpred_bound * (3 * ref.inv) + 3 * R.U * np.abs(g_ref)
    assert pg.grad.dtype == torch.float32
    assert np.all(np.abs(pg.grad.cpu().numpy() - g_ref) <= bound)
    # bf16: the returned gradient is bf16(dpred * (3 * inv)) of the kernel's own dpred, to one bf16 ulp
    pb = _d(pred, torch.bfloat16).requires_grad_(True)
    assert torch.equal(pb.detach().float().cpu(), torch.from_numpy(pred))
    (ops.ChamferLoss.apply(pb, gt_d, w_d) * 3).backward()
    assert pb.grad.dtype == torch.bfloat16
    want = (torch.from_numpy(dpred_k) * (np.float32(3.0) * inv_k)).to(torch.bfloat16)
    assert np.abs(_bf16_ordinal(pb.grad) - _bf16_ordinal(want)).max() <= 1
    # lazy: the unscaled dpred, the two scalars on the side, keyed by the gradient tensor's address
    seen = []
    leaf = _d(pred).requires_grad_(True)
    mid = leaf * 1.0
    mid.register_hook(lambda g: seen.append((g.data_ptr(), g.detach().clone())))
    try:
        ops.LAZY_SCALE.clear()
        (ops.ChamferLoss.apply(mid, gt_d, w_d, True) * 3).backward()
        assert len(seen) == 1 and np.array_equal(_bits(seen[0][1].cpu().numpy()), _bits(dpred_k)), "unscaled dpred"
        assert list(ops.LAZY_SCALE) == [seen[0][0]]
        up, inv = ops.LAZY_SCALE[seen[0][0]]
        assert float(up) == 3.0 and np.float32(float(inv)) == inv_k
        assert abs(float(inv) - ref.inv) <= 2 * R.U * ref.inv
    finally:
        ops.LAZY_SCALE.clear()


# ----------------------------------------------------------------------------------------------
# chained: crafted points -> targets -> Chamfer
# ----------------------------------------------------------------------------------------------
def test_group_gt_then_chamfer_chain():
    sc = R.chain_scene()
    gt_k, _ = _group_call(sc, 4, 64)
    gt_ref, _ = R.group_gt(sc["points"], 4, sc["pt_off"], sc["csr"], sc["voxel_coords"], 64, sc["lo"], sc["vs"])
    assert np.array_equal(_bits(gt_k), _bits(gt_ref))
    pred = gt_k[:, :16] + sc["perturb"]                           # multiples of 1 / 64: exact
    _check_chamfer_dyadic(np.ascontiguousarray(pred), gt_k, sc["w"], "chain")
