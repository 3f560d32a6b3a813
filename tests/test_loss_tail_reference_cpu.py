"""Pins tests/loss_tail_reference.py (CPU only): the references against ``oracle/`` and the goldens, and the properties of the input
generators that the tolerances of tests/test_loss_tail_gpu.py rest on, for every seed and shape the GPU tests use."""
import numpy as np
import pytest
import torch

import loss_tail_reference as R
from helpers import load_case
from oracle import gdmae_oracle as orc
from oracle import thirdparty as tp


# ----------------------------------------------------------------------------------------------
# mask
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("launch", list(R.MASK_LAUNCHES))
@pytest.mark.parametrize("kind", R.MASK_KINDS)
def test_random_mask_equals_oracle(launch, kind):
    lengths = R.MASK_LAUNCHES[launch]
    noise, off = R.mask_noise(kind, lengths)
    assert not np.any(np.signbit(noise) & (noise == 0)), "no -0.0 in any input"
    assert np.isfinite(noise).all()
    for kf in R.MASK_KEEP_FRACS:
        mask, lens = R.random_mask(noise, off, kf)
        for b, L in enumerate(lengths):
            exp = orc.random_masking(L, 1 - kf, torch.from_numpy(noise[off[b]:off[b + 1]]))
            # the oracle takes the ratio: 1 - (1 - kf) may differ from kf in the last bit, so its own len_keep is compared only where
            # both agree; the mask is compared through the reference's len_keep smallest of the oracle's stable order
            ids = torch.argsort(torch.from_numpy(noise[off[b]:off[b + 1]]), stable=True).numpy()
            want = np.ones(L, np.float32)
            want[ids[:max(0, min(L, lens[b]))]] = 0
            assert np.array_equal(mask[off[b]:off[b + 1]], want), (launch, kind, kf, b)
            if int(L * (1 - (1 - kf))) == lens[b]:
                assert np.array_equal(mask[off[b]:off[b + 1]], exp.numpy()), (launch, kind, kf, b)
            assert lens[b] == int(L * kf)


def test_random_mask_equals_mae_mask_over_a_batch():
    lengths = R.MASK_LAUNCHES["hundred"]
    noise, off = R.mask_noise("coarse", lengths)
    vc = torch.from_numpy(np.repeat(np.arange(len(lengths)), lengths)).view(-1, 1)
    for ratio in (0.75, 0.5, 0.25):                     # dyadic: 1 - ratio is exact, the oracle's len_keep is the reference's
        mask, _ = R.random_mask(noise, off, 1 - ratio)
        assert np.array_equal(mask, orc.mae_mask(vc, len(lengths), ratio, torch.from_numpy(noise)).numpy())


def test_mask_generators_keep_their_properties():
    assert 100 * 0.71 == 71.0                                 # no truncation here: the product rounds to 71.0 in doubles
    assert 100 * 0.57 < 57 and int(100 * 0.57) == 56 and int(40000 * 0.57) == 22799      # the truncation cases
    for launch, lengths in R.MASK_LAUNCHES.items():
        noise, off = R.mask_noise("distinct", lengths)
        for b, L in enumerate(lengths):
            assert len(np.unique(noise[off[b]:off[b + 1]])) == L
        if launch == "hundred":
            assert R.random_mask(noise, off, 0.71)[1][0] == int(100 * 0.71) == 71
            assert R.random_mask(noise, off, 0.57)[1][0] == 56
        small = [b for b, L in enumerate(lengths) if 0 < L < 2048]
        lens = R.random_mask(noise, off, 1.0 / 2048)[1]
        assert small and all(lens[b] == 0 for b in small)
        # coarse noise: the threshold value has copies on both sides of the keep boundary, in different 1024-element rounds
        noise, off = R.mask_noise("coarse", lengths)
        for b, L in enumerate(lengths):
            if L < 4096:
                continue
            v = noise[off[b]:off[b + 1]]
            for kf in (0.25, 0.71, 1 - 0.85, 0.57):
                k = int(L * kf)
                thr = np.sort(v, kind="stable")[k - 1]
                eq = np.flatnonzero(v == thr)
                kept = k - int((v < thr).sum())
                assert 0 < kept < len(eq), "ties straddle the keep boundary"
                assert eq[0] // 1024 != eq[-1] // 1024, "ties cross rounds"
        noise, _ = R.mask_noise("signed", lengths)
        assert (noise < 0).any() and (noise > 0).any()


def test_random_mask_equals_golden():
    z, _, _, _ = load_case("kitti_b2")
    B = int(z["batch_size"])
    off = np.searchsorted(z["voxel_coords"][:, 0], np.arange(B + 1))
    mask, lens = R.random_mask(z["noise"], off, 1 - float(z["mask_ratio"]))
    assert np.array_equal(mask.astype(np.uint8), z["mask"])
    assert lens == [int((off[b + 1] - off[b]) * (1 - float(z["mask_ratio"]))) for b in range(B)]


# ----------------------------------------------------------------------------------------------
# reconstruction targets
# ----------------------------------------------------------------------------------------------
def test_group_gt_equals_oracle_on_golden():
    z, ds, _, _ = load_case("kitti_b2")
    pts = torch.from_numpy(z["points"])
    keep, coords = orc.point_coords(pts, ds.point_cloud_range, ds.voxel_size, ds.grid_size)
    vc, inv, rank, cnt = orc.unique_pillars(coords, ds.grid_size)
    kept = pts[keep]
    N = len(inv)
    csr = torch.argsort(inv * (N + 1) + torch.arange(N)).numpy()              # by (pillar, ascending point index)
    pt_off = np.concatenate([[0], np.cumsum(cnt.numpy())])
    gt, gidx = R.group_gt(kept.numpy(), kept.shape[1], pt_off, csr, vc.numpy(), 64, ds.point_cloud_range[:3], ds.voxel_size[:3])
    gt_ref, gi_ref = orc.group_gt_points(kept[:, 1:4], inv, rank, cnt, 64)
    cen = orc.voxel_centers(vc[:, 1:], ds.voxel_size, ds.point_cloud_range)
    assert np.array_equal(gidx, z["gt_group_inds"]) and np.array_equal(gidx, gi_ref.numpy())
    assert np.array_equal(gt.view(np.uint32), (gt_ref - cen.unsqueeze(1)).numpy().view(np.uint32)), "bit for bit"


@pytest.mark.parametrize("K", [64, 16, 100])
def test_gt_scene_is_what_it_says(K):
    sc = R.gt_scene(K, 4)
    cnt = np.diff(sc["pt_off"])
    assert set(cnt) == {1, 2, K - 1, K, K + 1, 5 * K, 63, 64, 65} and cnt.min() >= 1 and 200 <= sc["M"] <= 400
    vc = sc["voxel_coords"]
    assert vc[0].tolist() == [0, 0, 0, 0] and vc[-1].tolist() == [2, 0, R.GT_GRID - 1, R.GT_GRID - 1]
    assert len({tuple(r) for r in vc.tolist()}) == sc["M"] and set(vc[:, 0]) == {0, 1, 2}
    # csr: each pillar's list holds exactly its points, and is not ascending (first-by-ascending-index would show)
    owner = np.empty(len(sc["csr"]), np.int64)
    unsorted = 0
    for p in range(sc["M"]):
        seg = sc["csr"][sc["pt_off"][p]:sc["pt_off"][p + 1]]
        owner[seg] = p
        unsorted += int(np.any(np.diff(seg) < 0))
        assert np.all(sc["points"][seg, 0] == vc[p, 0])
    assert np.array_equal(np.sort(sc["csr"]), np.arange(len(owner))) and unsorted > sc["M"] // 2
    gt, gidx = R.group_gt(sc["points"], 4, sc["pt_off"], sc["csr"], vc, K, sc["lo"], sc["vs"])
    assert np.abs(gt[:, :, :2]).max() <= 0.17 and np.abs(gt[:, :, 2]).max() <= 3.01       # inside the voxel
    for p in (0, 1, 2, 3, 4, 5):                        # slot rule, by hand
        seg = sc["csr"][sc["pt_off"][p]:sc["pt_off"][p + 1]]
        assert gidx[p].tolist() == [int(seg[k if k < len(seg) else k % len(seg)]) for k in range(K)]


def test_gt_scene_many_is_past_the_grid_cap():
    sc = R.gt_scene_many()
    cnt = np.diff(sc["pt_off"])
    assert sc["M"] == 4 * 8192 + 5 and set(cnt) == {1, 2, 3}


# ----------------------------------------------------------------------------------------------
# Chamfer
# ----------------------------------------------------------------------------------------------
def _torch_chamfer(pred, gt, w):
    pr = torch.from_numpy(pred).double().requires_grad_(True)
    wt = torch.from_numpy(np.asarray(w)).double()
    loss, _ = tp.chamfer_distance(pr, torch.from_numpy(gt).double(), wt)
    loss.backward()
    return float(loss.detach()), pr.grad.numpy()


@pytest.mark.parametrize("P1,P2", R.CHAMFER_RANDOM)
def test_chamfer_equals_oracle_fp64_on_tie_free_inputs(P1, P2):
    pred, gt, w = R.chamfer_random(777, P1, P2)
    ref = R.chamfer(pred, gt, w)
    loss, grad = _torch_chamfer(pred, gt, w)
    assert abs(ref.loss - loss) <= 1e-12 * abs(loss)
    # pillar 5 carries the one exact tie (two equal ground-truth points: the same gradient whichever is taken)
    assert np.abs(ref.dpred * ref.inv - grad).max() <= 1e-12 * np.abs(grad).max()
    # near ties of the random set: under the cap of 0.1 % of rows and of columns.  With the gap taken relative to the second-best
    # distance this seed has none in either shape (smallest column gaps 2.6e-5 and 2.3e-5): the GPU gradient check leaves nothing out
    rows, cols, pts = R.near_tie_points(ref, 1e-5)
    assert rows.sum() <= 1e-3 * rows.size and cols.sum() <= 1e-3 * cols.size
    assert (int(rows.sum()), int(cols.sum())) == (0, 0)
    assert pts.sum() <= rows.sum() + 2 * cols.sum()


@pytest.mark.parametrize("P1,P2", R.CHAMFER_FAST + R.CHAMFER_GENERIC)
@pytest.mark.parametrize("kind", ["fine", "coarse"])
def test_chamfer_on_tie_sets_loss_agrees_and_gradient_where_unique(kind, P1, P2):
    pred, gt = R.chamfer_dyadic(kind, R.CHAMFER_M, P1, P2)
    w = R.chamfer_weights(R.CHAMFER_M, seed=1)
    ref = R.chamfer(pred, gt, w)
    loss, grad = _torch_chamfer(pred, gt, w)
    assert abs(ref.loss - loss) <= 1e-12 * abs(loss)
    # torch documents no tie rule: compare the gradient of the pillars in which every minimiser is unique
    uniq = (ref.row_gap > 0).all(1) & (ref.col_gap > 0).all(1)
    if P1 > 1 and P2 > 1 and kind == "fine":
        assert uniq.sum() > 0
    assert np.abs(ref.dpred * ref.inv - grad)[uniq].max(initial=0.0) <= 1e-12 * np.abs(grad).max()
    # zero-weight pillars: exactly nothing
    assert np.all(ref.term[w == 0] == 0) and np.all(ref.dpred[w == 0] == 0)


@pytest.mark.parametrize("M,P1,P2", [(R.CHAMFER_M, a, b) for a, b in R.CHAMFER_FAST + R.CHAMFER_GENERIC]
                         + [(R.CHAMFER_M_MANY, a, b) for a, b in R.CHAMFER_MANY])
def test_dyadic_sets_are_exact_in_fp32(M, P1, P2):
    many = M == R.CHAMFER_M_MANY
    for kind in ("fine", "coarse"):
        pred, gt = R.chamfer_dyadic(kind, M, P1, P2)
        step, lim = (64, 4) if kind == "fine" else (2, 2)
        for a in (pred, gt):
            assert a.dtype == np.float32 and np.abs(a).max() <= lim and np.array_equal(a * step, np.round(a * step))
        # every squared distance evaluated in fp32 (any order of the three products) equals the float64 one
        s = slice(0, 64)
        d32 = ((pred[s, :, None, :] - gt[s, None, :, :]) ** 2).astype(np.float32)
        d32 = (d32[..., 0] + d32[..., 1]) + d32[..., 2]
        d64 = ((pred[s, :, None, :].astype(np.float64) - gt[s, None, :, :].astype(np.float64)) ** 2).sum(-1)
        assert d32.dtype == np.float32 and np.array_equal(d32.astype(np.float64), d64)
        assert (4 * 64) ** 2 * 3 * 4 < 2 ** 24                 # (2 * lim * step)^2 * 3 fits the significand
    w = R.chamfer_weights(M, seed=1, runs=many)
    assert set(np.unique(w)) <= set(R.WEIGHTS.tolist()) and R.weights_sum_exact(w) and np.all(w[:R.N_PLANTED] > 0)
    assert len(set(np.unique(w))) == 5
    if many:                                                   # a wave's second pillar exists; zero-weight runs sit between live ones
        z = w == 0
        flips = np.flatnonzero(np.diff(z.astype(np.int8)))
        stride = 4 * 8192                                      # pillar m and m + stride share a wave
        assert len(flips) > 1000 and z[stride:].size == 5
        assert (z[:5].tolist(), z[stride:].tolist()) == ([False] * 4 + [True], [False] * 3 + [True, False])


@pytest.mark.parametrize("P1,P2", [(16, 64), (16, 3), (3, 5), (17, 64), (64, 64)])
def test_coarse_set_has_ties_of_each_kind(P1, P2):
    """The tie sets have teeth: a reference with the opposite tie rule (highest index) gives another gradient, through rows and through
    columns, through ties between distinct points and through each planted pillar."""
    pred, gt = R.chamfer_dyadic("coarse", R.CHAMFER_M, P1, P2)
    w = R.chamfer_weights(R.CHAMFER_M, seed=1)
    lo, hi = R.chamfer(pred, gt, w), R.chamfer(pred, gt, w, tie="highest")
    assert np.allclose(lo.term, hi.term, rtol=1e-15)            # the loss does not depend on the rule
    live = w > 0
    assert (lo.row_arg != hi.row_arg)[live].any() and (lo.col_arg != hi.col_arg)[live].any()
    changed = np.abs(lo.dpred - hi.dpred).max((1, 2)) > 0
    assert changed[live].sum() > live.sum() // 4 and not changed[~live].any()
    # ... and by far more than the GPU tests allow: a kernel with the other rule fails test_chamfer_dyadic[coarse]
    assert (np.abs(lo.dpred - hi.dpred) > 100 * lo.dpred_bound).sum() > live.sum()
    # ties between DISTINCT points at equal distance: the two candidate minimisers are different points
    m, i = np.nonzero((lo.row_arg != hi.row_arg) & live[:, None])
    assert np.any(np.abs(gt[m, lo.row_arg[m, i]] - gt[m, hi.row_arg[m, i]]).sum(-1) > 0)
    m, j = np.nonzero((lo.col_arg != hi.col_arg) & live[:, None])
    assert np.any(np.abs(pred[m, lo.col_arg[m, j]] - pred[m, hi.col_arg[m, j]]).sum(-1) > 0)
    # planted pillars
    assert np.array_equal(pred[0, P1 // 2:2 * (P1 // 2)], pred[0, :P1 // 2])                      # duplicated predictions: column ties
    assert (lo.col_arg[0] != hi.col_arg[0]).any() and changed[0]
    assert (lo.row_arg[1] != hi.row_arg[1]).any()                                         # duplicated ground truth: row ties
    assert np.all(gt[2] == gt[2, 0]) and np.all(lo.row_arg[2] == 0) and np.all(hi.row_arg[2] == P2 - 1)
    n = min(P1, P2)
    d3 = ((pred[3, :n].astype(np.float64) - gt[3, :n]) ** 2).sum(-1)
    assert np.all(d3 == 0) and not np.any(np.signbit(d3))                                 # d == +0


def test_error_bounds_cover_an_fp32_evaluation():
    """The derived bounds hold for a plain fp32 evaluation of the same formula on the CPU (sequential sums, the worst association)."""
    P1, P2 = 16, 64
    pred, gt = R.chamfer_dyadic("fine", 64, P1, P2)
    w = R.chamfer_weights(64, seed=1)
    ref = R.chamfer(pred, gt, w)
    f = np.float32
    for m in range(64):
        d = ((pred[m, :, None, :] - gt[m, None, :, :]) ** 2).sum(-1, dtype=f)
        sx = f(0)
        for v in d.min(1):
            sx = f(sx + v)
        sy = f(0)
        for v in d.min(0):
            sy = f(sy + v)
        t = f(f(f(w[m]) / f(P1)) * sx) + f(f(f(w[m]) / f(P2)) * sy)
        assert abs(float(t) - ref.term[m]) <= ref.term_bound[m]
    assert np.all(ref.dpred_bound >= 0) and np.all(ref.dpred_bound[w > 0].max((1, 2)) > 0)
    assert np.all(np.abs(ref.dpred) <= ref.dpred_bound / ((P2 + R.DPRED_STEPS) * R.U) * (1 + 1e-12))


# ----------------------------------------------------------------------------------------------
# weighted-mean finish, chain
# ----------------------------------------------------------------------------------------------
def test_finish_inputs_keep_the_weight_sum_exact():
    term, w = R.finish_inputs()
    assert term.dtype == np.float32 and len(term) == max(R.FINISH_N) and (term >= 0).all()
    for n in R.FINISH_N:
        assert R.weights_sum_exact(w[:n]) and w[:n].sum() > 0
        loss, inv, lb, ib = R.mean_finish(term[:n], w[:n])
        ref = float(term[:n].astype(np.float64).sum()) / float(w[:n].astype(np.float64).sum())
        assert loss == pytest.approx(ref, rel=1e-14) and lb > 0 and ib == 2 * R.U
    assert R.mean_finish(term[:5], np.zeros(5, np.float32))[:2] == (0.0, 0.0)
    assert not R.weights_sum_exact(np.array([2.0 ** 24, 1.0])) and R.weights_sum_exact(np.array([0.0, 3.0, 2.0 ** -10]))


def test_chain_scene_is_dyadic():
    sc = R.chain_scene()
    gt, _ = R.group_gt(sc["points"], 4, sc["pt_off"], sc["csr"], sc["voxel_coords"], 64, sc["lo"], sc["vs"])
    assert np.array_equal(gt * 64, np.round(gt * 64)) and np.abs(gt).max() <= 2
    pred = gt[:, :16] + sc["perturb"]
    assert np.array_equal(pred * 64, np.round(pred * 64)) and np.abs(pred).max() <= 3
    assert R.weights_sum_exact(sc["w"])
