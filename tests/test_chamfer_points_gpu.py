"""gdmae_chamfer_points (csrc/chamfer.hip): the Chamfer kernel that takes its targets from the points, against the two launches it
replaces, gdmae_group_gt_points -> gdmae_chamfer, through the C ABI.

* bit-equality of `term` and `dpred` with the two-launch path on every scene; every call is made twice into NaN-filled buffers.
  The two-launch kernel evaluates the column term 2 cy (x_i - y_j) inside its loop over j, the fused one once per ground-truth
  point: the equality also holds that change against the loop it replaces
* on the dyadic scenes (point offsets and predictions are multiples of 1 / 64 around centres that are multiples of 1 / 4, so every
  squared distance is exact in fp32 - the property the operation counts of loss_tail_reference.chamfer rest on) both paths stay
  within that reference's own bounds times the factor 2 of tests/test_loss_tail_gpu.py.  The uniform scenes carry rounded
  differences, which those counts do not cover: there the two paths are compared with each other only.
* the points of zero-weight pillars overwritten with NaN: no output bit changes, so the kernel never reads them

Pillar sizes 1, 2, 3, 5, 63, 64, 65, 200: with K = 64 the cyclic pad (cnt < K) and the first-64-by-list-order rule (cnt > K); K = 5 and 63
leave lanes without a target.  Predictions lie within a pillar's half-width."""
import functools

import numpy as np
import pytest
import torch

import loss_tail_reference as R

pytestmark = pytest.mark.gpu
SLACK = 2.0               # over the derived bound and no more, as tests/test_loss_tail_gpu.py
SIZES = [1, 2, 3, 5, 63, 64, 65, 200]
P1 = 16


def dev():
    return torch.device("cuda:0")


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _scene(kind, K, n_cols):
    """-> (scene, pred (M, 16, 3), w (M,)); "dyadic" / "uniform": the crafted sizes, "many_*": M = 4 * 8192 + 5 pillars of 1 to 3 points"""
    dyadic = kind.endswith("dyadic")
    geo = dict(lo=R.CHAIN_LO, vs=R.CHAIN_VS, grid=256) if dyadic else {}
    if kind.startswith("many"):
        sizes = np.random.default_rng(1).integers(1, 4, R.CHAMFER_M_MANY)
        sc = R.gt_scene(K, n_cols, sizes=sizes, seed=1, dyadic=dyadic, **geo)
    else:
        sc = R.gt_scene(K, n_cols, sizes=SIZES * 12, seed=K + n_cols, dyadic=dyadic, **geo)
    M = sc["M"]
    rng = np.random.default_rng(100 + K)
    if dyadic:                                            # multiples of 1 / 64 within the half-width (0.25, 0.25, 2) of a pillar
        pred = rng.integers(-16, 17, (M, P1, 3)) / 64.0
        pred[:, :, 2] = rng.integers(-128, 129, (M, P1)) / 64.0
    else:
        pred = rng.uniform(-0.5, 0.5, (M, P1, 3)) * np.asarray(sc["vs"])
    w = R.chamfer_weights(M, seed=K, runs=True)           # zeros, runs of zeros, 1, 0.5, 2^-10, 3
    assert (w == 0).sum() > 3 and (w != 0).sum() > 3
    return sc, pred.astype(np.float32), w


def _two_launches(sc, n_cols, K, pred, w):
    from gdmae_hip import lib as L
    M = sc["M"]
    pts, off, csr, vc = _d(sc["points"]), _d(sc["pt_off"]), _d(sc["csr"]), _d(sc["voxel_coords"])
    gt = torch.full((M, K, 3), float("nan"), device=dev())
    L.call("gdmae_group_gt_points", L.ptr(pts), n_cols, L.ptr(off), L.ptr(csr), L.ptr(vc), M, K, L.host_f32(sc["lo"]),
           L.host_f32(sc["vs"]), L.ptr(gt), None, L.stream())
    term = torch.full((M,), float("nan"), device=dev())
    dpred = torch.full((M, P1, 3), float("nan"), device=dev())
    p_d, w_d = _d(pred), _d(w)                            # named: a temporary's memory would be handed out again before the launch
    L.call("gdmae_chamfer", L.ptr(p_d), L.ptr(gt), L.ptr(w_d), M, P1, K, L.ptr(term), L.ptr(dpred), L.stream())
    return term.cpu().numpy(), dpred.cpu().numpy(), gt.cpu().numpy()


def _fused(sc, n_cols, K, pred, w, points=None):
    """gdmae_chamfer_points twice into NaN-filled buffers: bit-equal, returned once"""
    from gdmae_hip import lib as L
    M = sc["M"]
    pts = _d(sc["points"] if points is None else points)
    off, csr, vc, p_d, w_d = _d(sc["pt_off"]), _d(sc["csr"]), _d(sc["voxel_coords"]), _d(pred), _d(w)
    res = []
    for _ in range(2):
        term = torch.full((M,), float("nan"), device=dev())
        dpred = torch.full((M, P1, 3), float("nan"), device=dev())
        L.call("gdmae_chamfer_points", L.ptr(p_d), L.ptr(pts), n_cols, L.ptr(off), L.ptr(csr), L.ptr(vc), L.host_f32(sc["lo"]),
               L.host_f32(sc["vs"]), L.ptr(w_d), M, P1, K, L.ptr(term), L.ptr(dpred), L.stream())
        res.append((term.cpu().numpy(), dpred.cpu().numpy()))
    assert np.array_equal(_bits(res[0][0]), _bits(res[1][0])) and np.array_equal(_bits(res[0][1]), _bits(res[1][1])), "two calls differ"
    return res[0]


def _nan_points_of_dead_pillars(sc, w):
    pts = sc["points"].copy()
    for m in np.flatnonzero(w == 0):
        ids = sc["csr"][sc["pt_off"][m]:sc["pt_off"][m + 1]]
        pts[ids, 1:4] = np.nan
    assert np.isnan(pts).any()
    return pts


def _check(kind, K, n_cols):
    sc, pred, w = _scene(kind, K, n_cols)
    term0, dpred0, gt = _two_launches(sc, n_cols, K, pred, w)
    term1, dpred1 = _fused(sc, n_cols, K, pred, w)
    for name, a, b in (("term", term0, term1), ("dpred", dpred0, dpred1)):
        assert np.isfinite(b).all(), f"{name}: unwritten output"
        bad = np.argwhere(_bits(a) != _bits(b))
        assert bad.size == 0, (name, len(bad), bad[:4].tolist(), np.diff(sc["pt_off"])[bad[:4, 0]].tolist())
    z = w == 0
    assert np.all(_bits(term1[z]) == 0) and np.all(_bits(dpred1[z]) == 0), "zero-weight pillars must be exactly +0"
    # the points of the zero-weight pillars are never read
    term2, dpred2 = _fused(sc, n_cols, K, pred, w, points=_nan_points_of_dead_pillars(sc, w))
    assert np.array_equal(_bits(term1), _bits(term2)) and np.array_equal(_bits(dpred1), _bits(dpred2))
    if kind.endswith("dyadic"):
        gt_ref, _ = R.group_gt(sc["points"], n_cols, sc["pt_off"], sc["csr"], sc["voxel_coords"], K, sc["lo"], sc["vs"])
        assert np.array_equal(_bits(gt), _bits(gt_ref))
        ref = R.chamfer(pred, gt_ref, w)
        for what, term, dpred in (("two launches", term0, dpred0), ("fused", term1, dpred1)):
            et = np.abs(term - ref.term)
            bad = np.flatnonzero(et > SLACK * ref.term_bound)
            assert bad.size == 0, (what, "term", bad[:6], et[bad[:6]], ref.term_bound[bad[:6]])
            ed = np.abs(dpred - ref.dpred)
            bad = np.argwhere(ed > SLACK * ref.dpred_bound)
            assert bad.size == 0, (what, "dpred", len(bad), bad[:6].tolist())


@pytest.mark.parametrize("n_cols", [4, 6])
@pytest.mark.parametrize("K", [5, 63, 64])
@pytest.mark.parametrize("kind", ["dyadic", "uniform"])
def test_chamfer_points_equals_the_two_launches(kind, K, n_cols):
    _check(kind, K, n_cols)


@pytest.mark.parametrize("kind", ["many_dyadic", "many_uniform"])
def test_chamfer_points_grid_stride_loop(kind):
    """M = 4 * 8192 + 5 > 4 * 8192: the launch is capped, waves 0 - 4 walk a second pillar (live after live, zero-weight after live,
    live after the early `continue`: loss_tail_reference.chamfer_weights(runs=True))."""
    _check(kind, 64, 4)


def test_chamfer_points_refuses_what_it_does_not_serve():
    from gdmae_hip import lib as L
    sc, pred, w = _scene("dyadic", 5, 4)
    M = sc["M"]
    t = [_d(pred), _d(sc["points"]), _d(sc["pt_off"]), _d(sc["csr"]), _d(sc["voxel_coords"]), _d(w), torch.zeros(M, device=dev()),
         torch.zeros(M, P1, 3, device=dev())]
    for p1, p2 in ((15, 5), (16, 65), (16, 0)):
        with pytest.raises(L.GdmaeHipError):
            L.call("gdmae_chamfer_points", L.ptr(t[0]), L.ptr(t[1]), 4, L.ptr(t[2]), L.ptr(t[3]), L.ptr(t[4]), L.host_f32(sc["lo"]),
                   L.host_f32(sc["vs"]), L.ptr(t[5]), M, p1, p2, L.ptr(t[6]), L.ptr(t[7]), L.stream())


def test_chamfer_loss_takes_lazy_targets_and_the_dict_materialises_them():
    """ops.ChamferLoss on ops.LazyTargets = on the materialised tensor, bit for bit (loss and gradient); ops.TargetDict hands the
    tensor to anyone who reads 'gt_points' by key and the lazy object to raw()."""
    from types import SimpleNamespace

    from gdmae_hip import ops
    sc, pred, w = _scene("uniform", 64, 4)
    vox = SimpleNamespace(points=_d(sc["points"]), n_cols=4, pt_off=_d(sc["pt_off"]), pillar_pts=_d(sc["csr"]),
                          voxel_coords=_d(sc["voxel_coords"]), M=sc["M"], lo=sc["lo"], vs=sc["vs"])
    lazy = ops.LazyTargets(vox, 64)
    fr = ops.TargetDict(gt_points=lazy, mask=_d(w))
    assert fr.raw("gt_points") is lazy and lazy._gt is None
    out = []
    for gt in (lazy, ops.group_gt_points(vox, 64)):
        p = _d(pred).requires_grad_(True)
        loss = ops.ChamferLoss.apply(p, gt, fr["mask"])
        loss.backward()
        out.append((loss.detach().cpu().numpy(), p.grad.cpu().numpy()))
    assert lazy._gt is None, "the loss must not have written the targets"
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0])) and np.array_equal(_bits(out[0][1]), _bits(out[1][1]))
    gt = fr["gt_points"]
    assert torch.is_tensor(gt) and gt.shape == (sc["M"], 64, 3) and fr.get("gt_points") is gt
    assert torch.equal(gt, ops.group_gt_points(vox, 64))
