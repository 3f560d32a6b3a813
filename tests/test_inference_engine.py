"""Inference engine of the config-D detector (gdmae_hip.inference): the three new C entry points against fp64 formulas on the CPU, and
the engine against the model's own evaluation path (``model.eval(); model(batch_dict)``: the exact fp32 mode, and its bf16-autocast
form as the yardstick for 16-bit deviation).

Bounds.  The C-ABI checks bound every element by the rounding of the formats involved: an output rounded to bf16 is within 2^-8 of
its value (half an ulp is 2^-9), an fp16 operand within 2^-11, and an fp32 accumulation of K terms within K 2^-24 of the sum of the
terms' magnitudes (2^-16 of it is used: K <= 3456 here).  The engine check uses the project's standing margin: the engine's
deviation from the fp32 evaluation path is at most 2 x the deviation of the bf16-autocast evaluation path on the same quantity (both
round activations to 16 bits at the same layer boundaries, in a different operation order).
"""
import logging

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gdmae_hip import configs, synth
from gdmae_hip import lib as L

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _bf(x):
    return x.to(torch.bfloat16).double()


# ------------------------------------------------------------------------------------------------------------------------------
# C ABI
# ------------------------------------------------------------------------------------------------------------------------------
def _vfe_case(dev, pts_np, B=1):
    """gdmae_vfe_infer on crafted points against the fp64 formula; -> (out, reference, bound)."""
    from gdmae_hip import plan as gplan
    _, ds, _ = configs.named_config("D")
    pts = torch.from_numpy(pts_np).to(dev)
    vox = gplan.voxelize(pts, ds.point_cloud_range, ds.voxel_size, ds.grid_size, B)
    g = torch.Generator().manual_seed(11)
    D = vox.n_cols - 1 + 6
    W1 = torch.randn(64, D, generator=g) * 0.3
    b1 = torch.randn(64, generator=g) * 0.2
    W2 = torch.randn(128, 64, generator=g) * 0.2
    b2 = torch.randn(128, generator=g) * 0.2
    out = torch.full((max(vox.M, 1), 128), float("nan"), device=dev)
    W1d, b1d, W2d, b2d = W1.to(dev), b1.to(dev), W2.to(dev), b2.to(dev)      # named: a temporary's block would be reused by the next copy
    L.call("gdmae_vfe_infer", L.ptr(vox.points_pm), L.ptr(vox.voxel_coords), L.ptr(vox.row_pillar), L.ptr(vox.pillar_mean), int(vox.N),
           int(vox.M), vox.n_cols, L.host_f32(vox.lo), L.host_f32(vox.vs), L.ptr(W1d), L.ptr(b1d), 64, L.ptr(W2d), L.ptr(b2d), 128, L.ptr(out),
           L.stream())
    torch.cuda.synchronize()
    if vox.N == 0:
        return vox, out, None, None
    p = vox.points_pm.cpu().double()
    rp = vox.row_pillar.cpu().long()
    vc = vox.voxel_coords.cpu().double()[rp]
    mean = vox.pillar_mean.cpu().double()[rp]
    lo, vs = torch.tensor(vox.lo, dtype=torch.float64), torch.tensor(vox.vs, dtype=torch.float64)
    ctr = (vc[:, [3, 2, 1]] + 0.5) * vs + lo
    f = torch.cat([p[:, 1:4] - ctr, p[:, 1:], p[:, 1:4] - mean[:, :3]], dim=1)
    h1 = torch.relu(f @ W1.double().t() + b1.double())
    h1r = h1.to(torch.float16).double()
    W2r = W2.to(torch.float16).double()
    h2 = torch.relu(h1r @ W2r.t() + b2.double())
    # layer 1 in fp32 (2^-20 of the magnitudes is generous), its output rounded to fp16 (2^-11), fp32 accumulation of layer 2
    e1 = 2.0 ** -20 * (f.abs() @ W1.double().abs().t() + b1.double().abs()) + 2.0 ** -11 * h1
    eb = e1 @ W2r.abs().t() + 2.0 ** -16 * (h1r @ W2r.abs().t() + b2.double().abs())
    M = vox.M
    ref = torch.zeros(M, 128, dtype=torch.float64).scatter_reduce(0, rp[:, None].expand(-1, 128), h2, "amax", include_self=True)
    bound = torch.zeros(M, 128, dtype=torch.float64).scatter_reduce(0, rp[:, None].expand(-1, 128), eb, "amax", include_self=True)
    return vox, out, ref, bound


def test_vfe_infer_matches_fp64_formula_with_crowded_and_single_point_pillars():
    dev = _dev()
    _, ds, skw = configs.named_config("D")
    rng = np.random.default_rng(5)
    base = synth.synth_batch(3, 1, ds.point_cloud_range, beams=8, azimuths=100, extra=100, features=4)
    crowd = np.zeros((5000, 5), dtype=np.float32)                        # 5 000 points inside one 0.16 m pillar
    crowd[:, 1] = 20.0 + 0.16 * 0.5 + rng.uniform(-0.07, 0.07, 5000)
    crowd[:, 2] = -39.68 + 0.16 * 267.5 + rng.uniform(-0.07, 0.07, 5000)
    crowd[:, 3] = rng.uniform(-2.5, 0.5, 5000)
    crowd[:, 4] = rng.uniform(0, 1, 5000)
    single = np.array([[0, 60.01, -30.01, -1.0, 0.5]], dtype=np.float32)   # a pillar of one point, far from the rest
    pts = np.concatenate([base, crowd, single]).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    vox, out, ref, bound = _vfe_case(dev, pts)
    counts = torch.bincount(vox.row_pillar.cpu().long(), minlength=vox.M)
    assert int(counts.max()) >= 5000 and int((counts == 1).sum()) >= 1
    dev_abs = (out.cpu().double() - ref).abs()
    print(f"vfe_infer: N={vox.N} M={vox.M} max |dev| {float(dev_abs.max()):.3e}  max bound {float(bound.max()):.3e}  "
          f"max ratio {float((dev_abs / (bound + 1e-30)).max()):.3f}")
    assert torch.isfinite(out).all()
    assert bool((dev_abs <= bound + 1e-6).all())
    # repeatable bit for bit (atomic maxima do not depend on their order)
    _, out2, _, _ = _vfe_case(dev, pts)
    assert torch.equal(out, out2)


def test_vfe_infer_empty_input_returns_without_touching_the_output():
    dev = _dev()
    pts = np.zeros((0, 5), dtype=np.float32)
    vox, out, _, _ = _vfe_case(dev, pts)
    assert vox.N == 0 and vox.M == 0 and torch.isnan(out).all()


@pytest.mark.parametrize("cin,cout,n", [(128, 128, 129), (128, 256, 65), (256, 256, 64)])
def test_spconv_bias_relu_matches_fp64_formula_at_tile_edges(cin, cout, n):
    from gdmae_hip import packing
    dev = _dev()
    g = torch.Generator().manual_seed(cin + cout + n)
    n_src = 200
    X = (torch.randn(n_src, cin, generator=g)).to(torch.bfloat16)
    W = torch.randn(cout, 3, 3, cin, generator=g) * 0.05
    b = torch.randn(cout, generator=g)
    nbr = torch.randint(-1, n_src, (n, 9), generator=g).int()
    nbr[0] = -1                                                          # a row without any neighbour: relu(b)
    Wdev = W.to(dev).contiguous()
    packed, _ = packing.conv_pack_now(Wdev)
    Y = torch.full((n + 7, cout), float("nan"), dtype=torch.bfloat16, device=dev)
    Xd_, nbrd, bd_ = X.to(dev), nbr.to(dev), b.to(dev)                   # named: a temporary's block would be reused by the next copy
    L.call("gdmae_spconv_bias_relu", L.ptr(Xd_), 0, L.ptr(nbrd), L.ptr(packed), L.ptr(bd_), n, cin, cout, L.ptr(Y), L.stream())
    torch.cuda.synchronize()
    Xd, Wd = X.double(), _bf(W)
    acc = torch.zeros(n, cout, dtype=torch.float64)
    sabs = torch.zeros(n, cout, dtype=torch.float64)
    for t in range(9):
        idx = nbr[:, t].long()
        rows = Xd[idx.clamp_min(0)] * (idx >= 0)[:, None]
        wt = Wd[:, t // 3, t % 3, :]
        acc += rows @ wt.t()
        sabs += rows.abs() @ wt.abs().t()
    ref = torch.relu(acc + b.double())
    dev_abs = (Y[:n].cpu().double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -16 * (sabs + b.double().abs())
    print(f"spconv_bias_relu {cin}->{cout} n={n}: max |dev| {float(dev_abs.max()):.3e}, max ratio {float((dev_abs / (bound + 1e-30)).max()):.3f}")
    assert bool((dev_abs <= bound + 1e-7).all())
    assert torch.isnan(Y[n:].float()).all()                              # nothing written past the last row


@pytest.mark.parametrize("dil", [1, 2])
@pytest.mark.parametrize("shortcut", [False, True])
def test_conv3x3_dense_relu_matches_fp64_formula(dil, shortcut):
    dev = _dev()
    B, H, W, cin, cout = 2, 13, 21, 64, 64                               # neither side a multiple of the 8 x 8 tile
    g = torch.Generator().manual_seed(10 * dil + int(shortcut))
    x = torch.randn(B, cin, H, W, generator=g).to(torch.bfloat16)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.05
    b = torch.randn(cout, generator=g)
    sc = torch.randn(B, cout, H, W, generator=g).to(torch.bfloat16)
    packed = torch.empty(L.load().gdmae_conv3x3_dense_packed_bytes(cin, cout), dtype=torch.uint8, device=dev)
    wdev, bdev = w.to(dev), b.to(dev)
    L.call("gdmae_conv3x3_dense_pack", L.ptr(wdev), cin, cout, dil, 0, L.ptr(packed), L.stream())
    xr = x.permute(0, 2, 3, 1).contiguous().to(dev)
    scr = sc.permute(0, 2, 3, 1).contiguous().to(dev)
    y = torch.full((B, H, W, cout), float("nan"), dtype=torch.bfloat16, device=dev)
    L.call("gdmae_conv3x3_dense_relu", L.ptr(xr), B, H, W, cin, cout, dil, L.ptr(packed), L.ptr(bdev), L.ptr(scr) if shortcut else None,
           L.ptr(y), L.stream())
    torch.cuda.synchronize()
    xd, wd = x.double(), _bf(w)
    conv = F.conv2d(xd, wd, b.double(), padding=dil, dilation=dil)
    sabs = F.conv2d(xd.abs(), wd.abs(), b.double().abs(), padding=dil, dilation=dil)
    r = torch.relu(conv)
    ref = r + sc.double() if shortcut else r
    bound = 2.0 ** -8 * r + 2.0 ** -16 * sabs + (2.0 ** -8 * ref.abs() + 2.0 ** -8 * 2.0 ** -8 * r if shortcut else 0.0)
    dev_abs = (y.permute(0, 3, 1, 2).cpu().double() - ref).abs()
    print(f"conv3x3_dense_relu dil={dil} shortcut={shortcut}: max |dev| {float(dev_abs.max()):.3e}, max ratio {float((dev_abs / (bound + 1e-30)).max()):.3f}")
    assert torch.isfinite(y.float()).all()
    assert bool((dev_abs <= bound + 1e-7).all())
    if shortcut:      # ReLU first, then the add: a negative shortcut shows through where the convolution was clipped
        assert float(y.float().min()) < 0


# ------------------------------------------------------------------------------------------------------------------------------
# engine
# ------------------------------------------------------------------------------------------------------------------------------
def _model(seed=3, stats=True):
    """Config-D detector with seeded weights and NON-TRIVIAL BatchNorm buffers (fresh buffers are (0, 1): folded and unfolded
    weights would agree to within eps)."""
    from pcdet.models import build_network
    cfg, ds, skw = configs.named_config("D")
    torch.manual_seed(seed)
    net = build_network(cfg, len(ds.class_names), ds, logging.getLogger("t"))
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                c = m.num_features
                if stats:
                    m.running_mean.copy_(torch.randn(c, generator=g) * 0.2)
                    m.running_var.copy_(torch.rand(c, generator=g) * 1.0 + 0.5)
                m.weight.copy_(1.0 + 0.2 * torch.randn(c, generator=g))
                m.bias.copy_(0.2 * torch.randn(c, generator=g))
    return net.to(_dev()).eval(), ds, skw


def _batch(ds, skw, seed=21, B=2):
    pts = synth.synth_batch(seed, B, ds.point_cloud_range, **skw)
    return {"points": torch.from_numpy(pts).to(_dev()), "batch_size": B}


def _fallback_maps(net, bd, autocast):
    """head maps, spatial maps and pillar features of today's evaluation path"""
    d = dict(bd)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        for mod in net.module_list:
            d = mod(d)
    pd = net.dense_head.forward_ret_dict["pred_dicts"][0]
    q = {k: v.float() for k, v in pd.items()}
    q.update(spatial_features=d["spatial_features"].float(), spatial_features_2d=d["spatial_features_2d"].float(),
             pillar_features=d["pillar_features"].float(), voxel_coords=d["voxel_coords"])
    return q


def _engine_maps(eng, bd):
    hm = eng.head_maps(dict(bd))
    q = {k: v.float() for k, v in hm[0].items()}
    q.update(spatial_features=hm.spatial_features.float(), spatial_features_2d=hm.spatial_features_2d.float(),
             pillar_features=hm.pillar_features.float(), voxel_coords=hm.voxel_coords)
    return q


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


QUANTITIES = ("pillar_features", "spatial_features", "spatial_features_2d", "hm", "center", "center_z", "dim", "rot")


@pytest.fixture(scope="module")
def compiled():
    from gdmae_hip import inference
    net, ds, skw = _model()
    return net, ds, skw, inference.compile_detector(net)


def _golden_model(z, buffers=True):
    """The detector of the evaluation golden: KITTI 0.32 m pillars, the golden's seeded weights and (buffers) its running statistics."""
    from head_seed import seeded_head_state
    from oracle import gdmae_oracle as orc
    from pcdet.config import AttrDict
    from pcdet.models import build_network
    ds = configs.SyntheticDatasetInfo(**{**configs.KITTI, "class_names": ['Vehicle', 'Pedestrian', 'Cyclist']})
    ssl = configs.gdmae_ssl_model_cfg(0.0, eval_metric='kitti')
    cfg = AttrDict({'NAME': 'CenterPoint', 'VFE': ssl.VFE, 'BACKBONE_3D': configs.gdmae_finetune_backbone_cfg(eval_metric='kitti'),
                    'BACKBONE_2D': configs.sst_bev_backbone_cfg(), 'DENSE_HEAD': configs.center_head_cfg(),
                    'POST_PROCESSING': ssl.POST_PROCESSING})
    net = build_network(cfg, 3, ds, logging.getLogger("t"))

    class Front(torch.nn.Module):
        def __init__(s):
            super().__init__()
            s.vfe, s.backbone_3d = net.vfe, net.backbone_3d

    class Back(torch.nn.Module):
        def __init__(s):
            super().__init__()
            s.backbone_2d, s.dense_head = net.backbone_2d, net.dense_head
    front, back = Front(), Back()
    shapes = {str(n): tuple(int(v) for v in sh if v > 0) for n, sh in zip(z["front_names"], z["front_shapes"])}
    assert {k: tuple(v.shape) for k, v in front.named_parameters()} == shapes
    seed = int(z["seed"])
    front.load_state_dict(orc.seeded_state_dict(shapes, seed=seed), strict=False)
    back.load_state_dict(seeded_head_state(back, seed), strict=False)
    if buffers:
        sd = net.state_dict()
        bufs = {k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("bn/")}
        assert bufs and all(k in sd and sd[k].shape == v.shape for k, v in bufs.items())
        n_bn = sum(isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)) for m in net.modules())
        assert len(bufs) == 2 * n_bn
        net.load_state_dict(bufs, strict=False)
    return net.to(_dev()).eval()


def _golden_dev(q, z, name):
    """(relative L2, max element / largest reference element) of quantity `name` against the golden's samples (and, for head maps,
    its values at the per-class top-64 heat-map cells)"""
    from helpers import sample
    s, _ = sample(q[name])
    ref = z[name + "_s"].astype(np.float64)
    got = s.astype(np.float64)
    if name + "_top" in z:
        t = q[name]
        B, c = t.shape[0], t.shape[1]
        cells = torch.from_numpy(z["top_cells"].astype(np.int64)).reshape(B, -1).to(t.device)
        flat = t.reshape(B, c, -1)
        top = torch.stack([flat[b][:, cells[b]] for b in range(B)]).double().cpu().numpy()
        got = np.concatenate([got, top.reshape(-1)])
        ref = np.concatenate([ref, z[name + "_top"].astype(np.float64).reshape(-1)])
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref)), float(np.abs(got - ref).max() / np.abs(ref).max())


def test_engine_parity_with_the_reference_eval_golden():
    """tests/golden/detector_eval_kitti_b2.npz: the UNMODIFIED reference chain in eval mode with running statistics it produced
    itself (one momentum-1 training forward on another batch).  voxel_coords bit-exact; for every quantity the engine's deviation from
    the golden (relative L2 and max element, on the golden's samples + top-64 cells) is at most 2 x the deviation of today's
    bf16-autocast evaluation path; the fp32 evaluation path must be sampled-close at 5e-4 on both dense maps (the sanity anchor:
    otherwise golden or loading is wrong).  Measured on an MI355X (relative L2: fp32 fallback / bf16 fallback / engine): see
    profiles/r08_inference.txt; the test prints the same table."""
    import os
    from gdmae_hip import inference
    from helpers import assert_sampled_close
    z = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detector_eval_kitti_b2.npz")))
    net = _golden_model(z)
    bd = {"points": torch.from_numpy(z["points"]).to(_dev()), "batch_size": int(z["batch_size"])}
    torch.backends.cudnn.allow_tf32 = False
    ref = _fallback_maps(net, bd, False)
    low = _fallback_maps(net, bd, True)
    got = _engine_maps(inference.compile_detector(net), bd)
    for q in (ref, low, got):
        assert np.array_equal(q["voxel_coords"].cpu().numpy(), z["voxel_coords"])
    rows, bad = [], []
    for k in QUANTITIES:
        f, y, e = _golden_dev(ref, z, k), _golden_dev(low, z, k), _golden_dev(got, z, k)
        rows.append(f"{k:20s} rel-L2 fp32 {f[0]:.3e} bf16 {y[0]:.3e} engine {e[0]:.3e} | max-el fp32 {f[1]:.3e} bf16 {y[1]:.3e} engine {e[1]:.3e}")
        if not (e[0] <= 2 * y[0] and e[1] <= 2 * y[1]):
            bad.append(k)
    print("\n".join(["golden parity (deviation from the reference's eval forward):"] + rows))
    assert_sampled_close(ref["spatial_features"], z["spatial_features_s"], z["spatial_features_c"], 5e-4, "spatial_features (fp32 fallback)")
    assert_sampled_close(ref["spatial_features_2d"], z["spatial_features_2d_s"], z["spatial_features_2d_c"], 5e-4, "spatial_features_2d (fp32 fallback)")
    assert not bad, bad
    # folding is exercised: the same weights with (0, 1) statistics are further from the golden than the engine's bound allows
    plain = _engine_maps(inference.compile_detector(_golden_model(z, buffers=False)), bd)
    for k in ("spatial_features_2d", "hm", "dim"):
        assert _golden_dev(plain, z, k)[0] > 2 * _golden_dev(low, z, k)[0], k


def test_engine_deviation_is_within_twice_the_bf16_evaluation_path(compiled):
    """Reference: the fp32 evaluation path of the model (the exact mode).  Yardstick: the same path under bf16 autocast.  Measured
    figures are printed (run with -s); the assertion is engine <= 2 x yardstick per quantity, relative L2."""
    net, ds, skw, eng = compiled
    bd = _batch(ds, skw)
    ref = _fallback_maps(net, bd, False)
    low = _fallback_maps(net, bd, True)
    got = _engine_maps(eng, bd)
    assert torch.equal(got["voxel_coords"], ref["voxel_coords"])
    bad = []
    for k in QUANTITIES:
        assert got[k].shape == ref[k].shape, k
        e, y = _rel(got[k], ref[k]), _rel(low[k], ref[k])
        emax, ymax = float((got[k] - ref[k]).abs().max()), float((low[k] - ref[k]).abs().max())
        print(f"{k:20s} rel-L2 engine {e:.3e}  bf16 fallback {y:.3e}   max-abs engine {emax:.3e}  bf16 fallback {ymax:.3e}")
        if not e <= 2 * y:
            bad.append((k, e, y))
    assert not bad, bad


def test_running_statistics_reach_the_kernels(compiled):
    """the same weights with the running statistics reset to (0, 1) give different head maps: the buffers are folded in"""
    from gdmae_hip import inference
    net, ds, skw, eng = compiled
    bd = _batch(ds, skw)
    got = _engine_maps(eng, bd)
    plain, _, _ = _model(stats=False)
    other = _engine_maps(inference.compile_detector(plain), bd)
    ref = _fallback_maps(net, bd, False)
    for k in ("spatial_features_2d", "hm", "dim"):
        assert _rel(other[k], got[k]) > 2 * _rel(got[k], ref[k]), k


def test_boxes_are_the_decoded_head_maps_and_recall_matches(compiled):
    from tests_golden_boxes import synth_boxes
    net, ds, skw, eng = compiled
    bd = _batch(ds, skw)
    B = bd["batch_size"]
    boxes, recall = eng(dict(bd))
    want = net.dense_head.generate_predicted_boxes(B, eng.head_maps(dict(bd)))
    assert len(boxes) == B and recall == {}
    for a, b in zip(boxes, want):
        assert a["pred_boxes"].shape[1] == 7
        for k in ("pred_boxes", "pred_scores", "pred_labels"):
            assert torch.equal(a[k], b[k]), k
    gt = torch.from_numpy(synth_boxes(np.random.default_rng(5), B, 20, np.asarray(ds.point_cloud_range), 3)).to(_dev())
    boxes2, recall2 = eng({**bd, "gt_boxes": gt})
    _, want_rec = net.post_processing({"final_box_dicts": boxes2, "batch_size": B, "gt_boxes": gt})
    assert recall2 == want_rec and recall2["gt_num"] > 0


# Framework ops one engine call may record.  STRUCTURAL: allocation, views, copies / casts (the decode path casts the head maps to fp32).
STRUCTURAL = {
    "aten::empty", "aten::empty_like", "aten::empty_strided", "aten::zeros", "aten::zero_", "aten::fill_", "aten::full", "aten::view",
    "aten::reshape", "aten::_reshape_alias", "aten::permute", "aten::slice", "aten::select", "aten::as_strided", "aten::contiguous",
    "aten::clone", "aten::copy_", "aten::to", "aten::_to_copy", "aten::unsqueeze", "aten::squeeze", "aten::expand", "aten::flatten",
    "aten::detach", "aten::detach_", "aten::resolve_conj", "aten::resolve_neg", "aten::alias", "aten::lift_fresh", "aten::item",
    "aten::_local_scalar_dense", "aten::resize_", "aten::narrow", "aten::unbind", "aten::split", "aten::split_with_sizes", "aten::t",
    "aten::transpose", "aten::result_type", "aten::_unsafe_view", "aten::view_as", "aten::set_", "aten::is_nonzero", "aten::tolist",
    "aten::tensor", "aten::scalar_tensor", "aten::ones", "aten::ones_like", "aten::zeros_like", "aten::new_tensor", "aten::new_zeros",
    "aten::new_empty", "aten::arange", "aten::float", "aten::long", "aten::int", "aten::bool", "aten::expand_as", "aten::empty_permuted",
}
# box decoding on the head maps, as CenterHead.generate_predicted_boxes does it today (unchanged): the heat map's sigmoid and top-K
DECODE = {"aten::sigmoid", "aten::topk"}
# SMALL: index arithmetic of the geometry plan and bookkeeping on the <= K selected boxes.  None of these may see a tensor as large as
# ONE channel of a full map (B H W elements) - a BatchNorm / ReLU / add pass under another name (clamp, where, mul, add ...) would.
SMALL = {
    "aten::div", "aten::floor_divide", "aten::remainder", "aten::mul", "aten::add", "aten::sub", "aten::flip", "aten::cat", "aten::stack",
    "aten::sin", "aten::cos", "aten::pow", "aten::index_select", "aten::sum", "aten::cumsum", "aten::index", "aten::index_put_",
    "aten::_index_put_impl_", "aten::gather", "aten::nonzero", "aten::sort", "aten::argsort", "aten::lt", "aten::gt", "aten::ge",
    "aten::le", "aten::eq", "aten::ne", "aten::bitwise_and", "aten::__and__", "aten::abs", "aten::max", "aten::min", "aten::any",
    "aten::all", "aten::where", "aten::masked_select", "aten::clamp", "aten::clamp_min", "aten::bitwise_not", "aten::logical_not",
}
FORBIDDEN = ("aten::convolution", "aten::_convolution", "aten::conv", "aten::miopen_", "aten::cudnn_", "aten::batch_norm", "aten::native_batch_norm",
             "aten::_native_batch_norm", "aten::_batch_norm", "aten::relu", "aten::threshold", "aten::mm", "aten::addmm", "aten::bmm",
             "aten::baddbmm", "aten::matmul", "aten::linear")


def test_no_framework_compute_kernels_in_an_engine_call(compiled):
    from torch.profiler import ProfilerActivity, profile
    net, ds, skw, eng = compiled
    bd = _batch(ds, skw)
    eng(dict(bd))
    with profile(activities=[ProfilerActivity.CPU], record_shapes=True) as prof:
        eng(dict(bd))
    evs = [e for e in prof.events() if e.name.startswith("aten::")]
    names = sorted({e.name for e in evs})
    bad = [n for n in names if any(n.startswith(f) for f in FORBIDDEN)]
    assert not bad, bad
    new = [n for n in names if n not in STRUCTURAL | DECODE | SMALL]
    assert not new, f"framework ops not on the allowed lists (add them on purpose if they are bookkeeping): {new}"
    one_channel = bd["batch_size"] * int(ds.grid_size[0]) * int(ds.grid_size[1])
    big = []
    for e in evs:
        if e.name in SMALL:
            numel = max([int(np.prod(sh)) for sh in (e.input_shapes or []) if isinstance(sh, (list, tuple)) and len(sh)] or [0])
            if numel >= one_channel:
                big.append((e.name, e.input_shapes))
    assert not big, f"elementwise framework ops over map-sized tensors: {big}"


_CHILD = """
import logging, sys, torch
sys.path[:0] = [{repo!r}, {pkg!r}]
from gdmae_hip import configs, inference, synth
from pcdet.models import build_network
cfg, ds, skw = configs.named_config("D")
torch.manual_seed(3)
net = build_network(cfg, 3, ds, logging.getLogger("t")).cuda().eval()
eng = inference.compile_detector(net)
pts = torch.from_numpy(synth.synth_batch(21, 2, ds.point_cloud_range, **skw)).cuda()
boxes, _ = eng({{"points": pts, "batch_size": 2}})
torch.cuda.synchronize()
assert len(boxes) == 2
print("engine-ok")
"""


def test_engine_runs_with_library_gemms_forbidden():
    """GDMAE_NO_LIBRARY=1 makes every product that would reach hipBLASLt fail.  The library reads the variable once per process, so
    the check runs compile + one engine call in a fresh child that has it set before anything is imported."""
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {**os.environ, "GDMAE_NO_LIBRARY": "1"}
    r = subprocess.run([sys.executable, "-c", _CHILD.format(repo=repo, pkg=os.path.join(repo, "gd-mae_amd"))], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "engine-ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_repeatable_and_frame_independent(compiled):
    net, ds, skw, eng = compiled
    bd = _batch(ds, skw)
    a, b = _engine_maps(eng, bd), _engine_maps(eng, bd)
    for k in QUANTITIES:
        assert torch.equal(a[k], b[k]), k
    pts = bd["points"]
    one = {"points": pts[pts[:, 0] == 0].contiguous(), "batch_size": 1}
    c = _engine_maps(eng, one)
    for k in QUANTITIES[1:]:
        # every kernel of the chain is row- / site-independent and the encoder's windows never span frames
        assert torch.equal(a[k][:1], c[k]), k


def test_engine_leaves_the_model_alone_and_training_is_unchanged(compiled):
    from gdmae_hip import inference, optim
    from pcdet.models import build_network, model_fn_decorator
    from tests_golden_boxes import synth_boxes
    net, ds, skw, eng = compiled
    bd = _batch(ds, skw)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    for _ in range(3):
        eng(dict(bd))
    after = net.state_dict()
    assert set(before) == set(after)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    # a training step after compile + use == the same step on a fresh model
    cfg, ds, skw = configs.named_config("D")
    B = 2
    pts = synth.synth_batch(77, B, ds.point_cloud_range, **skw)
    gt = synth_boxes(np.random.default_rng(5), B, 20, np.asarray(ds.point_cloud_range), 3)
    losses = []
    for use_engine in (False, True):
        torch.manual_seed(3)
        m = build_network(cfg, len(ds.class_names), ds, logging.getLogger("t")).to(_dev())
        if use_engine:
            m.eval()
            e2 = inference.compile_detector(m)
            e2({"points": torch.from_numpy(pts).to(_dev()), "batch_size": B})
        m.train()
        opt = optim.FlatAdamOneCycle(m, configs.optimization_cfg(B), total_steps=10)
        opt.zero_grad()
        ret = model_fn_decorator()(m, {"points": pts.copy(), "gt_boxes": gt.copy(), "batch_size": B})
        ret.loss.backward()
        opt.step(0)
        losses.append(float(ret.loss))
        if use_engine:
            m.eval()
            with pytest.raises(RuntimeError, match="refresh"):      # the flat optimizer stepped: the images are stale
                e2.head_maps({"points": torch.from_numpy(pts).to(_dev()), "batch_size": B})
    assert losses[0] == losses[1], losses
    eng.refresh()      # any FlatAdamOneCycle step marks every engine stale (optim.GENERATION): the shared fixture's too


def test_stale_images_raise_until_refresh():
    from gdmae_hip import inference
    net, ds, skw = _model(seed=4)
    eng = inference.compile_detector(net)
    bd = _batch(ds, skw)
    a = _engine_maps(eng, bd)
    with torch.no_grad():
        net.backbone_2d.conv_layer[0][1].running_mean.add_(0.5)
    with pytest.raises(RuntimeError, match="refresh"):
        eng(dict(bd))
    eng.refresh()
    b = _engine_maps(eng, bd)
    assert not torch.equal(a["hm"], b["hm"])
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    for p in net.parameters():
        p.grad = torch.ones_like(p) * 0.01
    opt.step()
    with pytest.raises(RuntimeError, match="refresh"):
        eng.head_maps(dict(bd))
    eng.refresh()
    assert all(torch.isfinite(v).all() for k, v in _engine_maps(eng, bd).items() if k != "voxel_coords")


def test_edge_batches(compiled):
    net, ds, skw, eng = compiled
    full = _batch(ds, skw)["points"]
    f0 = full[full[:, 0] == 0]
    outside = torch.tensor([[1, -500.0, 0.0, 0.0, 0.1]], device=_dev())          # frame 1: nothing inside the range
    single = torch.tensor([[0, 30.0, 1.0, -1.0, 0.3]], device=_dev())
    for pts, B in ((f0.contiguous(), 1), (torch.cat([f0, outside]).contiguous(), 2), (single, 1)):
        maps = eng.head_maps({"points": pts, "batch_size": B})
        for k, v in maps[0].items():
            assert v.shape[0] == B and torch.isfinite(v.float()).all(), k
        boxes, _ = eng({"points": pts, "batch_size": B})
        assert len(boxes) == B and all(b["pred_boxes"].shape[1] == 7 for b in boxes)


def test_refusals():
    from gdmae_hip import inference
    from pcdet.models import build_network
    cfg, ds, _ = configs.named_config("A")
    pre = build_network(cfg, 3, ds, logging.getLogger("t")).to(_dev()).eval()
    with pytest.raises(NotImplementedError, match="CenterPoint"):
        inference.compile_detector(pre)
    net, _, _ = _model()
    net.train()
    with pytest.raises(ValueError, match="evaluation mode"):
        inference.compile_detector(net)
    net.eval()
    net.backbone_2d.conv_layer[1][1] = torch.nn.BatchNorm2d(128, track_running_stats=False).to(_dev()).eval()
    with pytest.raises(NotImplementedError, match="running statistics"):
        inference.compile_detector(net)
