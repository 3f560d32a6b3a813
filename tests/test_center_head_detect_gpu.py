"""GPU: the batched CenterHead tail (``gdmae_center_head_detect``) against the op-by-op tail it reproduces
(``CenterHead.generate_predicted_boxes``; ``engine(batch_dict)``) on the same inputs.  Both run the same device functions for the
decode and the rotated IoU, so the expected result is equality (``torch.equal``): num[b] == len(pred), the rows below num[b] equal
pred_boxes / pred_scores / pred_labels, every row at or beyond num[b] is zero.

Scene condition (asserted, not assumed): inside one class segment no two valid candidates have the same rectified score, and the K-th
and (K + 1)-th heat-map scores differ - so neither the sort nor the top-K has a tie to break.  Planted logits come from a strictly
decreasing list spaced 1e-3 in [-2, 4]; the background and the dense maps are seeded permutations of a linspace.

IoU-aware config: r = s^(1 - a) q^a goes through powf in the kernel and torch.pow in the comparator.  Measured on an MI355X over the
two scenes below (the test prints it): largest |r - r_ref| = 0.0e+00 (MEASURED_POW_DEV): the two library calls agree bit for bit here;
asserted at 4 x that value, i.e. equality."""
import numpy as np
import pytest
import torch

from gdmae_hip import configs
from gdmae_hip import lib as L
from test_center_head_detect_cpu import _head, _ts_cfg

pytestmark = pytest.mark.gpu

MEASURED_POW_DEV = 0.0
B, H, W = 3, 48, 48
LOGITS = np.arange(4.0, -2.0, -1e-3)               # 6000 strictly decreasing planted logits, all above logit(0.1) = -2.197


def _dev():
    return torch.device("cuda:0")


class Scene:
    """Hand-built head maps: background below SCORE_THRESH (a seeded permutation of linspace(-12, -6)), 0.5 m axis-aligned boxes
    at the cell centres on the ground; ``plant`` raises one cell of one class and sets its regression values."""

    def __init__(self, seed, B=B, C=3, H=H, W=W, vel=False, iou=False):
        g = torch.Generator().manual_seed(seed)
        n = C * H * W
        self.pd = {"hm": torch.stack([torch.linspace(-12, -6, n)[torch.randperm(n, generator=g)].view(C, H, W) for _ in range(B)]),
                   "center": torch.full((B, 2, H, W), 0.5), "center_z": torch.zeros(B, 1, H, W),
                   "dim": torch.full((B, 3, H, W), float(np.log(0.5))), "rot": torch.zeros(B, 2, H, W)}
        self.pd["rot"][:, 0] = 1.0
        if vel:
            self.pd["vel"] = torch.randn(B, 2, H, W, generator=g)
        if iou:
            self.pd["iou"] = torch.rand(B, 1, H, W, generator=g) * 2 - 1
        self.next = 0

    def plant(self, b, c, y, x, size=None, z=None, logit=None):
        if logit is None:
            logit = LOGITS[self.next]
            self.next += 1
        self.pd["hm"][b, c, y, x] = float(logit)
        if size is not None:
            self.pd["dim"][b, :, y, x] = torch.tensor(np.log(np.asarray(size, dtype=np.float64)), dtype=torch.float32)
        if z is not None:
            self.pd["center_z"][b, 0, y, x] = z

    def plant_grid(self, b, c, count, step=3):
        """``count`` non-overlapping 0.5 m boxes of class c on every ``step``-th cell"""
        k = 0
        for y in range(0, H, step):
            for x in range(0, W, step):
                if k < count:
                    self.plant(b, c, y, x)
                    k += 1
        assert k == count

    def dev(self):
        return {k: v.to(_dev()) for k, v in self.pd.items()}


def dense_scene(seed, lo, hi, B=B, vel=False, iou=False):
    """Every cell random: logits a seeded permutation of linspace(lo, hi), boxes of 1 - 4 m x 0.8 - 2 m at random headings and
    offsets - heavily overlapping, so many pairs sit near the IoU thresholds."""
    s = Scene(seed, B=B, vel=vel, iou=iou)
    g = torch.Generator().manual_seed(seed + 1000)
    n = 3 * H * W
    s.pd["hm"] = torch.stack([torch.linspace(lo, hi, n)[torch.randperm(n, generator=g)].view(3, H, W) for _ in range(B)])
    s.pd["center"] = torch.rand(B, 2, H, W, generator=g)
    u = torch.rand(B, 3, H, W, generator=g)
    s.pd["dim"] = torch.log(torch.stack([1 + 3 * u[:, 0], 0.8 + 1.2 * u[:, 1], 1 + u[:, 2]], dim=1))
    ang = (torch.rand(B, H, W, generator=g) * 2 - 1) * np.pi
    s.pd["rot"] = torch.stack([torch.cos(ang), torch.sin(ang)], dim=1)
    s.pd["center_z"] = torch.rand(B, 1, H, W, generator=g) * 2 - 1
    return s


def candidates(head, pd, boundary_below_thresh_ok=False):
    """The comparator's candidates of every sample: (valid, global class, rectified score), computed as generate_predicted_boxes
    computes them; asserts the top-K boundary of the scene condition.  ``boundary_below_thresh_ok`` (the engine scenes, whose empty
    ground sits at one constant score below SCORE_THRESH): a K-th score equal to the (K + 1)-th is accepted when it is not above
    SCORE_THRESH - every cell tied with it is then discarded by both paths, whichever of them the top-K returns."""
    cfg = head.model_cfg.POST_PROCESSING
    nms = cfg.NMS_CONFIG
    hm = pd["hm"].float().sigmoid()
    Bn, C, Hh, Ww = hm.shape
    k = min(int(cfg.MAX_OBJ_PER_SAMPLE), C * Hh * Ww)
    score, cell = torch.topk(hm.reshape(Bn, -1), k + 1)
    differ = score[:, k - 1] != score[:, k]
    if boundary_below_thresh_ok:
        differ = differ | ~(score[:, k - 1] > float(cfg.SCORE_THRESH))
    assert bool(differ.all()), "scene condition: the K-th and (K + 1)-th heat-map scores are equal"
    score, cell = score[:, :k].contiguous(), cell[:, :k].contiguous()
    f = lambda name: pd[name].float().contiguous()   # noqa: E731
    dev = hm.device
    boxes = torch.empty(Bn, k, 9 if "vel" in pd else 7, dtype=torch.float32, device=dev)
    labels = torch.empty(Bn, k, dtype=torch.int32, device=dev)
    ious = torch.empty(Bn, k, dtype=torch.float32, device=dev)
    valid = torch.empty(Bn, k, dtype=torch.uint8, device=dev)
    L.call("gdmae_center_head_decode", L.ptr(cell), L.ptr(score), L.ptr(f("center")), L.ptr(f("center_z")), L.ptr(f("dim")), L.ptr(f("rot")),
           L.ptr(f("vel") if "vel" in pd else None), L.ptr(f("iou") if "iou" in pd else None), Bn, k, Hh, Ww,
           L.host_f32(list(head.point_cloud_range[:2])), L.host_f32(list(head.voxel_size[:2])), float(head.feature_map_stride),
           L.host_f32(list(cfg.POST_CENTER_LIMIT_RANGE)), float(cfg.SCORE_THRESH), 1, L.ptr(boxes), L.ptr(labels), L.ptr(ious), L.ptr(valid),
           L.stream())
    lab = labels.long()
    r = score
    if nms.NMS_TYPE == "multi_class_nms":
        a = score.new_tensor(list(nms.IOU_RECTIFIER))[lab]
        r = torch.pow(score, 1 - a) * torch.pow(ious, a)
    return valid.bool(), lab, r


def assert_scene_condition(head, pd, rel_gap=0.0, boundary_below_thresh_ok=False):
    """no two valid candidates of one class segment with equal r (or, with rel_gap, with r within that relative distance)"""
    valid, lab, r = candidates(head, pd, boundary_below_thresh_ok)
    aware = head.model_cfg.POST_PROCESSING.NMS_CONFIG.NMS_TYPE == "multi_class_nms"
    counts = []
    for b in range(valid.shape[0]):
        counts.append(int(valid[b].sum()))
        for c in (range(3) if aware else [None]):
            own = valid[b] if c is None else valid[b] & (lab[b] == c)
            v = torch.sort(r[b][own].double(), descending=True)[0]
            if v.numel() > 1:
                gap = (v[:-1] - v[1:]) / v[:-1].clamp_min(1e-30)
                assert float(gap.min()) > rel_gap, f"scene condition: sample {b} class {c}: two candidates with r within {float(gap.min()):.2e}"
    return counts


def compare(head, pd, score_tol=None):
    """batched == op-by-op, sample by sample; -> (padded output, comparator list, largest score deviation)"""
    Bn = pd["hm"].shape[0]
    with torch.no_grad():
        want = head.generate_predicted_boxes(Bn, [pd])
        out = head.generate_predicted_boxes_batched(Bn, [pd])
    num = out["num"].tolist()
    n_out = head.batched_rows(pd["hm"][0].numel())
    assert out["pred_boxes"].shape == (Bn, n_out, 9 if "vel" in pd else 7) and out["pred_scores"].shape == (Bn, n_out)
    assert out["pred_labels"].shape == (Bn, n_out) and out["pred_labels"].dtype == torch.int64 and out["num"].dtype == torch.int32
    dev = 0.0
    for b in range(Bn):
        n = num[b]
        assert n == want[b]["pred_boxes"].shape[0], (b, n, want[b]["pred_boxes"].shape[0])
        assert torch.equal(out["pred_labels"][b, :n], want[b]["pred_labels"]), b
        assert torch.equal(out["pred_boxes"][b, :n], want[b]["pred_boxes"]), b
        if score_tol is None:
            assert torch.equal(out["pred_scores"][b, :n], want[b]["pred_scores"]), b
        elif n:
            dev = max(dev, float((out["pred_scores"][b, :n] - want[b]["pred_scores"]).abs().max()))
        assert float(out["pred_boxes"][b, n:].abs().sum()) == 0 and float(out["pred_scores"][b, n:].abs().sum()) == 0
        assert int(out["pred_labels"][b, n:].abs().sum()) == 0
    if score_tol is not None:
        assert dev <= score_tol, (dev, score_tol)
    return out, want, dev


def ts_head(**post):
    """the gd_mae_ts head (class-aware, thresholds 0.7 / 0.55 / 0.55, rectifier 0), POST_PROCESSING / NMS_CONFIG entries edited"""
    cfg = _ts_cfg()
    for k, v in post.items():
        if k in cfg.POST_PROCESSING.NMS_CONFIG:
            cfg.POST_PROCESSING.NMS_CONFIG[k] = v
        else:
            cfg.POST_PROCESSING[k] = v
    return _head(cfg)


def agnostic_head():
    return _head(configs.center_head_cfg())


# ------------------------------------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------------------------------------
def small_scene():
    """sample 0: nothing above the threshold.  sample 1: a chain A > B > C of 4 x 2 m Vehicles 0.64 m apart (IoU(A, B) = IoU(B, C) =
    3.36 / 4.64 = 0.72 > 0.7, IoU(A, C) = 2.72 / 5.28 = 0.52), a Pedestrian and a Cyclist on the same spot, and a strong Vehicle
    above POST_CENTER_LIMIT_RANGE (center_z = 10).  sample 2: exactly one valid candidate."""
    s = Scene(11)
    s.plant(1, 0, 40, 5, size=(4, 2, 1.5), z=10.0)          # the best score of the sample, outside the range
    for x in (10, 12, 14):
        s.plant(1, 0, 10, x, size=(4, 2, 1.5))
    s.plant(1, 1, 30, 30, size=(1, 1, 1.7))
    s.plant(1, 2, 30, 30, size=(1, 1, 1.7))
    s.plant(2, 2, 7, 41)
    return s


def seam_scene():
    """sample 0: 65 Vehicles and 129 Pedestrians (one past a 64-bit word, one past two).  sample 1: exactly 64 valid candidates.
    sample 2: all K = 500 valid: 256 non-overlapping Vehicles (more than NMS_POST_MAXSIZE 200) and 244 Pedestrians."""
    s = Scene(12)
    s.plant_grid(0, 0, 65)
    s.plant_grid(0, 1, 129)
    s.plant_grid(1, 2, 64)
    s.plant_grid(2, 0, 256)
    s.plant_grid(2, 1, 244)
    return s


def test_small_scene_class_aware():
    head, pd = ts_head(), small_scene().dev()
    assert assert_scene_condition(head, pd) == [0, 5, 1]
    out, want, _ = compare(head, pd)
    assert out["num"].tolist() == [0, 4, 1]
    # A and C of the chain survive (B is suppressed by A and cannot suppress C); both boxes on the shared spot survive
    assert out["pred_labels"][1, :4].tolist() == [1, 1, 2, 3]
    x0 = lambda col: (col + 0.5) * 0.32   # noqa: E731
    assert torch.allclose(out["pred_boxes"][1, :2, 0].cpu(), torch.tensor([x0(10), x0(14)]), atol=1e-5)
    assert float(out["pred_scores"][1, 0]) > float(out["pred_scores"][1, 1])
    assert float(out["pred_boxes"][1, :4, 2].abs().max()) == 0          # the candidate at z = 10 is not among them


def test_small_scene_class_agnostic():
    head, pd = agnostic_head(), small_scene().dev()
    assert assert_scene_condition(head, pd) == [0, 5, 1]
    out, want, _ = compare(head, pd)
    assert out["num"].tolist() == [0, 3, 1]                              # the Cyclist on the Pedestrian's spot is lost
    assert sorted(out["pred_labels"][1, :3].tolist()) == [1, 1, 2]
    s = out["pred_scores"][1, :3]
    assert bool((s[:-1] > s[1:]).all())                                  # one list in descending score


@pytest.mark.parametrize("aware", [True, False])
def test_word_seams_exact_counts_and_post_max(aware):
    head, pd = (ts_head() if aware else agnostic_head()), seam_scene().dev()
    assert assert_scene_condition(head, pd) == [194, 64, 500]
    out, want, _ = compare(head, pd)
    if aware:
        assert out["num"].tolist() == [194, 64, 200 + 150]                 # sample 2: 256 -> 200 Vehicles, 244 -> 150 Pedestrians
        assert int((out["pred_labels"][2] == 1).sum()) == 200 and int((out["pred_labels"][2] == 2).sum()) == 150
    else:
        assert out["num"][1].item() == 64 and out["num"][2].item() < 500 and out["num"][0].item() < 194


def test_both_caps_bind():
    head = ts_head(NMS_PRE_MAXSIZE=[10, 5, 5], NMS_POST_MAXSIZE=[3, 2, 2], MAX_OBJ_PER_SAMPLE=40)
    assert head.batched_rows() == 7
    for scene in (seam_scene(), dense_scene(21, -12.0, -1.6)):
        pd = scene.dev()
        assert_scene_condition(head, pd)
        out, want, _ = compare(head, pd)
    assert out["num"].tolist() == [7, 7, 7]
    # NMS_PRE_MAXSIZE alone: 5 heavily overlapping candidates per class leave fewer than NMS_POST_MAXSIZE survivors somewhere
    head = ts_head(NMS_PRE_MAXSIZE=[10, 5, 5], NMS_THRESH=[0.05, 0.05, 0.05])
    compare(head, dense_scene(21, -12.0, -1.6).dev())


@pytest.mark.parametrize("aware", [True, False])
def test_dense_scene(aware):
    head, pd = (ts_head() if aware else agnostic_head()), dense_scene(22, -12.0, -1.6).dev()
    counts = assert_scene_condition(head, pd)
    assert all(200 <= c < 500 for c in counts), counts
    out, want, _ = compare(head, pd)
    assert all(0 < n < c for n, c in zip(out["num"].tolist(), counts))   # the NMS removes boxes in every sample


def test_1024_candidates():
    head, pd = ts_head(MAX_OBJ_PER_SAMPLE=1024), dense_scene(23, -12.0, -1.0).dev()
    counts = assert_scene_condition(head, pd)
    assert all(600 <= c <= 1024 for c in counts), counts
    assert head.batched_rows() == 500
    compare(head, pd)
    head = _head(configs.center_head_cfg())
    head.model_cfg.POST_PROCESSING.MAX_OBJ_PER_SAMPLE = 1024
    head.model_cfg.POST_PROCESSING.NMS_CONFIG.NMS_POST_MAXSIZE = 2000
    assert head.batched_rows() == 1024
    compare(head, pd)


def test_velocity_rows_are_carried_through():
    cfg = _ts_cfg()
    cfg.SEPARATE_HEAD_CFG.HEAD_ORDER = ['center', 'center_z', 'dim', 'rot', 'vel']
    cfg.SEPARATE_HEAD_CFG.HEAD_DICT['vel'] = {'out_channels': 2, 'num_conv': 2}
    head = _head(cfg)
    pd = dense_scene(24, -12.0, -1.6, vel=True).dev()
    assert_scene_condition(head, pd)
    out, want, _ = compare(head, pd)
    assert out["pred_boxes"].shape[2] == 9 and float(out["pred_boxes"][0, 0, 7:].abs().sum()) > 0


def _iou_head():
    return _head(configs.center_head_iou_cfg())


def iou_small_scene():
    """the scene of tests/test_center_head.py::test_iou_rectified_multi_class_nms_decode on this map: a same-class overlapping pair
    (4 x 2 m, one cell apart: IoU 0.85 > 0.8), two classes on neighbouring cells, iou values that clamp to 1 and to 0"""
    s = Scene(13, B=2, iou=True)
    for (b, c, y, x, logit, q) in ((0, 0, 20, 20, 3.0, 0.6), (0, 0, 20, 21, 2.0, None), (0, 1, 30, 30, 2.5, 3.0), (0, 2, 30, 31, 2.4, -3.0),
                                   (1, 2, 10, 40, 1.0, 0.0)):
        s.plant(b, c, y, x, size=(4.0, 2.0, 1.5), logit=logit)
        if q is not None:
            s.pd["iou"][b, 0, y, x] = q
    return s


def test_iou_rectified_scores():
    head = _iou_head()
    worst = 0.0
    # the dense scene: 137 candidates per sample (seed chosen so that no two rectified scores of a class are within 1e-5 relative:
    # the closest pair is 1.4e-4 apart; with the 397 candidates of the other dense scenes some pair always is)
    for scene in (iou_small_scene(), dense_scene(29, -12.0, -2.0, iou=True)):
        pd = scene.dev()
        assert_scene_condition(head, pd, rel_gap=1e-5)
        out, want, dev = compare(head, pd, score_tol=float("inf"))
        worst = max(worst, dev)
    print(f"rectified scores: largest |powf - torch.pow| deviation {worst:.3e}")
    assert worst <= 4 * MEASURED_POW_DEV, worst
    pd = iou_small_scene().dev()
    out = head.generate_predicted_boxes_batched(2, [pd])
    assert out["num"].tolist() == [3, 1] and out["pred_labels"][0, :3].tolist() == [1, 2, 3]
    assert float(out["pred_scores"][0, 2]) == 0.0                        # the Cyclist's iou clamps to 0; it keeps its place


def test_repeatable_and_independent_of_the_batch():
    head, pd = ts_head(), dense_scene(22, -12.0, -1.6).dev()
    a = head.generate_predicted_boxes_batched(B, [pd])
    b = head.generate_predicted_boxes_batched(B, [pd])
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for s in range(B):
        one = head.generate_predicted_boxes_batched(1, [{k: v[s:s + 1].contiguous() for k, v in pd.items()}])
        for k in a:
            assert torch.equal(one[k][0], a[k][s]), (s, k)


def test_no_host_read():
    head, pd = ts_head(), small_scene().dev()
    head.generate_predicted_boxes_batched(B, [pd])
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    control = False
    try:
        torch.cuda.set_sync_debug_mode("error")
        out = head.generate_predicted_boxes_batched(B, [pd])
        try:
            head.generate_predicted_boxes(B, [pd])
        except RuntimeError:
            control = True
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    if not control:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on the op-by-op tail's host reads in this torch build")
    assert out["num"].tolist() == [0, 4, 1]


def test_library_refusals():
    """K > 1024, C > 8 and a negative threshold are error returns (nothing is launched)."""
    dev = _dev()
    z = lambda *s: torch.zeros(*s, device=dev)   # noqa: E731

    def call(K=4, C=3, thresh=(0.7, 0.5, 0.5), n_out=4):
        Kw = min(K, 1024)
        t = [torch.zeros(1, K, dtype=torch.int64, device=dev), z(1, K), z(1, 2, 4, 4), z(1, 1, 4, 4), z(1, 3, 4, 4), z(1, 2, 4, 4),
             z(1, n_out, 7), z(1, n_out), torch.zeros(1, n_out, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
             torch.empty(max(int(L.load().gdmae_center_head_detect_workspace_bytes(1, Kw, 7)), 256), dtype=torch.uint8, device=dev)]
        pad = lambda v, fill: list(v) + [fill] * (16 - len(v))   # noqa: E731
        L.call("gdmae_center_head_detect", *[L.ptr(x) for x in t[:6]], None, None, 1, K, 4, 4, L.host_f32([0, 0]), L.host_f32([1, 1]), 1.0,
               L.host_f32([-9, -9, -9, 9, 9, 9]), 0.1, 1, C, L.host_f32(pad(thresh, 0.5)), L.host_i32(pad([10] * 3, 10)),
               L.host_i32(pad([10] * 3, 10)), L.host_f32(pad([0.0] * 3, 0.0)), L.host_i32(pad(range(3), 0)), 1, n_out,
               *[L.ptr(x) for x in t[6:]], L.stream())
        torch.cuda.synchronize()
    call()
    with pytest.raises(L.GdmaeHipError, match="1024"):
        call(K=1025)
    with pytest.raises(L.GdmaeHipError, match="classes"):
        call(C=9)
    with pytest.raises(L.GdmaeHipError, match="negative NMS threshold"):
        call(thresh=(0.7, -0.1, 0.5))
    with pytest.raises(L.GdmaeHipError, match="n_out"):
        call(n_out=3)


# ------------------------------------------------------------------------------------------------------------------------------
# engines (the small models of tests/test_inference_engine.py and tests/test_inference_engine_two_stage.py, built as those files do)
# ------------------------------------------------------------------------------------------------------------------------------
def test_centerpoint_engine_detect_equals_the_engine_call():
    from gdmae_hip import inference
    from test_inference_engine import _batch, _model
    net, ds, skw = _model()
    eng = inference.compile_detector(net)
    bd = _batch(ds, skw)
    preds, _ = eng(dict(bd))
    out = eng.detect(dict(bd))
    got = net.dense_head.padded_to_pred_dicts(out)
    assert out["pred_boxes"].shape[1] == net.dense_head.batched_rows() and sum(out["num"].tolist()) > 0
    for b in range(bd["batch_size"]):
        for k in ("pred_boxes", "pred_scores", "pred_labels"):
            assert torch.equal(got[b][k], preds[b][k]), (b, k)
        n = int(out["num"][b])
        assert float(out["pred_boxes"][b, n:].abs().sum()) == 0 and int(out["pred_labels"][b, n:].abs().sum()) == 0


TWO_STAGE_HM_SPREAD = 400.0


def two_stage_scene(cloud_seed=31, spread=TWO_STAGE_HM_SPREAD):
    """The model, the cloud (seed 31) and the heat-map calibration of tests/test_inference_engine_two_stage.py (its ``_model`` and the
    recipe of its ``scene`` fixture: final 1 x 1 heat-map weights along the direction in which busy cells differ from empty ground, the
    60 densest cells above SCORE_THRESH), with one difference: the length of that weight vector is 400 instead of 50.  The engine's
    head maps are bf16, and at 50 the logits of the ~60 busy cells crowd into so few bf16 values that two candidates of one class
    share a score in every cloud tried (seeds 31 - 40 at 50, eight of ten at 150, four of ten at 400) - a tie that ``torch.sort`` in
    the op-by-op tail and the top-K position in the batched tail are free to break differently (in every probed scene without a tie
    the RoIs of the two tails were bit-equal; they differed only in scenes with one).  The test asserts that this scene has none."""
    from gdmae_hip import inference, synth
    from test_inference_engine_two_stage import _model
    net, ds = _model()
    Bn = 2
    pts = synth.synth_batch(cloud_seed, Bn, ds.point_cloud_range, beams=16, azimuths=1100, extra=3000, features=5)
    points = torch.from_numpy(pts).cuda()
    with torch.no_grad():
        d = {"points": points, "batch_size": Bn}
        for m in net.module_list[:3]:
            d = m(d)
        sep = net.dense_head.heads_list[0]
        act = sep.hm[0](net.dense_head.shared_conv(d["spatial_features_2d"].float()))
        Hh, Ww = act.shape[2:]
        r0, vs = ds.point_cloud_range, ds.voxel_size
        cx = ((points[:, 1] - float(r0[0])) / vs[0]).long().clamp(0, Ww - 1)
        cy = ((points[:, 2] - float(r0[1])) / vs[1]).long().clamp(0, Hh - 1)
        cnt = torch.bincount((points[:, 0].long() * Hh + cy) * Ww + cx, minlength=Bn * Hh * Ww).view(Bn, 1, Hh, Ww).float()
        busy = torch.nn.functional.avg_pool2d(cnt, 9, stride=1, padding=4) * 81 >= 20
        far = torch.nn.functional.avg_pool2d(cnt, 41, stride=1, padding=20) == 0
        far[:, :, :24], far[:, :, -24:], far[:, :, :, :24], far[:, :, :, -24:] = False, False, False, False
        a0 = act.permute(0, 2, 3, 1)[far[:, 0]].double().median(0)[0]
        u = act.permute(0, 2, 3, 1)[busy[:, 0]].double().mean(0) - a0
        u = u - (u @ a0) * a0 / (a0 @ a0)
        w = (spread * u / u.norm() * torch.tensor([1.0, 0.9, 0.8], dtype=torch.float64, device=u.device)[:, None]).float()
        final = sep.hm[-1]
        final.weight.zero_()
        final.weight[:, :, 1, 1] = w
        kth = torch.topk(torch.einsum("bchw,kc->bkhw", act, w).reshape(-1), 60)[0][-1]
        thr = net.dense_head.model_cfg.POST_PROCESSING.SCORE_THRESH
        final.bias.fill_(float(np.log(thr / (1 - thr))) - float(kth))
    return {"net": net, "points": points, "engine": inference.compile_detector(net)}


def test_graphrcnn_engine_detect_equals_the_engine_call():
    from gdmae_hip import inference
    scene = two_stage_scene()
    eng, head = scene["engine"], scene["net"].dense_head
    bd = {"points": scene["points"], "batch_size": 2}
    counts = assert_scene_condition(head, eng.head_maps(dict(bd))[0], boundary_below_thresh_ok=True)
    assert all(c > 0 for c in counts), counts
    preds, _ = eng(dict(bd))
    prop = eng.proposals(dict(bd))
    out = eng.detect(dict(bd))
    M = prop["rois"].shape[1]
    first = inference.CenterPointEngine.detect(eng, dict(bd))
    print(f"two-stage detect: candidates {counts}, M {M}, first-stage counts {first['num'].tolist()}, "
          f"RoIs equal {torch.equal(first['pred_boxes'][:, :M], prop['rois'])}, "
          f"RoI scores equal {torch.equal(first['pred_scores'][:, :M], prop['roi_scores'])}")
    assert out["pred_boxes"].shape == (2, M, 7) and out["pred_scores"].shape == (2, M) and out["pred_labels"].shape == (2, M)
    assert torch.equal(out["pred_labels"], prop["roi_labels"])
    for b in range(2):
        ok = out["pred_labels"][b] != 0
        assert int(out["num"][b]) == int(ok.sum()) > 0
        assert torch.equal(out["pred_boxes"][b][ok], preds[b]["pred_boxes"])
        assert torch.equal(out["pred_scores"][b][ok], preds[b]["pred_scores"])
        assert torch.equal(out["pred_labels"][b][ok], preds[b]["pred_labels"])
        assert float(out["pred_boxes"][b][~ok].abs().sum()) == 0 and float(out["pred_scores"][b][~ok].abs().sum()) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_strided_maps_decode_like_their_contiguous_copies(dtype):
    """The head's convolutions leave every map as a channel slice of a wider channels-last map (bf16 under autocast), so both tails
    first make fp32 contiguous copies.  The copies have to live until the launch is issued: taken as temporaries inside the argument
    list, the copy of `center` went back to the caching allocator once its address was read and the copy of `center_z` was written
    over it before the kernel ran (with an emptied cache, as here, always; in a long-running process depending on which blocks were
    free).  Contiguous fp32 maps need no copies: their result is the reference."""
    head, pd = ts_head(), dense_scene(41, -3.0, 3.0, iou=True).dev()
    pd = {k: v.to(dtype).float() for k, v in pd.items()}                    # values both dtypes hold exactly

    def strided(m):
        wide = torch.zeros(m.shape[0], m.shape[2], m.shape[3], 32, dtype=dtype, device=m.device)
        wide[..., :m.shape[1]] = m.permute(0, 2, 3, 1).to(dtype)
        v = wide[..., :m.shape[1]].permute(0, 3, 1, 2)
        assert not v.is_contiguous() and torch.equal(v.float(), m)
        return v

    views = {k: strided(v) for k, v in pd.items()}
    Bn = pd["hm"].shape[0]
    with torch.no_grad():
        want = head.generate_predicted_boxes(Bn, [pd])
        want_b = head.generate_predicted_boxes_batched(Bn, [pd])
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        got = head.generate_predicted_boxes(Bn, [views])
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        got_b = head.generate_predicted_boxes_batched(Bn, [views])
    assert sum(w["pred_boxes"].shape[0] for w in want) > 50
    for b in range(Bn):
        for k in ("pred_boxes", "pred_scores", "pred_labels"):
            assert torch.equal(got[b][k], want[b][k]), (b, k)
    for k in want_b:
        assert torch.equal(got_b[k], want_b[k]), k
