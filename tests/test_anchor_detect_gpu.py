"""GPU: the batched anchor-head tail (``gdmae_anchor_detect``) against the pieces of the op-by-op tail it reproduces.
Boxes, scores and labels are copies of the inputs and the IoU decisions are taken by the ``bev_iou`` that ``gdmae_nms_bev`` uses, so
every comparison is ``torch.equal``; nothing here has a tolerance.

Comparator A (``comparator_a``), the contract with its tie rule: per sample a STABLE descending sort of the valid scores (equal scores
keep their row order), the first NMS_PRE_MAXSIZE of it, ``gdmae_nms_bev`` on those boxes, the first NMS_POST_MAXSIZE kept ones, rows
with label 0 dropped.  Comparator B is ``Detector3DTemplate.finish_sample`` itself; ``torch.topk`` and the sort inside ``nms_gpu``
leave ties unspecified, so it is only used where the test asserts that the scores are pairwise distinct."""
import numpy as np
import pytest
import torch

from gdmae_hip import lib as L
from test_anchor_detect_cpu import _model as _cpu_model

pytestmark = pytest.mark.gpu

B, A = 3, 9000
THRESH = 0.1


def _dev():
    return torch.device("cuda:0")


class Scene:
    """Crafted survivors of the anchor head: per sample ``A`` rows of pairwise distinct scores (a seeded permutation of
    linspace(0.05, 0.95, A)), labels 1 .. 3, boxes of 1 - 4 m x 0.8 - 2 m at random headings in a ``field`` x ``field`` metre square
    (40 m: heavily overlapping).  ``count`` says how many rows of a sample are valid."""

    def __init__(self, seed, counts, A=A, field=40.0):
        g = torch.Generator().manual_seed(seed)
        Bn = len(counts)
        self.A = A
        self.count = torch.tensor(counts, dtype=torch.int32)
        self.score = torch.stack([torch.linspace(0.05, 0.95, A)[torch.randperm(A, generator=g)] for _ in range(Bn)])
        self.label = torch.randint(1, 4, (Bn, A), generator=g, dtype=torch.int32)
        u = torch.rand(Bn, A, 7, generator=g)
        self.box = torch.stack([u[..., 0] * field, u[..., 1] * field, u[..., 2] * 2 - 1, 1 + 3 * u[..., 3], 0.8 + 1.2 * u[..., 4],
                                1 + u[..., 5], (u[..., 6] * 2 - 1) * np.pi], dim=-1)

    def dev(self):
        return tuple(t.contiguous().to(_dev()) for t in (self.count, self.score, self.label, self.box))


def detect(count, score, label, box, pre_max, post_max, thresh=THRESH, n_out=None):
    """the library entry, outputs pre-filled with canaries -> dict"""
    Bn, An = score.shape
    dev = score.device
    n_out = min(pre_max, post_max) if n_out is None else n_out
    o = {"pred_boxes": torch.full((Bn, n_out, 7), float("nan"), device=dev), "pred_scores": torch.full((Bn, n_out), float("nan"), device=dev),
         "pred_labels": torch.full((Bn, n_out), -7, dtype=torch.int64, device=dev), "num": torch.full((Bn,), -7, dtype=torch.int32, device=dev)}
    ws = torch.empty(max(int(L.load().gdmae_anchor_detect_workspace_bytes(Bn, pre_max)), 256), dtype=torch.uint8, device=dev)
    L.call("gdmae_anchor_detect", L.ptr(count), L.ptr(score), L.ptr(label), L.ptr(box), Bn, An, pre_max, post_max, float(thresh), n_out,
           L.ptr(o["pred_boxes"]), L.ptr(o["pred_scores"]), L.ptr(o["pred_labels"]), L.ptr(o["num"]), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    return o


def comparator_a(count, score, label, box, pre_max, post_max, thresh=THRESH):
    """-> (per-sample list of pred dicts, per-sample number of boxes the NMS kept before the NMS_POST_MAXSIZE cut)"""
    dev = score.device
    preds, kept_all = [], []
    for b, n in enumerate(count.tolist()):
        order = torch.sort(score[b, :n], descending=True, stable=True)[1][:pre_max]
        m = int(order.numel())
        kept = torch.zeros(0, dtype=torch.int64, device=dev)
        if m:
            bx = box[b][order].contiguous()
            keep = torch.empty(m, dtype=torch.int64, device=dev)
            nk = torch.empty(1, dtype=torch.int32, device=dev)
            ws = torch.empty(int(L.load().gdmae_nms_workspace_bytes(m)), dtype=torch.uint8, device=dev)
            L.call("gdmae_nms_bev", L.ptr(bx), m, float(thresh), 1, L.ptr(keep), L.ptr(nk), L.ptr(ws), L.stream())
            kept = keep[:int(nk)]
        kept_all.append(int(kept.numel()))
        sel = order[kept[:post_max]]
        lab = label[b][sel].long()
        ok = lab != 0
        preds.append({"pred_boxes": box[b][sel][ok], "pred_scores": score[b][sel][ok], "pred_labels": lab[ok]})
    return preds, kept_all


def check(out, want, n_out):
    """padded output == per-sample list: shapes, dtypes, bits, zero padding"""
    Bn = len(want)
    assert out["pred_boxes"].shape == (Bn, n_out, 7) and out["pred_scores"].shape == (Bn, n_out) and out["pred_labels"].shape == (Bn, n_out)
    assert out["pred_boxes"].dtype == torch.float32 and out["pred_scores"].dtype == torch.float32
    assert out["pred_labels"].dtype == torch.int64 and out["num"].dtype == torch.int32 and out["num"].shape == (Bn,)
    num = out["num"].tolist()
    for b in range(Bn):
        n = num[b]
        assert n == want[b]["pred_boxes"].shape[0], (b, n, want[b]["pred_boxes"].shape[0])
        for k in ("pred_boxes", "pred_scores", "pred_labels"):
            assert want[b][k].dtype == out[k].dtype and torch.equal(out[k][b, :n], want[b][k]), (b, k)
        assert torch.equal(out["pred_boxes"][b, n:], torch.zeros(n_out - n, 7, device=_dev())), b
        assert torch.equal(out["pred_scores"][b, n:], torch.zeros(n_out - n, device=_dev())), b
        assert torch.equal(out["pred_labels"][b, n:], torch.zeros(n_out - n, dtype=torch.int64, device=_dev())), b
    return num


def same(a, b):
    for k in a:
        assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k], b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), k


# ------------------------------------------------------------------------------------------------------------------------------
# the library entry on crafted survivors
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [(0, 1, 64), (65, 129, 4096), (4097, A, 0)])
def test_counts_at_the_seams(counts):
    """nothing, one row, one 64-bit word and one past it, one past two words, exactly NMS_PRE_MAXSIZE (the sort path at its largest),
    one more (the selection path at its smallest), every row"""
    t = Scene(31 + counts[0], counts).dev()
    out = detect(*t, 4096, 500)
    want, kept = comparator_a(*t, 4096, 500)
    num = check(out, want, 500)
    for c, n in zip(counts, num):
        if c <= 1:
            assert n == c
        elif c < 129:
            assert 0 < n <= c, (c, n)
        else:
            assert 0 < n < min(c, 4096), (c, n)                              # the dense field: the NMS removes boxes


def test_seventy_thousand_rows():
    """count = A = 70,000 in one sample: several steps of every selection pass, rows beyond 65,536"""
    t = Scene(41, (70000, 4097, 1), A=70000).dev()
    out = detect(*t, 4096, 500)
    want, _ = comparator_a(*t, 4096, 500)
    num = check(out, want, 500)
    assert 0 < num[0] < 4096 and num[2] == 1
    top = torch.sort(t[1][0], descending=True, stable=True)[1][:4096]
    assert int(top.max()) > 65536                                          # rows beyond 2^16 are among the selected ones


def test_chain_known_answer():
    """A > B > C by score, 4 x 2 m boxes 0.64 m apart: IoU(A, B) = IoU(B, C) = 6.72 / 9.28 = 0.72, IoU(A, C) = 5.44 / 10.56 = 0.52.
    At a threshold of 0.6 A suppresses B, B cannot suppress C any more: A and C are kept, and the far box D."""
    s = Scene(51, (4, 0, 1))
    rows = {"C": (0, 10.0 + 1.28, 0.5), "A": (1, 10.0, 0.9), "B": (2, 10.0 + 0.64, 0.7), "D": (3, 30.0, 0.6)}
    for name, (r, x, sc) in rows.items():
        s.box[0, r] = torch.tensor([x, 10.0, 0.0, 4.0, 2.0, 1.5, 0.0])
        s.score[0, r] = sc
        s.label[0, r] = 1 + r % 3
    t = s.dev()
    out = detect(*t, 4096, 500, thresh=0.6)
    assert out["num"].tolist() == [3, 0, 1]
    assert out["pred_scores"][0, :3].tolist() == [float(np.float32(0.9)), float(np.float32(0.6)), float(np.float32(0.5))]      # A, D, C
    assert out["pred_labels"][0, :3].tolist() == [2, 1, 1]
    assert out["pred_boxes"][0, :3, 0].tolist() == [10.0, 30.0, float(np.float32(11.28))]
    want, _ = comparator_a(*t, 4096, 500, thresh=0.6)
    check(out, want, 500)


def test_both_caps_bind():
    # NMS_PRE_MAXSIZE 10 of 40 candidates, NMS_POST_MAXSIZE 3; a sparse field (200 m), so that more than 3 of the 10 survive
    t = Scene(61, (40, 40, 40), field=200.0).dev()
    out = detect(*t, 10, 3)
    want, kept = comparator_a(*t, 10, 3)
    assert check(out, want, 3) == [3, 3, 3] and all(3 < k <= 10 for k in kept), kept
    lowest = torch.sort(t[1][:, :40], descending=True)[0][:, 9]
    assert bool((out["pred_scores"] >= lowest[:, None]).all())              # nothing from beyond the 10 best
    # the dense field: NMS_PRE_MAXSIZE binds alone somewhere
    t = Scene(62, (40, 40, 40), field=2.0).dev()
    out = detect(*t, 10, 3)
    want, kept = comparator_a(*t, 10, 3)
    num = check(out, want, 3)
    assert min(num) < 3, num
    # the shipped caps: 4096 / 500 with more than 500 survivors of the NMS
    t = Scene(63, (A, 4096, 5000), field=200.0).dev()
    out = detect(*t, 4096, 500)
    want, kept = comparator_a(*t, 4096, 500)
    assert check(out, want, 500) == [500, 500, 500] and all(500 < k < 4096 for k in kept), kept


def tie_scene():
    """Comparator A only.  Sample 0 (6000 rows, the selection path), over a seeded permutation of its rows: 4000 rows above the cut in
    2000 PAIRS of equal scores, the second box of a pair 0.3 m beside the first (IoU > 0.1: which of the two survives is the tie
    rule); then 300 rows at exactly 0.5 (with NMS_PRE_MAXSIZE 4096 the cut takes the first 96 of them in row order); distinct scores
    below.  Samples 1 and 2 (4096 and 700 rows, the sort path): the same pattern with 1998 / 300 pairs and what is left of the run.
    A 150 m field, so that rows of the run survive the NMS."""
    counts = (6000, 4096, 700)
    s = Scene(71, counts, field=150.0)
    g = torch.Generator().manual_seed(72)
    for b, c in enumerate(counts):
        perm = torch.randperm(c, generator=g)
        pairs = min(2000, c // 2 - 50)
        hi = torch.linspace(0.6, 0.95, pairs)
        first, second = perm[:pairs], perm[pairs:2 * pairs]
        s.score[b, first], s.score[b, second] = hi, hi
        s.box[b, second] = s.box[b, first]
        s.box[b, second, 0] += 0.3
        run = perm[2 * pairs:2 * pairs + 300]
        s.score[b, run] = 0.5
        rest = perm[2 * pairs + 300:]
        s.score[b, rest] = torch.linspace(0.05, 0.45, max(int(rest.numel()), 1))[:rest.numel()]
    return s


def test_ties_go_to_the_earlier_row():
    t = tie_scene().dev()
    count, score = t[0], t[1]
    assert int((score[0, :6000] > 0.5).sum()) == 4000 and int((score[0, :6000] == 0.5).sum()) == 300      # the run straddles the cut
    out = detect(*t, 4096, 500)
    want, kept = comparator_a(*t, 4096, 500)
    num = check(out, want, 500)
    assert all(0 < n for n in num)
    # without the NMS_POST_MAXSIZE cut: rows of the run at the NMS_PRE_MAXSIZE cut are among the output
    out = detect(*t, 4096, 4096)
    want, _ = comparator_a(*t, 4096, 4096)
    check(out, want, 4096)
    for b in range(3):
        sc = out["pred_scores"][b, :int(out["num"][b])]
        assert bool((sc[:-1] >= sc[1:]).all())
    n0 = int(out["num"][0])
    run_rows = (score[0, :6000] == 0.5).nonzero().view(-1)[:96]            # the 96 rows of the run the contract lets in
    emitted = out["pred_boxes"][0, :n0][out["pred_scores"][0, :n0] == 0.5]
    assert emitted.shape[0] > 0
    allowed = t[3][0][run_rows]
    assert all(bool((allowed == e).all(dim=1).any()) for e in emitted)


def test_distinct_scores_equal_finish_sample():
    """pairwise distinct scores (asserted): comparators A and B both apply, through the model's ``finish_batch``"""
    model = _cpu_model()
    cfg = model.model_cfg.POST_PROCESSING.NMS_CONFIG
    pre, post, thr = int(cfg.NMS_PRE_MAXSIZE), int(cfg.NMS_POST_MAXSIZE), float(cfg.NMS_THRESH)
    assert (pre, post) == (4096, 500)
    counts = (5000, 300, 4096)
    t = Scene(81, counts).dev()
    count, score, label, box = t
    for b, c in enumerate(counts):
        assert int(torch.unique(score[b, :c]).numel()) == c
    out = model.finish_batch(*t)
    want_a, _ = comparator_a(*t, pre, post, thr)
    num = check(out, want_a, model.batched_rows())
    assert all(0 < n < min(c, pre) for n, c in zip(num, counts)), num
    want_b = []
    with torch.no_grad():
        for b, c in enumerate(counts):
            want_b.append(model.finish_sample(box[b, :c], score[b, :c], label[b, :c].long(), {}, b, {"batch_size": 3})[0])
    check(out, want_b, 500)
    got = model.padded_to_pred_dicts(out)
    for a, w in zip(got, want_b):
        for k in w:
            assert a[k].dtype == w[k].dtype and torch.equal(a[k], w[k]), k


def test_rows_behind_the_count_are_never_read():
    counts = (5000, 300, 0)
    s = Scene(91, counts)
    t = s.dev()
    ref = detect(*t, 4096, 500)
    count, score, label, box = (x.clone() for x in t)
    for b, c in enumerate(counts):
        for k, v in enumerate((float("nan"), float("inf"), 2.0)):
            score[b, c + k::3] = v
        box[b, c:] = 1e30
        box[b, c::2, 3:6] = float("inf")
        label[b, c:] = 0
    out = detect(count, score, label, box, 4096, 500)
    same(ref, out)
    assert 0 < int(ref["num"][0]) < 4096 and 0 < int(ref["num"][1]) < 300 and int(ref["num"][2]) == 0


def test_label_zero_rows_leave_behind_the_post_max_cut():
    """X0 (label 0, best score) overlaps X1 (second best): X1 is suppressed.  X2, X3, X4 stand apart.  NMS_POST_MAXSIZE 3 keeps X0, X2,
    X3; X0 is then dropped: the output is X2, X3 (not X1, which X0 suppressed; not X4, whose place X0 took) and num = 2."""
    s = Scene(101, (5, 5, 0), field=1000.0)
    for b in range(2):
        for r, (x, sc) in enumerate(((10.0, 0.9), (10.3, 0.8), (30.0, 0.7), (50.0, 0.6), (70.0, 0.5))):
            row = 4 - r                                                     # the rows are in ascending score
            s.box[b, row] = torch.tensor([x, 10.0, 0.0, 4.0, 2.0, 1.5, 0.0])
            s.score[b, row] = sc
            s.label[b, row] = 0 if r == 0 and b == 0 else 2
    t = s.dev()
    out = detect(*t, 10, 3)
    assert out["num"].tolist() == [2, 3, 0]
    assert out["pred_boxes"][0, :2, 0].tolist() == [30.0, 50.0] and out["pred_labels"][0].tolist() == [2, 2, 0]
    assert out["pred_boxes"][1, :3, 0].tolist() == [10.0, 30.0, 50.0]       # the same sample with label 2 on X0
    want, _ = comparator_a(*t, 10, 3)
    check(out, want, 3)


def test_repeatable_and_independent_of_the_batch():
    t = Scene(111, (5000, 300, 4096)).dev()
    a, b = detect(*t, 4096, 500), detect(*t, 4096, 500)
    same(a, b)
    for s in range(3):
        one = detect(*(x[s:s + 1].contiguous() for x in t), 4096, 500)
        for k in a:
            assert torch.equal(one[k][0], a[k][s]), (s, k)


def test_no_host_read():
    model = _cpu_model()
    t = Scene(121, (5000, 300, 0)).dev()
    want = model.finish_batch(*t)["num"].tolist()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    control = False
    try:
        torch.cuda.set_sync_debug_mode("error")
        out = model.finish_batch(*t)
        try:
            t[0].tolist()                                                  # the host read the op-by-op tail starts with
        except RuntimeError:
            control = True
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert control, "torch.cuda.set_sync_debug_mode('error') did not raise on a host read: the check above proves nothing"
    assert out["num"].tolist() == want and want[2] == 0 and want[0] > 0


def test_library_refusals():
    """each is an error return: nothing is launched, the outputs keep their canaries"""
    t = Scene(131, (5, 5, 5), A=16).dev()
    ok = detect(*t, 10, 3)
    assert min(ok["num"].tolist()) > 0
    for kw, match in ((dict(pre_max=4097, post_max=500), "NMS_PRE_MAXSIZE"), (dict(pre_max=0, post_max=500, n_out=1), "NMS_PRE_MAXSIZE"),
                      (dict(pre_max=10, post_max=0, n_out=1), "NMS_POST_MAXSIZE"), (dict(pre_max=10, post_max=3, thresh=-0.1), "threshold"),
                      (dict(pre_max=10, post_max=3, thresh=float("nan")), "threshold"), (dict(pre_max=10, post_max=3, n_out=10), "n_out"),
                      (dict(pre_max=10, post_max=30, n_out=30), "n_out")):
        with pytest.raises(L.GdmaeHipError, match=match):
            detect(*t, **kw)
    dev = _dev()
    o = [torch.zeros(3, 3, 7, device=dev), torch.zeros(3, 3, device=dev), torch.zeros(3, 3, dtype=torch.int64, device=dev),
         torch.full((3,), -7, dtype=torch.int32, device=dev), torch.empty(4096, dtype=torch.uint8, device=dev)]

    def args(Bn=3, An=16, skip=None):
        ptrs = [None if skip == i else L.ptr(x) for i, x in enumerate(list(t) + o)]
        return ptrs[:4] + [Bn, An, 10, 3, 0.1, 3] + ptrs[4:] + [L.stream()]
    for kw, match in ((dict(Bn=0), "sizes"), (dict(An=0), "sizes"), (dict(skip=0), "null"), (dict(skip=3), "null"), (dict(skip=7), "null"),
                      (dict(skip=8), "null")):
        with pytest.raises(L.GdmaeHipError, match=match):
            L.call("gdmae_anchor_detect", *args(**kw))
    torch.cuda.synchronize()
    assert o[3].tolist() == [-7, -7, -7]


# ------------------------------------------------------------------------------------------------------------------------------
# engine (the model and the batch of tests/test_inference_engine_kitti.py)
# ------------------------------------------------------------------------------------------------------------------------------
def _head_output(eng, bd):
    with torch.no_grad(), torch.autocast("cuda", enabled=False):
        x2 = eng._trunk(dict(bd))[1]
        return eng._head(x2, False)[:4]


def test_engine_detect_is_comparator_a_on_the_head_output():
    """the seeded model: about a third of the 321,408 anchors of a sample survive SCORE_THRESH, so the selection path runs at full size"""
    from gdmae_hip import inference
    from test_inference_engine_kitti import _batch, _model
    net, ds = _model()
    eng = inference.compile_detector(net)
    bd = _batch(ds)
    nms = net.model_cfg.POST_PROCESSING.NMS_CONFIG
    out = eng.detect(dict(bd))
    t = _head_output(eng, bd)
    counts = t[0].tolist()
    print(f"anchor engine detect: survivors per sample {counts} of {t[1].shape[1]}, boxes {out['num'].tolist()}")
    assert all(c > 4096 for c in counts)
    want, _ = comparator_a(*t, int(nms.NMS_PRE_MAXSIZE), int(nms.NMS_POST_MAXSIZE), float(nms.NMS_THRESH))
    num = check(out, want, net.batched_rows())
    assert all(n > 0 for n in num)
    got = net.padded_to_pred_dicts(out)
    assert len(got) == 2
    for a, w in zip(got, want):
        assert set(a) == set(w) == {"pred_boxes", "pred_scores", "pred_labels"}
        for k in w:
            assert a[k].dtype == w[k].dtype and a[k].shape == w[k].shape and torch.equal(a[k], w[k]), k


# The seeded model's map is mostly its constant background: in every cloud probed (seeds 77 - 86 of ``_batch``) at least 4000 anchors of a
# sample share ONE score, 0.34423375129699707, and 3 to 25 anchors lie above it, pairwise distinct.  A threshold that leaves fewer than
# 4096 anchors without a tie therefore sits just above that value.  Seed 82 has the most anchors above it in both samples (measured on an
# MI355X: 25 and 13; seed 77: 16 and 3, seed 81: 3 and 25, seeds 78, 83, 84, 86: 3 in at least one sample).
TIE_FREE_SEED, TIE_FREE_THRESH, TIE_FREE_COUNTS = 82, 0.34424, [25, 13]


def test_engine_detect_equals_the_engine_call_on_a_tie_free_scene():
    from gdmae_hip import inference
    from test_inference_engine_kitti import _batch, _model

    def edit(cfg):
        cfg.POST_PROCESSING.SCORE_THRESH = TIE_FREE_THRESH
    net, ds = _model(cfg_edit=edit)
    eng = inference.compile_detector(net)
    bd = _batch(ds, seed=TIE_FREE_SEED)
    count, score, label, box = _head_output(eng, bd)
    counts = count.tolist()
    print(f"tie-free engine scene: survivors per sample {counts}")
    assert counts == TIE_FREE_COUNTS and all(0 < c < 4096 for c in counts)
    for b, c in enumerate(counts):
        assert int(torch.unique(score[b, :c]).numel()) == c, f"sample {b}: two surviving anchors share a score"
    preds, _ = eng(dict(bd))
    out = eng.detect(dict(bd))
    got = net.padded_to_pred_dicts(out)
    check(out, preds, net.batched_rows())
    assert len(got) == len(preds) == 2 and sum(out["num"].tolist()) > 0
    for a, w in zip(got, preds):
        assert set(a) == set(w)
        for k in w:
            assert a[k].dtype == w[k].dtype and a[k].shape == w[k].shape and torch.equal(a[k], w[k]), k


def test_engine_detect_before_refresh_raises():
    from gdmae_hip import inference
    from test_inference_engine_kitti import _batch, _model
    net, ds = _model(seed=4)
    eng = inference.compile_detector(net)
    bd = _batch(ds)
    eng.detect(dict(bd))
    with torch.no_grad():
        net.dense_head.conv_box.weight.mul_(1.5)
    with pytest.raises(RuntimeError, match="refresh"):
        eng.detect(dict(bd))
    with pytest.raises(RuntimeError, match="refresh"):
        eng(dict(bd))
    eng.refresh()
    assert eng.detect(dict(bd))["num"].shape == (2,)
