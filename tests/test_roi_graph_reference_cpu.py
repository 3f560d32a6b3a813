"""CPU: the two numpy statements of the second stage (tests/roi_graph_reference.py) against the unmodified reference head
(tests/golden/roi_head_b2.npz) and against each other.

Statement (a), fp64, deviates from the fixture's fp32 outputs by (measured, the fixture's own fp32 round-off):
rcnn_cls 1.56e-6, rcnn_reg 1.74e-6, batch_box_preds 5.68e-6 (under one fp32 ulp of a 64 m coordinate), batch_cls_preds 1.08e-7
(the fp32 torch head, single-threaded, is 1.8e-6 / 1.7e-6 / 7.7e-6 / 1.2e-7 away from it); the test asserts 4 x these.  Statement (b) without rounding is the same function in another association: 1e-10."""
import os

import numpy as np
import pytest

import roi_graph_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED_A_VS_GOLDEN = {"rcnn_cls": 1.56e-6, "rcnn_reg": 1.74e-6, "batch_box_preds": 5.68e-6, "batch_cls_preds": 1.08e-7}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "roi_head_b2.npz"))


@pytest.fixture(scope="module")
def state(golden):
    return R.seeded_state(int(golden["seed"]))


def _run(fn, sd, z, **kw):
    return fn(sd, z["feats_local"], z["pooled_num"], z["rois"], z["roi_scores"], normalized=True, **kw)


def test_state_and_folded_buffer_shapes(golden, state):
    keys = {str(k)[len("roi_head."):] for k in golden["state_keys"] if not str(k).endswith("num_batches_tracked")}
    assert set(state) == keys
    flat = R.folded_flat(state)
    from gdmae_hip import lib as L
    assert flat.dtype == np.float32 and flat.shape == (sum(v.size for v in R.fold(state).values()),)
    assert flat.size == L.load().gdmae_roi_graph_folded_floats()             # the buffer the pack call reads (host-only query)


def test_statement_a_reproduces_the_reference_head(golden, state):
    out = _run(R.statement_a, state, golden)
    dev = R.deviation(out, golden)
    print("statement (a) vs the fixture:", dev)
    for k, m in MEASURED_A_VS_GOLDEN.items():
        assert dev[k] <= 4 * m, (k, dev[k])
    assert out["batch_box_preds"].shape == (2, 6, 7) and out["batch_cls_preds"].shape == (2, 6, 1)


@pytest.mark.parametrize("negative", [False, True])
def test_statement_b_equals_statement_a(golden, state, negative):
    sd = R.seeded_state(int(golden["seed"]), negative_scales=True) if negative else state
    if negative:
        for l in range(3):
            w = sd[f"{R.G}edge_layes.{l}.1.weight"]
            assert (w < 0).sum() >= 4 and (w > 0).sum() >= 4
    a, b = _run(R.statement_a, sd, golden), _run(R.statement_b, sd, golden)
    dev = R.deviation(b, a)
    print("statement (b) vs (a), negative scales", negative, dev)
    assert R.same_neighbour_sets(a["nbr"], b["nbr"])
    assert max(dev.values()) <= 1e-10


def test_negative_scales_catch_a_fold_after_the_max(golden):
    """the crafted state does what it is for: with the BatchNorm scale applied AFTER the neighbour max the outputs move"""
    sd = R.seeded_state(int(golden["seed"]), negative_scales=True)
    x = golden["feats_local"].astype(np.float64) * (golden["pooled_num"] > 0)[:, None, None]
    idx = R.neighbours(x[..., :3], fp32=True)
    W = sd[R.G + "edge_layes.0.0.weight"].reshape(32, 22)
    s = sd[R.G + "edge_layes.0.1.weight"] / np.sqrt(sd[R.G + "edge_layes.0.1.running_var"] + R.EPS)
    f = R.fold(sd)
    t = np.arange(x.shape[0])[:, None, None]
    right = (x @ f["e1_P"].T)[t, idx].max(axis=2)
    wrong = s * (x @ W[:, :11].T)[t, idx].max(axis=2)
    assert np.abs(right - wrong).max() > 1e-2


def test_bf16_rounding_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0e-3, 0.0], dtype=np.float64)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, 0.0, 0.0])
    got = R.round_bf16(x)
    assert np.array_equal(got[:4], want[:4]) and abs(got[4] + 3.0e-3) < 3.0e-3 * 2.0 ** -8 and got[5] == 0.0
    import torch
    v = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    assert np.array_equal(R.round_bf16(v).astype(np.float32), torch.from_numpy(v).to(torch.bfloat16).float().numpy())


def test_lattice_cases_are_what_they_say():
    feats, num, rois, scores = R.lattice_case(3, 1, 8, [0, 1, 7, 8, 9, 255, 256, 200], grid_rois=(7,))
    assert feats.shape == (8, 256, 11) and not feats[0].any()
    assert (feats[1] == feats[1][0]).all()                                         # one point: all slots equal
    assert np.array_equal(feats[3][8:16], feats[3][:8])                            # repeat padding
    assert np.array_equal(feats[..., :3] * 64, np.round(feats[..., :3] * 64))      # on the lattice
    x = feats[7][:, :3].astype(np.float64)
    d = np.sort(((x[:, None] - x[None]) ** 2).sum(-1), axis=1)
    assert (d[:, 7] == d[:, 8]).sum() >= 50                                        # distinct points tie at the 8th place
    nbr = R.neighbours(feats[..., :3], fp32=True)
    assert (nbr[1] == np.arange(8)).all() and (nbr[0] == np.arange(8)).all()
    own = feats[3][:, :3]
    assert (own[nbr[3]] == own[:, None]).all()                                     # 8 points: every neighbour a copy of the slot


def test_engine_fold_equals_the_reference_fold(golden):
    """``inference.fold_roi_head`` (torch, from the modules) writes the buffer ``folded_flat`` (numpy, from the state) writes"""
    import torch
    from gdmae_hip import configs, inference
    from pcdet.models.roi_heads.graphrcnn_head import GraphRCNNHead
    _, ds = configs.waymo_two_stage_cfg()
    head = GraphRCNNHead(input_channels=5, model_cfg=configs.graphrcnn_head_cfg(), point_cloud_range=ds.point_cloud_range, num_class=1).eval()
    sd = R.seeded_state(int(golden["seed"]), negative_scales=True)
    head.load_state_dict({k: torch.from_numpy(v.reshape(tuple(head.state_dict()[k].shape))).float() for k, v in sd.items()}, strict=False)
    with torch.no_grad():
        flat = inference.fold_roi_head(head).numpy()
    want = R.folded_flat({k: v.astype(np.float32) for k, v in sd.items()})
    assert flat.shape == want.shape and np.abs(flat - want).max() <= 1e-6 * np.abs(want).max()
    bad = GraphRCNNHead(input_channels=5, model_cfg=configs.graphrcnn_head_cfg(), point_cloud_range=ds.point_cloud_range, num_class=3).eval()
    with pytest.raises(NotImplementedError, match="num_class"):
        inference.fold_roi_head(bad)
    head.attn_gnn_layer.reduction = None
    with pytest.raises(NotImplementedError, match="USE_REDUCTION"):
        inference.fold_roi_head(head)
