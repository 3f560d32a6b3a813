"""GPU: ``gdmae_roi_graph_forward`` (csrc/roi_graph.hip) through the C ABI on crafted pooled tensors, no detector.

Two bounds, both measured on an MI355X (every test prints its figures before it asserts):

* against the unmodified reference head (tests/golden/roi_head_b2.npz, fp32): the bf16-vs-fp32 deviation of the five bf16 products,
  MEASURED_VS_GOLDEN; asserted at 2 x (the project's margin for bf16-vs-fp32 bounds);
* against statement (b) of tests/roi_graph_reference.py with the kernel's roundings switched on: what is left is fp32 accumulation
  order, the device's expf / sinf / cosf, and the rare activation that the two round to different bf16 neighbours because it sits
  within fp32 round-off of a rounding boundary; MEASURED_VS_B, asserted at 4 x.

Most RoIs sit 1e-6 to 8e-6 from statement (b) (three to four orders below the first bound): the seeded state on the fixture's inputs
gives 1.5e-6 / 2.8e-6 / 6.3e-6 / 6.6e-8, the lattice scenes t1, b3_m1, pooled_num_edges and regular_grid_ties at most 8.6e-6 on the
boxes.  A few RoIs sit at 1e-4 to 6e-4: two of the fixture's twelve with the negative-scale state (the figures below) and one of
t5_one_sample (6.3e-4 on the boxes).  That is the bf16 flip of one high-leverage activation, not the kernels: statement (b) evaluated
with numpy fp32 arithmetic in place of fp64 deviates from statement (b) by 2.26e-4 / 2.44e-4 / 5.55e-4 / 3.33e-5 on the same inputs, in
the same two RoIs, and by up to 8e-5 on one RoI in six of other lattice scenes.  MEASURED_VS_B therefore records the flip, and stays
6 to 40 times below the bf16-vs-fp32 bound.
"""
import os

import numpy as np
import pytest

import roi_graph_reference as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# largest |library - fixture| over the 12 RoIs of the fixture (logits, residuals, metres / radians, probabilities)
MEASURED_VS_GOLDEN = {"rcnn_cls": 3.03e-3, "rcnn_reg": 5.93e-3, "batch_box_preds": 2.22e-2, "batch_cls_preds": 1.49e-4}
# largest |library - statement (b), rounded| over the fixture's inputs with the seeded and with the negative-scale state
MEASURED_VS_B = {"rcnn_cls": 2.28e-4, "rcnn_reg": 2.45e-4, "batch_box_preds": 5.50e-4, "batch_cls_preds": 3.34e-5}


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "roi_head_b2.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def states(golden):
    seed = int(golden["seed"])
    return {"seeded": R.seeded_state(seed), "negative": R.seeded_state(seed, negative_scales=True)}


def _args(z):
    return z["feats_local"], z["pooled_num"], z["rois"], z["roi_scores"]


def _within(dev, measured, factor):
    return all(dev[k] <= factor * measured[k] for k in R.OUTPUTS)


def test_golden_fixture_through_the_kernels(golden, states):
    """T = 12: one empty RoI, one with 40 points and repeat-padded slots"""
    out = R.run_library(states["seeded"], *_args(golden), key="seeded")
    dev = R.deviation(out, golden)
    print("library vs the reference head's fixture (bf16 vs fp32):", dev)
    assert all(np.isfinite(out[k]).all() for k in R.OUTPUTS)
    assert _within(dev, MEASURED_VS_GOLDEN, 2), dev


@pytest.mark.parametrize("which", ["seeded", "negative"])
def test_against_the_rounded_decomposition(golden, states, which):
    sd = states[which]
    out = R.run_library(sd, *_args(golden), key=which)
    ref = R.statement_b(sd, *_args(golden), bf16=True)
    dev = R.deviation(out, ref)
    print(f"library vs statement (b) with rounding, {which} state:", dev)
    assert R.same_neighbour_sets(out["nbr"], ref["nbr"])
    assert _within(dev, MEASURED_VS_B, 4), dev


CASES = {
    "t1": (11, 1, 1, [256], ()),
    "t5_one_sample": (12, 1, 5, [256, 9, 255, 7, 100], ()),
    "b3_m1": (13, 3, 1, [256, 8, 1], ()),
    "pooled_num_edges": (14, 1, 7, [0, 1, 7, 8, 9, 255, 256], ()),
    "regular_grid_ties": (15, 1, 2, [200, 256], (0, 1)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_crafted_lattice_scenes(states, name):
    """points on a 1/64 m lattice: distances exact, ties genuine; the neighbour SETS must be the reference's"""
    seed, B, M, nums, grid = CASES[name]
    case = R.lattice_case(seed, B, M, nums, grid_rois=grid)
    sd = states["negative"]
    out = R.run_library(sd, *case, key="negative")
    ref = R.statement_b(sd, *case, bf16=True)
    dev = R.deviation(out, ref)
    print(f"{name}: library vs statement (b) with rounding:", dev)
    assert out["nbr"].min() >= 0 and out["nbr"].max() < 256
    assert R.same_neighbour_sets(out["nbr"], ref["nbr"])
    if name == "b3_m1":
        own = case[0][1][:, :3]
        assert (own[out["nbr"][1]] == own[:, None]).all()          # 8 points: every neighbour is a copy of the slot's own point
    assert _within(dev, MEASURED_VS_B, 4), dev


def test_roi_scores_as_logits(states):
    case = R.lattice_case(21, 2, 2, [256, 30, 0, 256])
    logits = np.log(case[3] / (1 - case[3])).astype(np.float32)
    sd = states["seeded"]
    out = R.run_library(sd, case[0], case[1], case[2], logits, normalized=False, key="seeded")
    ref = R.statement_b(sd, case[0], case[1], case[2], logits, normalized=False, bf16=True)
    dev = R.deviation(out, ref)
    print("roi_scores as logits:", dev)
    assert _within(dev, MEASURED_VS_B, 4), dev


def test_rows_do_not_depend_on_the_launch_geometry(golden, states):
    """the same 12 RoIs alone, permuted, and inside a batch of 16: bit-identical rows"""
    sd = states["seeded"]
    feats, num, rois, scores = _args(golden)
    r12, s12 = rois.reshape(12, -1), scores.reshape(12)
    base = R.run_library(sd, feats, num, rois, scores, key="seeded")

    def rows(o):
        return [o["rcnn_cls"].reshape(-1, 1), o["rcnn_reg"].reshape(-1, 7), o["batch_box_preds"].reshape(-1, 7),
                o["batch_cls_preds"].reshape(-1, 1), o["nbr"].reshape(-1, 256 * 8)]
    want = rows(base)
    for t in range(12):
        one = rows(R.run_library(sd, feats[t:t + 1], num[t:t + 1], r12[t:t + 1][None], s12[t:t + 1][None], key="seeded"))
        for a, b in zip(one, want):
            assert a[0].tobytes() == b[t].tobytes(), t
    perm = np.random.default_rng(4).permutation(12)
    got = rows(R.run_library(sd, feats[perm], num[perm], r12[perm].reshape(3, 4, -1), s12[perm].reshape(3, 4), key="seeded"))
    for a, b in zip(got, want):
        assert a.tobytes() == b[perm].tobytes()
    extra = R.lattice_case(5, 1, 4, [256, 0, 77, 256])
    where = np.array([0, 1, 3, 4, 5, 7, 8, 9, 10, 12, 14, 15])            # the 12 among 16, the others are lattice RoIs
    f16, n16 = np.zeros((16, 256, 11), np.float32), np.zeros(16, np.int32)
    r16, s16 = np.zeros((16, 7), np.float32), np.zeros(16, np.float32)
    rest = np.setdiff1d(np.arange(16), where)
    f16[where], n16[where], r16[where], s16[where] = feats, num, r12[:, :7], s12
    f16[rest], n16[rest], r16[rest], s16[rest] = extra[0], extra[1], extra[2].reshape(4, 7), extra[3].reshape(4)
    got = rows(R.run_library(sd, f16, n16, r16.reshape(2, 8, 7), s16.reshape(2, 8), key="seeded"))
    for a, b in zip(got, want):
        assert a[where].tobytes() == b.tobytes()
