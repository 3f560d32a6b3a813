"""Fine-tune input pipeline, GPU half: the library against the reference golden and against the numpy statement
(tests/finetune_input_reference.py) on the crafted scenes of tests/finetune_input_scenes.py."""
import numpy as np
import pytest
import torch

import finetune_input_scenes as sc
from gdmae_hip import input_pipeline as ip

pytestmark = pytest.mark.gpu

COORD_TOL = 2e-5          # the project's bound for this arithmetic (tests/test_input_pipeline.py)


def _database(scene):
    d = scene["db"]
    return ip.GtDatabase(d["points"], d["offsets"], d["boxes"], d["names"])


def _pipe(scene, **kw):
    return ip.GpuFinetuneInputPipeline(sc.PC_RANGE, sc.CLASS_NAMES, sc.AUG_CFG, _database(scene), **kw)


def _run(pipe, scene, **kw):
    out = pipe(scene["frames"], scene["gt_boxes"], scene["gt_names"], params=scene["params"], candidates=scene["candidates"], **kw)
    return {"points": out["points"].cpu().numpy(), "gt_boxes": out["gt_boxes"].cpu().numpy(), "num_gt": out["num_gt"],
            "valid": out["sampled_valid"], "batch_size": out["batch_size"]}


def _compare_boxes(got, exp, num_gt, head_tol):
    """Shape, counts, order and class column exact; centres and sizes within COORD_TOL; headings within head_tol."""
    assert got.shape == exp.shape
    assert np.array_equal(got[:, :, 7], exp[:, :, 7])
    for b, n in enumerate(num_gt):
        assert not got[b, n:].any()                                              # zero rows behind the kept boxes
    print("boxes: max |centre, size| deviation", np.abs(got[:, :, :6] - exp[:, :, :6]).max(initial=0), "heading", np.abs(got[:, :, 6] - exp[:, :, 6]).max(initial=0))
    assert np.abs(got[:, :, :6] - exp[:, :, :6]).max(initial=0) <= COORD_TOL
    assert np.abs(got[:, :, 6] - exp[:, :, 6]).max(initial=0) <= head_tol


def _compare(got, st, head_tol=0.0):
    assert [v.tolist() for v in got["valid"]] == [v.tolist() for v in st["valid"]]
    assert got["num_gt"] == st["num_gt"]
    gp, ep = got["points"], st["points"]
    assert gp.shape == ep.shape                                                  # row counts
    assert np.array_equal(gp[:, 0], ep[:, 0]) and np.array_equal(gp[:, 4:], ep[:, 4:])       # frames, row order (features identify a row)
    print("points: max coordinate deviation", np.abs(gp - ep).max(initial=0))
    assert np.abs(gp - ep).max(initial=0) <= COORD_TOL
    _compare_boxes(got["gt_boxes"], st["gt_boxes"], st["num_gt"], head_tol)


def _assert_margins(st):
    m = st["margins"]
    assert m["pair"] >= 1e-2 and m["inbox"] >= 1e-3 and m["range"] >= 1e-3 and m["corner"] >= 1e-3, m


def test_golden_points_and_boxes():
    """The reference's own augmentation / limit_period / range masks / collate on 4 frames with 6 - 8 boxes each (no database).
    Headings: the generator measured a deviation of 0.0 between the numpy statement and the reference (every operation on the
    heading is a single correctly rounded fp32 operation), so 4 x that deviation asks for bit-equal headings."""
    z, frames, boxes, names, params, perms = sc.load_golden()
    pipe = ip.GpuFinetuneInputPipeline(z["pc_range"], z["class_names"].tolist(), ip.FINETUNE_AUG_CONFIG, None)
    out = pipe(frames, boxes, names, params=params, perms=perms)
    got, exp = out["points"].cpu().numpy(), z["expected_points"]
    assert got.shape == exp.shape and out["batch_size"] == 4
    assert np.array_equal(got[:, 0], exp[:, 0]) and np.array_equal(got[:, 4:], exp[:, 4:])
    assert np.abs(got - exp).max() <= COORD_TOL
    assert out["num_gt"] == z["num_gt"].tolist()
    _compare_boxes(out["gt_boxes"].cpu().numpy(), z["expected_gt_boxes"], out["num_gt"], 4 * float(z["err_heading"]))


def test_crafted_sampling_scene_matches_the_statement():
    s = sc.crafted()
    st = sc.statement(s)
    _assert_margins(st)
    assert not st["valid"][0][:2].any() and st["valid"][1].tolist() == [False, False, False, True, True, True, True, True, False, True]
    _compare(_run(_pipe(s, shuffle=False), s), st)


@pytest.mark.parametrize("size", ["small", "tile", "multi"])
def test_scan_seams(size):
    """'small': one workgroup's loop (rows <= GD_SCAN_SINGLE_MAX); 'tile': just above one GD_SCAN_TILE, an object segment astride the
    seam, the frame boundary in the tile before it, a one-point candidate, an empty frame; 'multi': above GD_SCAN_SINGLE_MAX, where
    the scan really runs tile by tile (an object segment astride row 8192, a frame boundary and an object astride row 65536)."""
    s = sc.seams(size)
    rows = sum(len(f) for f in s["frames"]) + len(s["db"]["points"])
    assert {"small": rows < 4096, "tile": 4096 < rows < 4096 + 512, "multi": rows > 65536}[size]
    st = sc.statement(s)
    _assert_margins(st)
    _compare(_run(_pipe(s, shuffle=False), s), st)


def test_resident_and_staged_database_agree():
    s = sc.crafted()
    a, b = _run(_pipe(s, shuffle=False, resident=True), s), _run(_pipe(s, shuffle=False, resident=False), s)
    assert a["points"].tobytes() == b["points"].tobytes() and a["gt_boxes"].tobytes() == b["gt_boxes"].tobytes()
    assert a["points"].shape[0] > 0 and a["gt_boxes"].shape[1] > 0


def test_default_mode_draws_and_shuffles():
    """Drawn candidates, world parameters and order: reproducible from the two seeds; the shuffled rows of every frame are a
    permutation of the unshuffled ones; frames stay contiguous and in order."""
    s = sc.crafted()

    def run(shuffle):
        np.random.seed(4)
        torch.manual_seed(4)
        out = _pipe(s, shuffle=shuffle)(s["frames"], s["gt_boxes"], s["gt_names"])
        return out["points"].cpu().numpy(), out["gt_boxes"].cpu().numpy(), out["num_gt"]
    p1, g1, n1 = run(True)
    p2, g2, n2 = run(True)
    assert p1.tobytes() == p2.tobytes() and g1.tobytes() == g2.tobytes() and n1 == n2
    p0, g0, n0 = run(False)
    assert g0.tobytes() == g1.tobytes() and n0 == n1 and p0.shape == p1.shape and not np.array_equal(p0, p1)
    assert np.array_equal(p0[:, 0], p1[:, 0]) and (np.diff(p1[:, 0]) >= 0).all()
    key = lambda a: a[np.lexsort(a.T[::-1])]                                # noqa: E731
    assert np.array_equal(key(p0), key(p1))
    assert len(s["gt_boxes"][0]) == 0 and n1[0] > 0                         # frame 0 has no box of its own: the draw did paste objects


def test_limits():
    s = sc.limits(64, 448)
    st = sc.statement(s)
    assert st["margins"]["pair"] >= 1e-2
    got = _run(_pipe(s, shuffle=False), s)
    assert got["valid"][0].tolist() == st["valid"][0].tolist() and 0 < st["valid"][0].sum() < 64
    assert got["num_gt"] == st["num_gt"]
    for n_cand, n_gt, msg in ((65, 448, "more than 64 candidates"), (64, 449, "more than 448 existing boxes")):
        s = sc.limits(n_cand, n_gt)
        with pytest.raises(NotImplementedError, match=msg):
            _run(_pipe(s, shuffle=False), s)
    torch.cuda.synchronize()                                                # the refusals launched nothing: the device is fine
