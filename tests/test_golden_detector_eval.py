"""CPU: the evaluation-mode detector golden (tests/golden/make_golden_detector_eval.py) is self-consistent, so that the fixture the
inference-engine parity test rests on cannot rot unnoticed."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEAD_MAPS = {"hm": 3, "center": 2, "center_z": 1, "dim": 3, "rot": 2}


def test_eval_golden_is_self_consistent():
    path = os.path.join(GOLDEN, "detector_eval_kitti_b2.npz")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(GOLDEN, "waymo_b1.npz"))
    z = dict(np.load(path))
    B = int(z["batch_size"])
    pts = z["points"]
    assert pts.ndim == 2 and pts.shape[1] == 1 + int(z["num_point_features"]) and np.isfinite(pts).all()
    assert set(np.unique(pts[:, 0]).astype(int)) == set(range(B))
    vc = z["voxel_coords"]
    assert vc.ndim == 2 and vc.shape[1] == 4 and vc.min() >= 0 and len(np.unique(vc, axis=0)) == len(vc)
    means = {k: v for k, v in z.items() if k.startswith("bn/") and k.endswith("running_mean")}
    vars_ = {k: v for k, v in z.items() if k.startswith("bn/") and k.endswith("running_var")}
    # DynVFE 2 + sparse convolutions 5 + deblocks 3 + conv_out 1 + BEV 4 + shared_conv 1 + head branches 5
    assert len(means) == len(vars_) == 21
    for k, v in vars_.items():
        m = means[k.replace("running_var", "running_mean")]
        assert v.shape == m.shape and np.isfinite(v).all() and np.isfinite(m).all(), k
        assert (v > 0).all() and not np.allclose(v, 1.0), k           # real batch statistics, not the (0, 1) initialisation
        assert not np.allclose(m, 0.0), k
    for name in ("pillar_features", "spatial_features", "spatial_features_2d", *HEAD_MAPS):
        s, c = z[name + "_s"], z[name + "_c"]
        assert s.shape == (4096,) and c.shape == (3,) and np.isfinite(s).all() and np.isfinite(c).all(), name
        assert c[1] > 0 and c[2] > 0 and abs(c[0]) <= c[1] * (1 + 1e-9), name
    assert (z["pillar_features_s"] >= 0).all() and (z["spatial_features_s"] >= 0).all()      # ReLU / maximum outputs
    top = z["top_cells"]
    assert top.shape == (B, 3, 64) and top.min() >= 0
    for name, c in HEAD_MAPS.items():
        assert z[name + "_top"].shape == (B, c, 3 * 64) and np.isfinite(z[name + "_top"]).all(), name
    hm_top = z["hm_top"].reshape(B, 3, 3, 64)
    for k in range(3):                                                   # class k's own cells are sorted by its heat map
        assert (np.diff(hm_top[:, k, k, :], axis=1) <= 0).all()
    # the decoder-background case the engine must get right: empty sites whose relu(b_i) is not zero
    share = z["deblock_positive_bias_share"]
    assert share.shape == (3,) and (share > 0.05).all()
