"""GPU: ``gdmae_roi_dfvs_pool`` (csrc/roi_pool.hip) against the numpy reference of tests/roi_pool_reference.py.  Indices and
counts are compared exactly; features to an absolute 1e-5 (the device's sin / cos: |local coordinate| < 8 m here, one fp32 ulp
there is 4.8e-7 and the rotation is two products and a sum).  The scenes keep every decision 1e-4 m / 1e-3 cells away from
what the contract leaves implementation-defined, so the fp32 device geometry has one answer."""
import numpy as np
import pytest
import torch

import roi_pool_reference as R

pytestmark = pytest.mark.gpu


def check(name):
    pts, rois, pcr, P, ref = R.scene(name)
    idx, num, feats, glob = R.run_module(name, 'cuda')
    print(f"{name}: N={pts.shape[0]} rois={rois.shape[:2]} num={num.reshape(-1)[:12].tolist()} "
          f"feature deviation={np.abs(feats - ref['feats']).max(initial=0):.2e}")
    assert np.array_equal(num, ref['num'])
    assert np.array_equal(idx, ref['idx'])
    assert np.abs(feats - ref['feats']).max(initial=0) <= 1e-5
    assert np.array_equal(glob, ref['glob'])
    return idx, num, feats, glob


def test_shipped_parameters():
    """B = 2, M = 12, headings over the full circle, RoIs partly outside the xy range, an empty RoI, repeat padding, the
    1024-candidate cap."""
    _, num, _, _ = check('shipped')
    assert num[0, 0] == 1024 and num[0, 5] == 0 and 0 < num[1, 3] < 256


def test_tiny_parameters():
    check('tiny')


def test_box_cap_keeps_the_lowest_roi_indices():
    _, num, _, _ = check('box_cap')
    assert (num[0, :32] > 0).all() and (num[0, 32:] == 0).all()


@pytest.mark.parametrize("name", ["one_by_one", "empty_sample", "padded_rois"])
def test_other_shapes(name):
    check(name)


def test_roi_beyond_the_lds_table():
    """more distinct voxels than one pass of the LDS table accepts: the row-limit bisection, exact"""
    check('lds_overflow')


def test_no_points_and_no_rois():
    from pcdet.ops.patch_ops import patch_ops_utils as po
    lo, shape = po.patch_grid(R.WAYMO_RANGE)
    args = ([-74.88, -74.88, 74.88, 74.88], lo, shape, 1024, 256, 4099, 0.18, 50.0, [0.8] * 3, 32)
    rois = torch.from_numpy(R.scene('one_by_one')[1].copy()).cuda()
    idx, num, feats, glob = po.roi_dfvs_pool(torch.zeros(0, 6, device='cuda'), rois, *args)
    assert int(num.sum()) == 0 and not idx.any() and not feats.any() and not glob.any()
    idx, num, feats, glob = po.roi_dfvs_pool(torch.zeros(5, 6, device='cuda'), rois[:, :0], *args)
    assert idx.shape == (1, 0, 256) and feats.shape == (0, 256, 11)


def test_repeatability():
    a = R.run_module('shipped', 'cuda')
    b = R.run_module('shipped', 'cuda')
    c = R.run_module('lds_overflow', 'cuda')
    d = R.run_module('lds_overflow', 'cuda')
    for x, y in zip(a + c, b + d):
        assert x.tobytes() == y.tobytes()
