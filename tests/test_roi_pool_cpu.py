"""CPU: the numpy statement of the RoI pooling contract in ``pcdet.ops.patch_ops`` equals the reference of
tests/roi_pool_reference.py on every scene of the GPU test (indices and counts exactly, features to 1e-6), and the reference
itself has the properties the contract promises."""
import numpy as np
import pytest

import roi_pool_reference as R


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_cpu_path_equals_the_reference(name):
    pts, rois, pcr, P, ref = R.scene(name)
    idx, num, feats, glob = R.run_module(name, 'cpu')
    assert np.array_equal(num, ref['num'])
    assert np.array_equal(idx, ref['idx'])
    assert np.abs(feats - ref['feats']).max(initial=0) <= 1e-6
    assert np.array_equal(glob, ref['glob'])


def test_scenes_cover_what_they_are_for():
    _, _, _, P, ref = R.scene('shipped')
    num = ref['num']
    assert num[0, 0] == P['num_dvs_points'] and num[0, 5] == 0 and 0 < num[1, 3] < P['num_fps_points']
    assert (num[(num > 0)] >= 1).all() and (num >= P['num_fps_points']).sum() >= 8
    assert ref['num'].shape == (2, 12) and 5000 < R.scene('shipped')[0].shape[0] < 8000
    _, _, _, _, cap = R.scene('box_cap')
    assert (cap['num'][0, :32] > 0).all() and (cap['num'][0, 32:] == 0).all() and (cap['idx'][0, 32:] == 0).all()
    assert (cap['idx'][0, :32] == cap['idx'][0, 0]).all()
    pts, rois, pcr, P, big = R.scene('lds_overflow')
    inside = np.isfinite(R.pair_margins(pts, rois[:, :1], P)[1]).sum()
    assert inside > R.LDS_TABLE_FILL and big['num'][0, 0] == P['num_dvs_points']      # every lattice point is its own voxel
    _, _, _, _, e = R.scene('empty_sample')
    assert (e['num'][1] == 0).all() and (e['num'][0] > 0).all() and not e['feats'][3:].any()
    _, _, _, _, z = R.scene('padded_rois')
    assert (z['num'][1] > 0).all() and (z['idx'][1] == z['idx'][1, 0]).all()
    _, _, _, Pt, t = R.scene('tiny')
    assert t['num'].max() == Pt['num_dvs_points'] and t['num'].min() < Pt['num_fps_points']


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_reference_properties(name):
    pts, rois, pcr, P, ref = R.scene(name)
    B, M = rois.shape[:2]
    K = P['num_fps_points']
    for b in range(B):
        for r in range(M):
            cand, vox, n = ref['cand'][b * M + r], ref['voxels'][b * M + r], int(ref['num'][b, r])
            assert n == len(cand) <= P['num_dvs_points']
            if n == 0:
                assert not ref['idx'][b, r].any() and not ref['feats'][b * M + r].any() and not ref['glob'][b * M + r].any()
                continue
            # every selected row lies inside its enlarged RoI, in its sample, inside the xy range
            c, d, h = R._box64(rois[b, r], P['pool_extra_width'])
            loc = R._local(pts[cand, 1:4], c, h)
            assert (np.abs(loc) < d / 2 + 1e-5).all() and (pts[cand, 0] == b).all()
            assert (pts[cand, 1:3] >= pcr[:2]).all() and (pts[cand, 1:3] <= pcr[3:5]).all()
            # at most one row per voxel, rows ascending
            assert len(set(vox)) == len(vox) and (np.diff(cand) > 0).all()
            # FPS: prefix property (the first k slots are the k-round result), no repeats before the padding, padding repeats
            idx = ref['idx'][b, r]
            m = min(K, n)
            assert len(set(idx[:m].tolist())) == m and set(idx[:m].tolist()) <= set(cand.tolist()) and idx[0] == cand[0]
            assert np.array_equal(idx[m:], idx[np.arange(m, K) % n]) if n < K else True
            k = max(1, m // 2)
            sel, _ = R.fps_fp32(pts[cand, 1:4], k)
            assert np.array_equal(cand[sel], idx[:k])
            # each pick is a farthest point of what was picked before it
            xyz = pts[cand, 1:4].astype(np.float64)
            for s in (1, m - 1):
                if 0 < s < m:
                    dist = ((xyz[:, None] - pts[idx[:s], 1:4].astype(np.float64)[None]) ** 2).sum(-1).min(1)
                    assert dist[np.nonzero(cand == idx[s])[0][0]] == dist.max()
