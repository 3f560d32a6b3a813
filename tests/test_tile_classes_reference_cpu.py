"""CPU: the numpy reference of the tile classes / pairing order (tests/tile_classes_reference.py) on crafted grids, so that the GPU test
of both builders (tests/test_tile_conv_skip_gpu.py) compares against something that was itself checked."""
import numpy as np
import pytest

import tile_classes_reference as R


def _check_order(r):
    n = r["n_act"]
    o, c = r["tile_order"], r["tile_class"]
    assert sorted(o.tolist()) == list(range(n))                       # a permutation of the slots
    assert np.all(np.diff(c[o]) >= 0)                                  # classes ascend along it
    for g in np.unique(c):
        assert np.all(np.diff(o[c[o] == g]) > 0)                       # slots ascend within a class
    assert np.array_equal(r["tile_slot"][r["tile_list"]], np.arange(n))
    assert np.all(np.diff(r["tile_list"]) > 0)


def _class_of_tile(r, B, H, W, b, ty, tx):
    TH, TW = (H + 7) // 8, (W + 7) // 8
    s = r["tile_slot"][(b * TH + ty) * TW + tx]
    return None if s < 0 else int(r["tile_class"][s])


@pytest.mark.parametrize("level", [2, 1, 0])
def test_center_tile_takes_each_class(level):
    maps, strides, B, H, W = R.scene_center(level)
    r = R.tile_classes(maps, strides, B, H, W)
    _check_order(r)
    assert _class_of_tile(r, B, H, W, 0, 1, 1) == level               # level 0: the token sits in the halo ring, outside the tile
    for ty in range(3):
        for tx in range(3):
            if (ty, tx) != (1, 1):
                assert _class_of_tile(r, B, H, W, 0, ty, tx) in (None, 0)   # a tile on the map's edge is class 0 whatever it holds


def test_halo_ring_token_makes_class_0_not_1():
    maps, strides, B, H, W = R.scene_center(1)
    assert _class_of_tile(R.tile_classes(maps, strides, B, H, W), B, H, W, 0, 1, 1) == 1
    for y, x in ((7, 12), (16, 12), (12, 7), (12, 16), (16, 16)):       # each side of the ring and a corner
        m = [a.copy() for a in maps]
        R.put(m[0], 0, y, x)
        assert _class_of_tile(R.tile_classes(m, strides, B, H, W), B, H, W, 0, 1, 1) == 0, (y, x)


def test_edge_tiles_are_class_0_whatever_they_hold():
    B, H, W = 1, 40, 40
    for ty, tx in ((0, 2), (4, 2), (2, 0), (2, 4)):
        maps = R.empty_maps(B, H, W, R.STRIDES)
        R.put(maps[2], 0, ty * 2, tx * 2)                              # only a stage-2 token, inside the tile
        r = R.tile_classes(maps, R.STRIDES, B, H, W)
        _check_order(r)
        assert _class_of_tile(r, B, H, W, 0, ty, tx) == 0
        assert 2 in r["tile_class"] or (ty, tx) in ((0, 2), (2, 0))   # its interior neighbour, through the halo, is class 2


def test_map_height_not_a_multiple_of_the_tile():
    B, H, W = 1, 36, 40                                                # TH = 5, the last tile row holds 4 map rows
    maps = R.empty_maps(B, H, W, R.STRIDES)
    R.put(maps[2], 0, 7, 4)                                            # sites (28 .. 31, 16 .. 19): tile (3, 2), halo rows 23 .. 32
    R.put(maps[2], 0, 8, 6)                                            # sites (32 .. 35, 24 .. 27): tile (4, 3), sites past the map
    r = R.tile_classes(maps, R.STRIDES, B, H, W)
    _check_order(r)
    assert _class_of_tile(r, B, H, W, 0, 3, 2) == 2
    assert _class_of_tile(r, B, H, W, 0, 4, 3) == 0
    assert _class_of_tile(r, B, H, W, 0, 4, 2) == 0                    # active through its halo row 31, and on the edge


def test_classes_are_capped_at_k_minus_1():
    B, H, W = 1, 24, 24
    m1 = R.empty_maps(B, H, W, (4,))
    R.put(m1[0], 0, 3, 3)
    r = R.tile_classes(m1, (4,), B, H, W)
    _check_order(r)
    assert r["n_act"] == 4 and np.all(r["tile_class"] == 0)            # k = 1: nothing to skip
    maps, strides, B, H, W = R.scene_k2()
    r = R.tile_classes(maps, strides, B, H, W)
    _check_order(r)
    assert set(r["tile_class"].tolist()) == {0, 1}
    assert _class_of_tile(r, B, H, W, 0, 2, 2) == 1 and _class_of_tile(r, B, H, W, 0, 1, 3) == 0


def leads(r):
    """per workgroup of the tile convolution the number of skipped phases: min class of its two slots"""
    c = r["tile_class"][r["tile_order"]]
    return [int(min(c[i:i + 2])) for i in range(0, len(c), 2)], [len(set(c[i:i + 2].tolist())) > 1 for i in range(0, len(c), 2)]


def test_crafted_scenes_hold_what_the_gpu_test_says_they_hold():
    maps, strides, B, H, W = R.scene_mixed()
    r = R.tile_classes(maps, strides, B, H, W)
    _check_order(r)
    ld, mixed = leads(r)
    print("mixed scene: n_act", r["n_act"], "classes", np.bincount(r["tile_class"], minlength=3).tolist(), "leads", ld, "mixed", mixed)
    assert r["n_act"] % 2 == 1 and set(r["tile_class"].tolist()) == {0, 1, 2}
    assert {0, 1, 2} <= set(ld) and any(mixed)
    assert not np.array_equal(r["tile_order"], np.arange(r["n_act"]))
    maps, strides, B, H, W = R.scene_all_class0()
    r = R.tile_classes(maps, strides, B, H, W)
    _check_order(r)
    assert r["n_act"] > 2 and np.all(r["tile_class"] == 0) and np.array_equal(r["tile_order"], np.arange(r["n_act"]))
    maps, strides, B, H, W = R.scene_k2()
    r = R.tile_classes(maps, strides, B, H, W)
    assert 1 in leads(r)[0]
