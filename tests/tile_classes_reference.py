"""Plain numpy reference for the tile classes and the class-sorted pairing order of the decoder's tile convolution
(csrc/conv_tiles.hip: k_ct_tile_flags, k_ct_tile_order).

maps[g]: (B, H // s_g, W // s_g) integer cell -> token map of source stage g (-1: no token), s_g = strides[g].
A tile (8 x 8 sites) is ACTIVE if some in-map site of its 10 x 10 halo patch is covered by a token of some stage.
Its class is the number of LEADING stages without a token anywhere in the patch, capped at k - 1, and 0 if any site of the patch
lies outside the map.  Slots number the active tiles in ascending tile id; the order lists the slots by ascending class, stable."""
import numpy as np


def tile_classes(maps, strides, B, H, W):
    """-> dict(tile_slot (B*TH*TW,), tile_list (n_act,), tile_class (n_act,), tile_order (n_act,), n_act), all int64."""
    k = len(maps)
    TH, TW = (H + 7) // 8, (W + 7) // 8
    slot = -np.ones(B * TH * TW, dtype=np.int64)
    tlist, tcls = [], []
    for b in range(B):
        for ty in range(TH):
            for tx in range(TW):
                tok = [False] * k
                outside = False
                for py in range(10):
                    for px in range(10):
                        y, x = ty * 8 - 1 + py, tx * 8 - 1 + px
                        if y < 0 or y >= H or x < 0 or x >= W:
                            outside = True
                            continue
                        for g in range(k):
                            s = strides[g]
                            tok[g] = tok[g] or maps[g][b, y // s, x // s] >= 0
                if not any(tok):
                    continue
                cls = 0
                while cls < k - 1 and not tok[cls]:
                    cls += 1
                t = (b * TH + ty) * TW + tx
                slot[t] = len(tlist)
                tlist.append(t)
                tcls.append(0 if outside else cls)
    tcls = np.asarray(tcls, dtype=np.int64)
    order = np.argsort(tcls, kind="stable").astype(np.int64)
    return dict(tile_slot=slot, tile_list=np.asarray(tlist, dtype=np.int64), tile_class=tcls, tile_order=order, n_act=len(tlist))


def empty_maps(B, H, W, strides):
    return [-np.ones((B, H // s, W // s), dtype=np.int64) for s in strides]


def put(m, b, y, x):
    """a token at cell (b, y, x) of a stage's own grid; tokens are numbered in the order they are put"""
    assert m[b, y, x] < 0
    m[b, y, x] = int((m >= 0).sum())


# ---- the crafted maps of tests/test_tile_conv_skip_gpu.py and tests/test_tile_classes_reference_cpu.py (strides 1, 2, 4)
STRIDES = (1, 2, 4)


def scene_center(level):
    """B = 1, 24 x 24: 3 x 3 tiles, tile (1, 1) is the only one whose halo stays inside the map.  level 2: one stage-2 token under it
    (class 2); 1: a stage-1 token added (class 1); 0: a stage-0 token in the corner site of its halo ring, outside the tile (class 0)."""
    maps = empty_maps(1, 24, 24, STRIDES)
    put(maps[2], 0, 3, 3)                 # sites 12 .. 15
    if level <= 1:
        put(maps[1], 0, 5, 6)             # sites (10 .. 11, 12 .. 13)
    if level <= 0:
        put(maps[0], 0, 7, 7)             # the corner of tile (1, 1)'s halo ring: site (7, 7) belongs to tile (0, 0)
    return maps, STRIDES, 1, 24, 24


def scene_mixed():
    """B = 2, 40 x 40 (5 x 5 tiles a frame): all three classes among the interior tiles, an odd number of active tiles, and class
    changes at odd places of the order (a workgroup whose two tiles differ in class)."""
    B, H, W = 2, 40, 40
    maps = empty_maps(B, H, W, STRIDES)
    put(maps[2], 0, 4, 4)                 # sites 16 .. 19 of frame 0: tile (2, 2) and, through their halos, its upper / left neighbours
    put(maps[2], 0, 2, 6)                 # sites (8 .. 11, 24 .. 27): tile (1, 3), whose halo stays inside -> class 2 ...
    put(maps[1], 0, 5, 13)                # ... made class 1 by a stage-1 token at sites (10 .. 11, 26 .. 27)
    put(maps[2], 0, 6, 6)                 # sites 24 .. 27: three more class-2 tiles (an odd number of active tiles in all)
    put(maps[0], 1, 20, 20)               # frame 1: a stage-0 token inside tile (2, 2) -> class 0
    put(maps[2], 1, 6, 3)                 # sites (24 .. 27, 12 .. 15): tile (3, 1) -> class 2
    put(maps[1], 1, 4, 12)                # sites (8 .. 9, 24 .. 25): tile (1, 3), and (1, 2) through its halo -> class 1
    put(maps[2], 1, 0, 0)                 # a border tile: class 0 whatever it holds
    return maps, STRIDES, B, H, W


def scene_all_class0():
    """every active tile holds a stage-0 token or touches the border: the order is the identity"""
    B, H, W = 1, 24, 40
    maps = empty_maps(B, H, W, STRIDES)
    put(maps[0], 0, 12, 12)
    put(maps[0], 0, 9, 20)
    put(maps[1], 0, 5, 10)
    put(maps[2], 0, 0, 9)
    return maps, STRIDES, B, H, W


def scene_k2():
    """two source stages (strides 1, 2): classes capped at 1"""
    B, H, W = 1, 40, 40
    maps = empty_maps(B, H, W, (1, 2))
    put(maps[1], 0, 10, 10)               # sites 20 .. 21: tile (2, 2) -> class 1
    put(maps[1], 0, 5, 13)                # sites (10 .. 11, 26 .. 27): tile (1, 3) -> class 1 ...
    put(maps[0], 0, 9, 25)                # ... with a stage-0 token in its halo -> class 0
    put(maps[1], 0, 14, 5)                # sites (28 .. 29, 10 .. 11): tile (3, 1) -> class 1
    return maps, (1, 2), B, H, W
