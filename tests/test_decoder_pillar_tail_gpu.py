"""The pillar-row passes of the decoder head that are folded into their neighbours, through the C ABI, bit for bit against the
launches they replace (csrc/decoder.hip, csrc/conv_tiles.hip):

* gdmae_decoder_dy_rows  = gdmae_rows_bwd (c0 = c1 = 0) -> gdmae_decoder_dy
* gdmae_border_sums_rows = gdmae_rows_bwd (c0 = c1 = 0) -> gdmae_border_sums
* gdmae_tiles_gather_rows_affine_relu = gdmae_tiles_gather_rows -> gdmae_rows_affine_relu_scatter

One crafted map: B = 2, H = W = 20 (3 x 3 tiles of 8 x 8 sites, partial on both axes), C = 128; pillars on the four corners, on each border
row and column, in the interior; batch 0 has an active tile without any pillar, batch 1 an inactive tile that holds a border pillar (its
row is the border-class constant).  The conv output, a2 and b2 are small multiples of 1 / 8, so a2 * y + b2 is exactly 0 at many
entries and negative at many others; dout has all-zero rows and +0 / -0 entries.  Every output buffer starts NaN-filled."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
B, H, W, C = 2, 20, 20, 128
TH = TW = 3
M = 150


def dev():
    return torch.device("cuda:0")


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).numpy()


@functools.lru_cache(maxsize=None)
def _map():
    rng = np.random.default_rng(14)
    fixed = [(0, 0, 0), (0, 0, 19), (0, 19, 0), (0, 19, 19), (0, 0, 7), (0, 19, 9), (0, 5, 0), (0, 11, 19), (0, 3, 4), (0, 5, 6),
             (1, 0, 18), (1, 19, 19), (1, 0, 0), (1, 12, 0), (1, 19, 3), (1, 7, 19), (1, 9, 9), (1, 10, 12), (1, 8, 15)]
    cells = [(b * H + y) * W + x for b, y, x in fixed]
    # batch 0, tile (1, 1) (sites 8..15 x 8..15) stays without a pillar
    free = [c for c in range(B * H * W) if c not in cells and not (c < H * W and 8 <= (c // W) % H < 16 and 8 <= c % W < 16)]
    border = [c for c in free if (c // W) % H in (0, H - 1) or c % W in (0, W - 1)]
    extra = list(rng.choice(border, 40, replace=False))
    extra += list(rng.choice([c for c in free if c not in extra], M - len(cells) - 40, replace=False))
    pillar_cell = np.array(cells + extra, dtype=np.int32)[rng.permutation(M)]
    assert len(set(pillar_cell.tolist())) == M
    cell2pillar = np.full(B * H * W, -1, np.int32)
    cell2pillar[pillar_cell] = np.arange(M, dtype=np.int32)
    inactive = (1 * TH + 0) * TW + 2                      # batch 1, tile (0, 2): holds the pillar at (0, 18)
    tile_list = np.array([t for t in range(B * TH * TW) if t != inactive], dtype=np.int32)[rng.permutation(B * TH * TW - 1)]
    tile_slot = np.full(B * TH * TW, -1, np.int32)
    tile_slot[tile_list] = np.arange(len(tile_list), dtype=np.int32)
    n_act = len(tile_list)
    eighths = lambda shape, k: torch.from_numpy(rng.integers(-k, k + 1, shape) / 8.0).float()         # noqa: E731
    d = dev()
    m = dict(pillar_cell=torch.from_numpy(pillar_cell).to(d), cell2pillar=torch.from_numpy(cell2pillar).to(d),
             tile_list=torch.from_numpy(tile_list).to(d), tile_slot=torch.from_numpy(tile_slot).to(d), n_act=n_act,
             Yc=eighths((n_act * 64, C), 16).to(torch.bfloat16).to(d), ybg=eighths((9, C), 16).to(torch.bfloat16).to(d),
             a2=torch.from_numpy(rng.choice([0.5, 1.0, -1.0, 2.0, -0.5, 0.25], C)).float().to(d), b2=eighths((C,), 8).to(d),
             k0=torch.from_numpy(rng.standard_normal(C)).float().to(d), k1=torch.from_numpy(rng.standard_normal(C)).float().to(d))
    dout = torch.from_numpy(rng.standard_normal((M, C))).float()
    dout[3] = 0.0
    dout[40] = 0.0
    z = torch.from_numpy(rng.random((M, C)) < 0.1)
    dout[z] = 0.0
    dout[z & torch.from_numpy(rng.random((M, C)) < 0.5)] = -0.0
    assert (_bits(dout) == np.int32(-2 ** 31)).any() and (_bits(dout) == 0).any()
    m["dout"] = dout.to(d)
    return m


def _gather(m):
    from gdmae_hip import lib as L
    yrows = torch.full((M, C), float("nan"), dtype=torch.bfloat16, device=dev())
    L.call("gdmae_tiles_gather_rows", L.ptr(m["Yc"]), L.ptr(m["tile_slot"]), L.ptr(m["ybg"]), L.ptr(m["pillar_cell"]), M, H, W, C, 2,
           L.ptr(yrows), L.stream())
    return yrows


def _rows(yrows, a2, b2, dout, bf):
    from gdmae_hip import lib as L
    zero = torch.zeros(2 * C, device=dev())
    rows = torch.full((M, C), float("nan"), device=dev())
    L.call("gdmae_rows_bwd", L.ptr(yrows), bf, None, M, C, L.ptr(a2), L.ptr(b2), L.ptr(zero), L.ptr(zero[C:]), L.ptr(dout), 0, C, 0,
           L.ptr(rows), 0, L.stream())
    return rows


def _dy(m, rows=None, b2=None):
    from gdmae_hip import lib as L
    dYc = torch.full((m["n_act"] * 64, C), float("nan"), dtype=torch.bfloat16, device=dev())
    if rows is not None:
        L.call("gdmae_decoder_dy", L.ptr(m["Yc"]), L.ptr(m["tile_list"]), m["n_act"], L.ptr(m["k0"]), L.ptr(m["k1"]), L.ptr(rows),
               L.ptr(m["cell2pillar"]), H, W, C, L.ptr(dYc), L.stream())
    else:
        L.call("gdmae_decoder_dy_rows", L.ptr(m["Yc"]), L.ptr(m["tile_list"]), m["n_act"], L.ptr(m["k0"]), L.ptr(m["k1"]), L.ptr(m["dout"]),
               L.ptr(m["a2"]), L.ptr(m["b2"] if b2 is None else b2), L.ptr(m["cell2pillar"]), H, W, C, L.ptr(dYc), L.stream())
    return dYc


def _border(Y, bf, tile_slot, ybg, pillar_cell, rows=None, fused=None):
    from gdmae_hip import lib as L
    reg = torch.full((16, C), float("nan"), dtype=torch.float64, device=dev())
    ws = torch.empty(L.load().gdmae_border_sums_workspace_bytes(B, C), dtype=torch.uint8, device=dev())
    if rows is not None:
        L.call("gdmae_border_sums", L.ptr(Y), bf, L.ptr(tile_slot), L.ptr(ybg), L.ptr(rows), L.ptr(pillar_cell), M, B, H, W, C, L.ptr(reg),
               L.ptr(ws), L.stream())
    else:
        dout, yrows, a2, b2 = fused
        L.call("gdmae_border_sums_rows", L.ptr(Y), bf, L.ptr(tile_slot), L.ptr(ybg), L.ptr(dout), L.ptr(yrows), L.ptr(a2), L.ptr(b2),
               L.ptr(pillar_cell), M, B, H, W, C, L.ptr(reg), L.ptr(ws), L.stream())
    return reg


def test_the_map_exercises_the_relu_edges():
    m = _map()
    yrows = _gather(m).float()
    h = torch.addcmul(m["b2"], m["a2"], yrows)            # exact: products and sums of small multiples of 1 / 64
    live = m["dout"] != 0
    assert int(((h == 0) & live).sum()) > 50 and int(((h < 0) & live).sum()) > 1000 and int(((h > 0) & live).sum()) > 1000
    pc = m["pillar_cell"].cpu().numpy()
    y, x = (pc // W) % H, pc % W
    for sel in (y == 0, y == H - 1, x == 0, x == W - 1, (y == 0) & (x == 0), (y == 0) & (x == W - 1), (y == H - 1) & (x == 0),
                (y == H - 1) & (x == W - 1)):
        assert sel.any()
    # the pillar in the inactive tile reads the border-class constant (row 0, interior column: class 1)
    p = int(m["cell2pillar"][(1 * H + 0) * W + 18])
    assert torch.equal(yrows[p], m["ybg"][1].float())


def test_decoder_dy_rows_equals_rows_bwd_then_decoder_dy():
    m = _map()
    rows = _rows(_gather(m), m["a2"], m["b2"], m["dout"], 1)
    old = _dy(m, rows=rows)
    new, again = _dy(m), _dy(m)
    assert not torch.isnan(old.float()).any() and not torch.isnan(new.float()).any(), "unwritten rows"
    bad = np.argwhere(_bits(old) != _bits(new))
    assert bad.size == 0, (len(bad), bad[:6].tolist())
    assert np.array_equal(_bits(new), _bits(again))
    # the relu' path is live: with b2 of the other sign the pillar sites change
    assert not np.array_equal(_bits(_dy(m, b2=(-m["b2"]).contiguous())), _bits(new))


def test_border_sums_rows_equals_rows_bwd_then_border_sums():
    m = _map()
    yrows = _gather(m)
    rows = _rows(yrows, m["a2"], m["b2"], m["dout"], 1)
    old = _border(m["Yc"], 1, m["tile_slot"], m["ybg"], m["pillar_cell"], rows=rows)
    new = _border(m["Yc"], 1, m["tile_slot"], m["ybg"], m["pillar_cell"], fused=(m["dout"], yrows, m["a2"], m["b2"]))
    again = _border(m["Yc"], 1, m["tile_slot"], m["ybg"], m["pillar_cell"], fused=(m["dout"], yrows, m["a2"], m["b2"]))
    assert not torch.isnan(old).any() and not torch.isnan(new).any()
    bad = np.argwhere(_bits(old) != _bits(new))
    assert bad.size == 0, (len(bad), bad[:6].tolist())
    assert np.array_equal(_bits(new), _bits(again))
    assert float(new[8:].abs().sum()) > 0
    flipped = _border(m["Yc"], 1, m["tile_slot"], m["ybg"], m["pillar_cell"], fused=(m["dout"], yrows, m["a2"], (-m["b2"]).contiguous()))
    assert np.array_equal(_bits(flipped[:8]), _bits(new[:8])) and not np.array_equal(_bits(flipped[8:]), _bits(new[8:]))


def test_border_sums_rows_on_a_dense_fp32_map():
    """the fp32 instantiation: Y the plain (B H W, C) map (no tile table), yrows its rows at the pillar cells"""
    m = _map()
    g = torch.Generator().manual_seed(3)
    Y = (torch.randint(-16, 17, (B * H * W, C), generator=g) / 8.0).float().to(dev())
    yrows = Y[m["pillar_cell"].long()].contiguous()
    rows = _rows(yrows, m["a2"], m["b2"], m["dout"], 0)
    old = _border(Y, 0, None, None, m["pillar_cell"], rows=rows)
    new = _border(Y, 0, None, None, m["pillar_cell"], fused=(m["dout"], yrows, m["a2"], m["b2"]))
    assert not torch.isnan(new).any() and np.array_equal(_bits(old), _bits(new))


def test_gather_with_affine_relu_equals_the_two_launches():
    from gdmae_hip import lib as L
    m = _map()
    yrows_old = _gather(m)
    out_old = torch.full((M, C), float("nan"), device=dev())
    L.call("gdmae_rows_affine_relu_scatter", L.ptr(yrows_old), 1, None, M, C, L.ptr(m["a2"]), L.ptr(m["b2"]), L.ptr(out_old), 0, C, 0, L.stream())
    res = []
    for _ in range(2):
        yrows = torch.full((M, C), float("nan"), dtype=torch.bfloat16, device=dev())
        out = torch.full((M, C), float("nan"), device=dev())
        L.call("gdmae_tiles_gather_rows_affine_relu", L.ptr(m["Yc"]), L.ptr(m["tile_slot"]), L.ptr(m["ybg"]), L.ptr(m["pillar_cell"]), M, H, W, C,
               L.ptr(m["a2"]), L.ptr(m["b2"]), L.ptr(yrows), L.ptr(out), L.stream())
        res.append((yrows, out))
    for yr, out in res:
        assert np.array_equal(_bits(yr), _bits(yrows_old)) and np.array_equal(_bits(out), _bits(out_old))
    assert not torch.isnan(out_old).any() and int((out_old == 0).sum()) > 1000 and int((out_old > 0).sum()) > 1000
