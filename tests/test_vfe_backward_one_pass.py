"""Backward of the two DynVFE point layers through the C ABI against an fp64 reference (k_v2_dydw computes dy1 and dW of the second
layer in one pass over the rows; the first layer's backward reads that dy1).

Forward on the GPU (gdmae_vfe_point_layer_fwd -> y1 in bf16 / fp16, gdmae_vfe_max_layer_fwd[_f16] -> out, arg), then
gdmae_vfe_max_layer_bwd[_f16] and gdmae_vfe_point_layer_bwd.  The reference is plain torch in fp64 on the CPU from the SAME rounded
inputs: layer 2 from the y1 rows the GPU wrote and the 16-bit rounding of W, the gradient routed to the arg-max rows the GPU chose
(checked to lie inside their pillars); layer 1 from the decorated points and the dy1 the GPU wrote.

Error = |got - want|_F / |want|_F.  The bound of every output is 2 x the worst error of the parent library (the separate k_v2_dy +
k_v2_dw kernels) over all the cases below, measured with this same test body; PARENT_WORST holds those figures:

    dy1 2.876e-3   dW2 3.720e-3   dgamma2 1.605e-7   dbeta2 9.317e-8   dW1 9.207e-4   dgamma1 3.590e-4   dbeta1 4.567e-6

(the fused kernel measures the same figures for dy1 to all digits shown: every dy1 element is the same chain of products as before.)
Determinism: two calls on the same inputs give bit-equal dy1 and dW."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# worst relative error of the parent commit's library per output, over all cases (sizes x row type)
PARENT_WORST = {"dy1": 2.876e-3, "dW2": 3.720e-3, "dgamma2": 1.605e-7, "dbeta2": 9.317e-8, "dW1": 9.207e-4, "dgamma1": 3.590e-4, "dbeta1": 4.567e-6}

CASES = {
    "crowded": [1, 700, 3, 1, 2600, 17, 2, 2, 1, 90, 31, 33, 1],      # a crowded pillar; N = 3 482 is not a multiple of 32
    "tiny": [1] * 300,                                                # 32 pillars per tile
    "one_tile": [5, 1, 9, 2],                                         # N = 17: less than one tile
    # 1 313 tiles, N % 32 = 24.  A workgroup takes four tiles per pass, so this is 329 workgroups - below the grid cap of 1 024: layer 1
    # (k_vfe1) makes ONE pass; later passes of its tile loop are reached by ``deep`` of tests/test_vfe_point_layer_gpu.py
    "many_tiles": [40] * 600 + [9000, 1, 7, 9000],
}
LO, VS, NX = (0.0, -40.0, -3.0), (0.32, 0.32, 6.0), 64


def _inputs(sizes, gen):
    """pillar-major rows [batch, x, y, z, intensity] inside their pillars' cells; every second pillar is made of identical rows"""
    N, M = sum(sizes), len(sizes)
    off = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int32)
    rowpil = torch.repeat_interleave(torch.arange(M, dtype=torch.int32), torch.tensor(sizes))
    coords = torch.stack([torch.zeros(M), torch.zeros(M), torch.arange(M) // NX, torch.arange(M) % NX], 1).long()   # (b, z, y, x)
    u = torch.rand(N, 3, generator=gen)
    for p in range(1, M, 2):
        u[off[p]:off[p + 1]] = u[off[p]].clone()
    cell = coords[rowpil.long()][:, [3, 2, 1]].float()
    xyz = (cell + u) * torch.tensor(VS) + torch.tensor(LO)
    inten = torch.rand(N, 1, generator=gen)
    for p in range(1, M, 2):
        inten[off[p]:off[p + 1]] = inten[off[p]].clone()
    pts = torch.cat([torch.zeros(N, 1), xyz, inten], 1).float().contiguous()
    mean = torch.stack([pts[off[p]:off[p + 1], 1:].mean(0) for p in range(M)]).float().contiguous()      # (M, F): every feature's mean
    return pts, coords, rowpil, off, mean


def _decorate(pts, coords, rowpil, mean):
    p, c = pts.double(), coords[rowpil.long()].double()
    centre = torch.stack([(c[:, 3] + 0.5) * float(np.float32(VS[0])) + LO[0], (c[:, 2] + 0.5) * float(np.float32(VS[1])) + LO[1],
                          (c[:, 1] + 0.5) * float(np.float32(VS[2])) + LO[2]], 1)
    return torch.cat([p[:, 1:4] - centre, p[:, 1:], p[:, 1:4] - mean.double()[rowpil.long()][:, :3]], 1)


def _bn_relu(h, g, b):
    return torch.relu((h - h.mean(0)) / torch.sqrt(h.var(0, unbiased=False) + 1e-3) * g + b)


def _run(sizes, f16):
    from gdmae_hip import lib as L
    d = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(len(sizes) * 13 + sizes[0] + int(f16))
    N, M, n_cols = sum(sizes), len(sizes), 5
    D = n_cols + 5
    pts, coords, rowpil, off, mean = _inputs(sizes, gen)
    W1, W2 = torch.randn(64, D, generator=gen) * 0.3, torch.randn(128, 64, generator=gen) * 0.2
    g1, b1 = torch.rand(64, generator=gen) + 0.5, torch.randn(64, generator=gen) * 0.3
    g2, b2 = torch.rand(128, generator=gen) + 0.5, torch.randn(128, generator=gen) * 0.3
    up = torch.randn(M, 128, generator=gen)
    ptsd, cd, rpd, offd, md = (t.to(d).contiguous() for t in (pts, coords, rowpil, off, mean))
    W1d, g1d, b1d, g2d, b2d, upd = (t.to(d).contiguous() for t in (W1, g1, b1, g2, b2, up))
    W2d = (W2 if f16 else W2.bfloat16()).to(d).contiguous()
    lo, vs = L.host_f32(LO), L.host_f32(VS)
    geo = (L.ptr(ptsd), L.ptr(cd), L.ptr(rpd), L.ptr(md), 1, N, n_cols, lo, vs)
    # forward, layer 1 then layer 2
    y1 = torch.empty(N, 64, dtype=torch.float16 if f16 else torch.bfloat16, device=d)
    st1, ab1, mv1 = torch.empty(128, dtype=torch.float64, device=d), torch.empty(128, device=d), torch.empty(128, device=d)
    ws1 = torch.empty(L.load().gdmae_vfe_point_layer_workspace_bytes(n_cols), dtype=torch.uint8, device=d)
    L.call("gdmae_vfe_point_layer_fwd", *geo, L.ptr(W1d), 64, L.ptr(g1d), L.ptr(b1d), 1e-3, 0.0, None, None, None, L.ptr(st1), L.ptr(ab1),
           L.ptr(mv1), L.ptr(y1), 2 if f16 else 1, L.ptr(ws1), L.stream())
    C = 128
    out = torch.empty(M, C, device=d)
    arg = torch.full((M, C), -7, dtype=torch.int32, device=d)
    st2, ab2, mv2 = torch.empty(2 * C, dtype=torch.float64, device=d), torch.empty(2 * C, device=d), torch.empty(2 * C, device=d)
    ws2 = torch.empty(L.load().gdmae_vfe_max_layer_workspace_bytes(), dtype=torch.uint8, device=d)
    sfx = "_f16" if f16 else ""
    L.call("gdmae_vfe_max_layer_fwd" + sfx, L.ptr(y1), N, L.ptr(W2d), L.ptr(offd), L.ptr(rpd), M, L.ptr(g2d), L.ptr(b2d), 1e-3, 0.0, None, None,
           None, L.ptr(st2), L.ptr(ab2), L.ptr(mv2), L.ptr(out), L.ptr(arg), L.ptr(ws2), L.stream())
    # backward, layer 2 (twice: determinism) then layer 1
    got2 = []
    for _ in range(2):
        gm, dy1 = torch.empty_like(out), torch.full((N, 64), float("nan"), dtype=torch.bfloat16, device=d)
        dg2, db2, dW2 = torch.empty(C, device=d), torch.empty(C, device=d), torch.empty(C, 64, device=d)
        L.call("gdmae_vfe_max_layer_bwd" + sfx, L.ptr(y1), N, L.ptr(W2d), L.ptr(rpd), M, L.ptr(g2d), L.ptr(st2), L.ptr(ab2), L.ptr(out),
               L.ptr(arg), L.ptr(upd), L.ptr(gm), L.ptr(dy1), L.ptr(dg2), L.ptr(db2), L.ptr(dW2), 0, L.ptr(ws2), L.stream())
        got2.append((dy1, dW2, dg2, db2))
    dg1, db1, dW1 = torch.empty(64, device=d), torch.empty(64, device=d), torch.empty(64, D, device=d)
    L.call("gdmae_vfe_point_layer_bwd", *geo, L.ptr(W1d), 64, L.ptr(g1d), L.ptr(st1), L.ptr(ab1), L.ptr(got2[0][0]), 1, L.ptr(dg1),
           L.ptr(db1), L.ptr(dW1), 0, L.ptr(ws1), L.stream())
    torch.cuda.synchronize()
    assert torch.equal(got2[0][0], got2[1][0]) and torch.equal(got2[0][1], got2[1][1]), "dy1 / dW differ between two calls"
    dy1, dW2, dg2, db2 = got2[0]
    assert bool(torch.isfinite(dy1.float()).all()), "a row of dy1 was not written"
    # fp64 reference, layer 2: from the rows the GPU wrote, routed to the rows it chose
    a = arg.cpu().long()
    assert bool(((a >= off[:-1].long()[:, None]) & (a < off[1:].long()[:, None])).all()), "arg-max row outside its pillar"
    yr = y1.cpu().double().requires_grad_()
    Wr = (W2.half() if f16 else W2.bfloat16()).double().requires_grad_()
    gr, br = g2.double().requires_grad_(), b2.double().requires_grad_()
    v = _bn_relu(yr @ Wr.t(), gr, br)
    (v.gather(0, a) * up.double()).sum().backward()
    want = {"dy1": yr.grad, "dW2": Wr.grad, "dgamma2": gr.grad, "dbeta2": br.grad}
    # layer 1: from the decorated points and the dy1 the GPU wrote
    W1r, g1r, b1r = W1.double().requires_grad_(), g1.double().requires_grad_(), b1.double().requires_grad_()
    y = _bn_relu(_decorate(pts, coords, rowpil, mean) @ W1r.t(), g1r, b1r)
    (y * dy1.cpu().double()).sum().backward()
    want.update({"dW1": W1r.grad, "dgamma1": g1r.grad, "dbeta1": b1r.grad})
    got = {"dy1": dy1, "dW2": dW2, "dgamma2": dg2, "dbeta2": db2, "dW1": dW1, "dgamma1": dg1, "dbeta1": db1}
    return {k: float((got[k].cpu().double() - want[k]).norm()) / max(float(want[k].norm()), 1e-12) for k in want}


@pytest.mark.parametrize("f16", [False, True], ids=["bf16_rows", "fp16_rows"])
@pytest.mark.parametrize("case", list(CASES))
def test_vfe_backward_against_fp64(case, f16):
    err = _run(CASES[case], f16)
    print(f"[vfe backward {case} {'fp16' if f16 else 'bf16'} rows] " + "  ".join(f"{k} {e:.3e}" for k, e in err.items()))
    for k, e in err.items():
        assert e <= 2 * PARENT_WORST[k], (k, e, PARENT_WORST[k])
