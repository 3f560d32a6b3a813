"""Plain numpy fp64 reference of the second stage after the pooling (GraphRCNNHead in eval mode).  Not a test.

Two statements of the head from a ``state_dict`` (numpy arrays, keys with or without the ``roi_head.`` prefix):

``statement_a``  op by op, as the reference module writes it: edge features [neighbour - centre, centre], 1 x 1 convolution,
                 BatchNorm affine, ReLU, max over the k neighbours, concat, calib gate, expansion, max over the K slots, reduction,
                 shortcut block, shared layer, heads, box decoding, score fusion.  Neighbours from fp64 direct squared distances,
                 ties to the lowest slot.
``statement_b``  the kernel's own decomposition (``fold``): BatchNorm folded into the weights FIRST, an edge layer as
                 ReLU(max_j P_j + Q_i) with P = (a W_nbr) x, Q = (a (W_ctr - W_nbr)) x + b; neighbours from the contract's fp32
                 d = (dx dx + dy dy) + dz dz.  ``bf16=True`` rounds (nearest even) exactly what the kernels round: the folded weights
                 of edge layers 2 / 3, calib W1 / W2 and the expansion (fp64 -> fp32 -> bf16), and the activations stored to the
                 128-channel tile (the three edge outputs, the gated tile) and the calib hidden tile (fp32 -> bf16).

``folded_flat`` is the fp32 buffer ``gdmae_roi_graph_pack`` takes, ``run_library`` calls the C ABI on device copies."""
import numpy as np

K_SLOTS, K_NBR, EPS = 256, 8, 1e-5
G = "attn_gnn_layer."


def state64(sd):
    """numpy fp64 copy, ``roi_head.`` prefix dropped, bookkeeping counters dropped"""
    out = {}
    for k, v in sd.items():
        k = str(k)
        if k.endswith("num_batches_tracked"):
            continue
        v = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        out[k[len("roi_head."):] if k.startswith("roi_head.") else k] = v.astype(np.float64)
    return out


def seeded_state(seed, negative_scales=False):
    """The fixture's seeded head state (tests/roi_head_seed.py) as fp64 numpy; ``negative_scales``: every BatchNorm of the graph
    network gets a seeded ~40 % of negative ``weight`` entries (the seeded ones are all >= 0.5: they cannot tell a BatchNorm scale
    folded after the max from one folded before it)."""
    import torch
    from gdmae_hip import configs
    from pcdet.models.roi_heads.graphrcnn_head import GraphRCNNHead
    from roi_head_seed import seeded_roi_head_state

    class Wrap(torch.nn.Module):
        def __init__(self):
            super().__init__()
            _, ds = configs.waymo_two_stage_cfg()
            self.roi_head = GraphRCNNHead(input_channels=5, model_cfg=configs.graphrcnn_head_cfg(), point_cloud_range=ds.point_cloud_range,
                                          num_class=1)
    sd = state64(seeded_roi_head_state(Wrap(), seed))
    if negative_scales:
        rng = np.random.default_rng(seed + 7)
        for k in sorted(sd):
            if k.startswith(G) and k.endswith(".weight") and sd[k].ndim == 1:
                sd[k] = sd[k] * np.where(rng.random(sd[k].shape) < 0.4, -1.0, 1.0)
    return sd


def _bn(sd, p):
    a = sd[p + ".weight"] / np.sqrt(sd[p + ".running_var"] + EPS)
    return a, sd[p + ".bias"] - a * sd[p + ".running_mean"]


def _w(sd, k):
    w = sd[k]
    return w.reshape(w.shape[0], w.shape[1])


def neighbours(xyz, fp32):
    """xyz (T, K, 3) -> (T, K, 8) slots with the smallest squared distance, the slot itself included, ties to the lowest slot"""
    x = xyz.astype(np.float32 if fp32 else np.float64)
    d = x[:, None, :, :] - x[:, :, None, :]                       # [t, i, j] = x_j - x_i
    d = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d.dtype == x.dtype
    return np.argsort(d, axis=-1, kind="stable")[..., :K_NBR]


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _decode(reg, cls, rois, roi_scores, normalized):
    """rcnn_reg (T, 7), rcnn_cls (T, 1), rois (B, M, >= 7), roi_scores (B, M) -> boxes (B, M, 7), scores (B, M, 1)"""
    B, M = rois.shape[:2]
    r = rois.reshape(B * M, -1).astype(np.float64)
    diag = np.sqrt(r[:, 3] ** 2 + r[:, 4] ** 2)
    xl, yl, zl = reg[:, 0] * diag, reg[:, 1] * diag, reg[:, 2] * r[:, 5]
    c, s = np.cos(r[:, 6]), np.sin(r[:, 6])
    box = np.stack([xl * c - yl * s + r[:, 0], xl * s + yl * c + r[:, 1], zl + r[:, 2], np.exp(reg[:, 3]) * r[:, 3],
                    np.exp(reg[:, 4]) * r[:, 4], np.exp(reg[:, 5]) * r[:, 5], reg[:, 6] + r[:, 6]], axis=1)
    ps = roi_scores.reshape(-1).astype(np.float64)
    ps = ps if normalized else _sigmoid(ps)
    score = np.sqrt(_sigmoid(cls[:, 0])) * np.sqrt(ps)
    return box.reshape(B, M, 7), score.reshape(B, M, 1)


def _inputs(feats, num):
    x = feats.astype(np.float64) * (np.asarray(num).reshape(-1) > 0)[:, None, None]
    assert x.shape[1:] == (K_SLOTS, 11)
    return x


def statement_a(sd, feats, num, rois, roi_scores, normalized=True):
    sd = state64(sd)
    x = _inputs(feats, num)
    T = x.shape[0]
    idx = neighbours(x[..., :3], fp32=False)
    t = np.arange(T)[:, None, None]
    outs = []
    for l in range(3):
        W = _w(sd, f"{G}edge_layes.{l}.0.weight")
        a, b = _bn(sd, f"{G}edge_layes.{l}.1")
        nb = x[t, idx]                                                        # (T, K, k, C)
        ctr = np.broadcast_to(x[:, :, None, :], nb.shape)
        e = np.concatenate([nb - ctr, ctr], axis=-1)                          # (T, K, k, 2 C)
        y = np.maximum(a * (e @ W.T) + b, 0.0)
        x = y.max(axis=2)
        outs.append(x)
    x = np.concatenate(outs, axis=-1)                                         # (T, K, 128)
    a, b = _bn(sd, G + "calib.1")
    h = np.maximum(a * (x @ _w(sd, G + "calib.0.weight").T) + b, 0.0)
    x = _sigmoid(h @ _w(sd, G + "calib.3.weight").T + sd[G + "calib.3.bias"]) * x
    a, b = _bn(sd, G + "expansion.1")
    v = np.maximum(a * (x @ _w(sd, G + "expansion.0.weight").T) + b, 0.0).max(axis=1)          # (T, 512)
    a, b = _bn(sd, G + "reduction.1")
    v = np.maximum(a * (v @ _w(sd, G + "reduction.0.weight").T) + b, 0.0)
    v = v + v                                                                 # x + dropout1(x) in eval
    a, b = _bn(sd, G + "shortcut.norm1")
    v = a * v + b
    v2 = np.maximum(v @ _w(sd, G + "shortcut.conv1.weight").T + sd[G + "shortcut.conv1.bias"], 0.0)
    v2 = v2 @ _w(sd, G + "shortcut.conv2.weight").T + sd[G + "shortcut.conv2.bias"]
    a, b = _bn(sd, G + "shortcut.norm2")
    v = a * (v + v2) + b
    a, b = _bn(sd, "shared_fc_layer.1")
    s = np.maximum(a * (v @ _w(sd, "shared_fc_layer.0.weight").T) + b, 0.0)
    cls = s @ _w(sd, "cls_layers.weight").T + sd["cls_layers.bias"]
    reg = s @ _w(sd, "reg_layers.weight").T + sd["reg_layers.bias"]
    box, score = _decode(reg, cls, rois, roi_scores, normalized)
    return {"rcnn_cls": cls, "rcnn_reg": reg, "batch_box_preds": box, "batch_cls_preds": score, "nbr": idx}


FOLDED_ORDER = ("e1_P", "e1_Q", "e1_b", "e2_P", "e2_Q", "e2_b", "e3_P", "e3_Q", "e3_b", "c1_W", "c1_b", "c2_W", "c2_b", "ex_W", "ex_b",
                "rd_W", "rd_b", "n1_a", "n1_b", "s1_W", "s1_b", "s2_W", "s2_b", "n2_a", "n2_b", "fc_W", "fc_b", "hd_W", "hd_b")
BF16_WEIGHTS = ("e2_P", "e2_Q", "e3_P", "e3_Q", "c1_W", "c2_W", "ex_W")


def fold(sd):
    """fp64 folded weights in the order and under the names of the C ABI's ``folded`` buffer"""
    sd = state64(sd)
    f = {}
    for l in range(3):
        W = _w(sd, f"{G}edge_layes.{l}.0.weight")
        a, b = _bn(sd, f"{G}edge_layes.{l}.1")
        c = W.shape[1] // 2
        f[f"e{l + 1}_P"], f[f"e{l + 1}_Q"], f[f"e{l + 1}_b"] = a[:, None] * W[:, :c], a[:, None] * (W[:, c:] - W[:, :c]), b
    a, b = _bn(sd, G + "calib.1")
    f["c1_W"], f["c1_b"] = a[:, None] * _w(sd, G + "calib.0.weight"), b
    f["c2_W"], f["c2_b"] = _w(sd, G + "calib.3.weight"), sd[G + "calib.3.bias"]
    for name, conv, bn in (("ex", G + "expansion.0", G + "expansion.1"), ("rd", G + "reduction.0", G + "reduction.1"),
                           ("fc", "shared_fc_layer.0", "shared_fc_layer.1")):
        a, b = _bn(sd, bn)
        f[name + "_W"], f[name + "_b"] = a[:, None] * _w(sd, conv + ".weight"), b
    a, b = _bn(sd, G + "shortcut.norm1")
    f["n1_a"], f["n1_b"] = 2.0 * a, b
    f["s1_W"], f["s1_b"] = _w(sd, G + "shortcut.conv1.weight"), sd[G + "shortcut.conv1.bias"]
    f["s2_W"], f["s2_b"] = _w(sd, G + "shortcut.conv2.weight"), sd[G + "shortcut.conv2.bias"]
    f["n2_a"], f["n2_b"] = _bn(sd, G + "shortcut.norm2")
    f["hd_W"] = np.concatenate([_w(sd, "cls_layers.weight"), _w(sd, "reg_layers.weight")], axis=0)
    f["hd_b"] = np.concatenate([sd["cls_layers.bias"], sd["reg_layers.bias"]])
    assert f["hd_W"].shape == (8, 256) and f["e1_P"].shape == (32, 11) and f["e3_Q"].shape == (64, 32) and f["ex_W"].shape == (512, 128)
    return {k: f[k] for k in FOLDED_ORDER}


def folded_flat(sd):
    return np.concatenate([v.reshape(-1) for v in fold(sd).values()]).astype(np.float32)


def round_bf16(x):
    """fp64 / fp32 -> fp32 -> bf16, round to nearest even; returned as fp64"""
    u = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64).reshape(np.shape(x))


def statement_b(sd, feats, num, rois, roi_scores, normalized=True, bf16=False):
    f = fold(sd)
    if bf16:
        f = {k: v.astype(np.float32).astype(np.float64) for k, v in f.items()}          # the library takes fp32
        for k in BF16_WEIGHTS:
            f[k] = round_bf16(f[k])
    r = round_bf16 if bf16 else (lambda v: v)
    x = _inputs(feats, num)
    T = x.shape[0]
    idx = neighbours(x[..., :3], fp32=True)
    t = np.arange(T)[:, None, None]
    outs = []
    for l in (1, 2, 3):
        P, Q = x @ f[f"e{l}_P"].T, x @ f[f"e{l}_Q"].T
        x = r(np.maximum((P[t, idx].max(axis=2) + Q) + f[f"e{l}_b"], 0.0))
        outs.append(x)
    x = np.concatenate(outs, axis=-1)
    h = r(np.maximum(x @ f["c1_W"].T + f["c1_b"], 0.0))
    x = r(x * _sigmoid(h @ f["c2_W"].T + f["c2_b"]))
    v = np.maximum((x @ f["ex_W"].T).max(axis=1) + f["ex_b"], 0.0)
    v = f["n1_a"] * np.maximum(v @ f["rd_W"].T + f["rd_b"], 0.0) + f["n1_b"]
    h = np.maximum(v @ f["s1_W"].T + f["s1_b"], 0.0)
    v = f["n2_a"] * (v + (h @ f["s2_W"].T + f["s2_b"])) + f["n2_b"]
    s = np.maximum(v @ f["fc_W"].T + f["fc_b"], 0.0)
    o = s @ f["hd_W"].T + f["hd_b"]
    cls, reg = o[:, :1], o[:, 1:]
    box, score = _decode(reg, cls, rois, roi_scores, normalized)
    return {"rcnn_cls": cls, "rcnn_reg": reg, "batch_box_preds": box, "batch_cls_preds": score, "nbr": idx}


OUTPUTS = ("rcnn_cls", "rcnn_reg", "batch_box_preds", "batch_cls_preds")


def deviation(got, want):
    return {k: float(np.abs(np.asarray(got[k], dtype=np.float64) - np.asarray(want[k], dtype=np.float64)).max(initial=0.0)) for k in OUTPUTS}


def same_neighbour_sets(a, b):
    return bool(np.array_equal(np.sort(np.asarray(a), axis=-1), np.sort(np.asarray(b), axis=-1)))


_PACKED = {}


def run_library(sd, feats, num, rois, roi_scores, normalized=True, key=None):
    """The C ABI on device copies -> the four outputs and the neighbour slots, as numpy.  ``key``: cache the packed image."""
    import torch
    from gdmae_hip import lib as L
    lib = L.load()
    dev = torch.device("cuda")
    packed = _PACKED.get(key) if key is not None else None
    if packed is None:
        flat = torch.from_numpy(folded_flat(sd)).to(dev)
        assert flat.numel() == lib.gdmae_roi_graph_folded_floats()
        packed = torch.empty(lib.gdmae_roi_graph_packed_bytes(), dtype=torch.uint8, device=dev)
        L.call("gdmae_roi_graph_pack", L.ptr(flat), L.ptr(packed), L.stream())
        torch.cuda.synchronize()
        if key is not None:
            _PACKED[key] = packed
    B, M = rois.shape[:2]
    T = B * M
    f = torch.from_numpy(np.ascontiguousarray(feats, dtype=np.float32)).to(dev)
    n = torch.from_numpy(np.ascontiguousarray(np.asarray(num).reshape(-1), dtype=np.int32)).to(dev)
    r = torch.from_numpy(np.ascontiguousarray(rois, dtype=np.float32)).to(dev)
    s = torch.from_numpy(np.ascontiguousarray(roi_scores, dtype=np.float32)).to(dev)
    assert f.shape == (T, K_SLOTS, 11) and n.shape == (T,) and s.shape == (B, M)
    cls = torch.empty(T, 1, dtype=torch.float32, device=dev)
    reg = torch.empty(T, 7, dtype=torch.float32, device=dev)
    box = torch.empty(B, M, 7, dtype=torch.float32, device=dev)
    score = torch.empty(B, M, 1, dtype=torch.float32, device=dev)
    nbr = torch.full((T, K_SLOTS, K_NBR), -1, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.gdmae_roi_graph_workspace_bytes(T), dtype=torch.uint8, device=dev)
    L.call("gdmae_roi_graph_forward", L.ptr(f), L.ptr(n), L.ptr(r), r.shape[2], L.ptr(s), B, M, int(bool(normalized)), L.ptr(packed),
           L.ptr(cls), L.ptr(reg), L.ptr(box), L.ptr(score), L.ptr(nbr), L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    return {"rcnn_cls": cls.cpu().numpy(), "rcnn_reg": reg.cpu().numpy(), "batch_box_preds": box.cpu().numpy(),
            "batch_cls_preds": score.cpu().numpy(), "nbr": nbr.cpu().numpy()}


# ---- crafted pooled tensors on a 1/64 m lattice: distances are exact in fp32, ties are genuine
def lattice_roi(rng, n, grid=False):
    """feats_local (256, 11) of a RoI with ``n`` distinct pooled points (slot s >= n repeats slot s % n; n = 0: zero rows).
    ``grid``: the points sit on a regular 1/4 m grid, so that several distinct points tie at the 8th place."""
    f = np.zeros((K_SLOTS, 11), dtype=np.float32)
    if n == 0:
        return f
    if grid:
        g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(4), indexing="ij"), axis=-1).reshape(-1, 3)
        assert n <= g.shape[0]
        xyz = (g[rng.permutation(g.shape[0])[:n]] * 16 - np.array([56, 56, 24])) / 64.0
    else:
        cells = rng.choice(257 * 129 * 65, size=n, replace=False)
        xyz = (np.stack([cells % 257, cells // 257 % 129, cells // (257 * 129)], axis=1) - np.array([128, 64, 32])) / 64.0
    pts = np.concatenate([xyz, rng.integers(0, 64, (n, 2)) / 64.0], axis=1).astype(np.float32)
    s = np.arange(K_SLOTS)
    f[:, :5] = pts[np.where(s < n, s, s % n)]
    half = np.array([2.25, 1.0, 0.875], dtype=np.float32)
    f[:, 5:8], f[:, 8:] = -half, half
    return f


def lattice_case(seed, B, M, nums, grid_rois=()):
    """-> feats (B M, 256, 11), pooled_num (B M), rois (B, M, 7), roi_scores (B, M); ``nums``: pooled points per RoI"""
    rng = np.random.default_rng(seed)
    assert len(nums) == B * M
    feats = np.stack([lattice_roi(rng, int(n), grid=i in grid_rois) for i, n in enumerate(nums)])
    rois = np.zeros((B, M, 7), dtype=np.float32)
    rois[..., 0:2] = rng.uniform(-60, 60, (B, M, 2))
    rois[..., 2] = rng.uniform(0, 2, (B, M))
    rois[..., 3:6] = np.array([4.5, 2.0, 1.75]) * rng.uniform(0.8, 1.25, (B, M, 3))
    rois[..., 6] = rng.uniform(-np.pi, np.pi, (B, M))
    return feats, np.asarray(nums, dtype=np.int32), rois, rng.uniform(0.1, 0.95, (B, M)).astype(np.float32)
