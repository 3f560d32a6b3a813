"""RoI point pooling of the two-stage detector: ``RoILocalDFVSPool3dV2`` / ``gather_features`` with the reference's
interface (pcdet/ops/patch_ops/patch_ops_utils.py:10-22, 59-98) and ``roi_dfvs_pool``, the fused call ``GraphRCNNHead`` uses.

Device tensors go to ``gdmae_roi_dfvs_pool`` (csrc/roi_pool.hip); there is no fallback.  CPU tensors go to
``roi_dfvs_pool_cpu``, an op-by-op numpy statement of the same contract (slow, exact) - the arrangement of the anchor head's
``fused = False`` path.

The contract is deterministic where the reference races: a voxel is represented by its lowest ``points`` row, a
RoI with more than ``num_dvs_points`` voxels keeps the lowest rows, farthest-point sampling starts at the lowest row and
resolves ties towards the lowest row, a patch covered by more than ``num_boxes_per_patch`` RoIs keeps the lowest RoI
indices.  Every such outcome is one the reference can produce.  ``hash_size`` is accepted and unused: the voxel table never
drops a point, so the reference's probe-limit drops on a crowded table are not reproduced.
"""
import numpy as np
import torch
import torch.nn as nn


def gather_features(feats, pooled_pts_idx, pooled_pts_num):
    """feats (N, C), pooled_pts_idx (..., K), pooled_pts_num (...) -> (..., K, C); rows of empty RoIs stay zero."""
    pooled = feats.new_zeros(*pooled_pts_idx.shape, feats.shape[-1])
    ok = pooled_pts_num > 0
    pooled[ok] = feats[pooled_pts_idx[ok].long()]
    return pooled


def patch_grid(point_cloud_range):
    """(patch_lo (2,), (X, Y)) of the 1 m BEV patch grid over round(range -/+ 1) (graphrcnn_head.py:135-136)."""
    r = np.asarray(point_cloud_range, dtype=np.float32)
    pr = np.round(np.concatenate([r[:3] - 1, r[3:] + 1]))
    shape = np.round((pr[3:5] - pr[0:2]) / 1.0).astype(np.int32)
    return pr[:2].astype(np.float32), (int(shape[0]), int(shape[1]))


def _fps_fp32(xyz, rounds):
    """Indices of ``rounds`` farthest-point samples of xyz (n, 3) fp32, starting at 0; fp32 distances
    (dx dx + dy dy) + dz dz, minimum updated on d < d2, largest minimum wins, ties to the lowest index."""
    n = xyz.shape[0]
    mind = np.full(n, np.inf, dtype=np.float32)
    sel = np.zeros(rounds, dtype=np.int64)
    cur = 0
    for s in range(1, rounds):
        d = xyz - xyz[cur]
        d = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert d.dtype == np.float32
        mind = np.where(d < mind, d, mind)
        cur = int(np.argmax(mind))                     # first maximum = lowest index
        sel[s] = cur
    return sel


def roi_dfvs_pool_cpu(points, rois, range_xy, patch_lo, patch_shape, num_dvs_points, num_fps_points, lambda_, delta,
                      pool_extra_width, num_boxes_per_patch):
    """numpy statement of the pooling contract.  points (N, 1 + 3 + C) fp32 [batch, x, y, z, features], rois (B, M, >= 7).
    -> pooled_idx (B, M, K) int32, pooled_num (B, M) int32, feats_local (B M, K, 3 + C + 6) fp32, xyz_global (B M, K, 3) fp32."""
    f32 = np.float32
    pts = np.ascontiguousarray(points.detach().cpu().numpy().astype(f32))
    boxes = np.ascontiguousarray(rois.detach().cpu().numpy().astype(f32))[..., :7]
    B, M = boxes.shape[:2]
    K, C = int(num_fps_points), pts.shape[1] - 4
    X, Y = patch_shape
    lo = np.asarray(patch_lo, dtype=f32)
    extra = np.broadcast_to(np.asarray(pool_extra_width, dtype=f32), (3,))
    idx = np.zeros((B, M, K), dtype=np.int32)
    num = np.zeros((B, M), dtype=np.int32)
    feats = np.zeros((B * M, K, 3 + C + 6), dtype=f32)
    glob = np.zeros((B * M, K, 3), dtype=f32)
    x, y, z = pts[:, 1], pts[:, 2], pts[:, 3]
    rng = np.asarray(range_xy, dtype=f32)
    keep = (x >= rng[0]) & (x <= rng[2]) & (y >= rng[1]) & (y <= rng[3])
    px = np.clip((x - lo[0]).astype(np.int32), 0, X - 1)      # fp32 difference, truncated
    py = np.clip((y - lo[1]).astype(np.int32), 0, Y - 1)
    for b in range(B):
        rows_b = np.nonzero(keep & (pts[:, 0] == b))[0]
        covered = np.zeros((Y, X), dtype=np.int32)            # RoIs below the current one that cover each patch
        for r in range(M):
            box = boxes[b, r]
            cx, cy, cz, rz = box[0], box[1], box[2], box[6]
            dx, dy, dz = box[3] + extra[0], box[4] + extra[1], box[5] + extra[2]
            # truncated patch span of the rotated corners' bounding box (patch_query_gpu.cu:35-93)
            c, s = np.cos(rz), np.sin(rz)
            hx, hy = dx / f32(2), dy / f32(2)
            qx = np.array([cx - hx, cx + hx, cx + hx, cx - hx], dtype=f32) - cx
            qy = np.array([cy - hy, cy - hy, cy + hy, cy + hy], dtype=f32) - cy
            nx = qx * c + qy * (-s) + cx
            ny = qx * s + qy * c + cy
            span = [int(np.clip(v, -1e6, 1e6)) for v in (nx.min() - lo[0], ny.min() - lo[1], nx.max() - lo[0], ny.max() - lo[1])]
            x0, y0, x1, y1 = max(span[0], 0), max(span[1], 0), min(span[2], X - 1), min(span[3], Y - 1)
            if x1 < x0 or y1 < y0:
                continue
            allowed = covered[y0:y1 + 1, x0:x1 + 1] < num_boxes_per_patch
            covered[y0:y1 + 1, x0:x1 + 1] += 1
            cand = rows_b[(px[rows_b] >= x0) & (px[rows_b] <= x1) & (py[rows_b] >= y0) & (py[rows_b] <= y1)]
            cand = cand[allowed[py[cand] - y0, px[cand] - x0]]
            # in-box test of the enlarged RoI (roipatch_dfvs_pool3d_gpu.cu:63-72)
            cand = cand[np.abs(z[cand] - cz) <= dz / f32(2)]
            ca, sa = np.cos(-rz), np.sin(-rz)
            sx, sy = x[cand] - cx, y[cand] - cy
            lx = sx * ca + sy * (-sa)
            ly = sx * sa + sy * ca
            margin = float(f32(1e-5))
            inb = (np.abs(lx).astype(np.float64) < float(dx) / 2.0 + margin) & (np.abs(ly).astype(np.float64) < float(dy) / 2.0 + margin)
            cand, lx, ly = cand[inb], lx[inb], ly[inb]
            if cand.size == 0:
                continue
            # dynamic voxel (roipatch_dfvs_pool3d_gpu.cu:74-84)
            lz = z[cand] - cz
            res = max(0.02, float(f32(lambda_) * np.exp(-np.sqrt(cx * cx + cy * cy + cz * cz) / f32(delta))))
            out = [int(float(d) / res) for d in (dx, dy, dz)]
            vox = []
            for loc, d, o in ((lx, dx, out[0]), (ly, dy, out[1]), (lz, dz, out[2])):
                v = ((loc + d / f32(2)).astype(np.float64) / res).astype(np.int64)      # truncation
                vox.append(np.minimum(np.maximum(v, 0), o - 1))
            key = np.stack(vox, axis=1)
            _, first = np.unique(key, axis=0, return_index=True)       # cand ascends: the first occurrence is the lowest row
            reps = np.sort(cand[first])[:int(num_dvs_points)]
            n = reps.shape[0]
            num[b, r] = n
            sel = _fps_fp32(pts[reps, 1:4], min(K, n))
            slots = np.arange(K)
            slots = np.where(slots < n, slots, slots % n)
            rows = reps[sel[slots]]                                       # slot s >= n repeats slot s % n
            idx[b, r] = rows
            # features in fp64, rounded once (rotate_points_along_z by -heading; local corners of the un-enlarged RoI)
            p64 = pts[rows, 1:4].astype(np.float64)
            ox, oy = p64[:, 0] - float(cx), p64[:, 1] - float(cy)
            c64, s64 = np.cos(-float(rz)), np.sin(-float(rz))
            o = b * M + r
            feats[o, :, 0] = ox * c64 - oy * s64
            feats[o, :, 1] = ox * s64 + oy * c64
            feats[o, :, 2] = p64[:, 2] - float(cz)
            feats[o, :, 3:3 + C] = pts[rows, 4:]
            half = boxes[b, r, 3:6] / f32(2)
            feats[o, :, 3 + C:3 + C + 3] = -half
            feats[o, :, 3 + C + 3:] = half
            glob[o] = pts[rows, 1:4]
    dev = points.device
    return (torch.from_numpy(idx).to(dev), torch.from_numpy(num).to(dev), torch.from_numpy(feats).to(dev),
            torch.from_numpy(glob).to(dev))


_WORKSPACE = {}      # device -> uint8 scratch, grown on demand


def roi_dfvs_pool_hip(points, rois, range_xy, patch_lo, patch_shape, num_dvs_points, num_fps_points, hash_size, lambda_, delta,
                      pool_extra_width, num_boxes_per_patch, phases=3):
    """The same through ``gdmae_roi_dfvs_pool`` (device tensors)."""
    from gdmae_hip import lib as L
    points = points.float().contiguous()
    rois = rois.float().contiguous()
    B, M = rois.shape[:2]
    N, cols = points.shape
    K, C = int(num_fps_points), cols - 4
    dev = points.device
    idx = torch.empty(B, M, K, dtype=torch.int32, device=dev)
    num = torch.empty(B, M, dtype=torch.int32, device=dev)
    feats = torch.empty(B * M, K, 3 + C + 6, dtype=torch.float32, device=dev)
    glob = torch.empty(B * M, K, 3, dtype=torch.float32, device=dev)
    if B * M == 0:
        return idx, num, feats, glob
    X, Y = patch_shape
    need = int(L.load().gdmae_roi_dfvs_pool_workspace_bytes(N, B, M, X, Y))
    ws = _WORKSPACE.get(dev)
    if ws is None or ws.numel() < need:
        ws = _WORKSPACE[dev] = torch.empty(int(need * 1.25) + 256, dtype=torch.uint8, device=dev)
    extra = np.broadcast_to(np.asarray(pool_extra_width, dtype=np.float32), (3,))
    L.call("gdmae_roi_dfvs_pool", L.ptr(points), N, cols, L.ptr(rois), B, M, rois.shape[2], L.host_f32(list(range_xy)),
           L.host_f32(list(patch_lo)), X, Y, L.host_f32(list(extra)), int(num_dvs_points), K, int(hash_size), float(lambda_),
           float(delta), int(num_boxes_per_patch), int(phases), L.ptr(idx), L.ptr(num), L.ptr(feats), L.ptr(glob), L.ptr(ws),
           ws.numel(), L.stream())
    return idx, num, feats, glob


def roi_dfvs_pool(points, rois, range_xy, patch_lo, patch_shape, num_dvs_points, num_fps_points, hash_size, lambda_, delta,
                  pool_extra_width, num_boxes_per_patch):
    """Fused pooling: (pooled_idx, pooled_num, feats_local, xyz_global).  Device tensors: the HIP library; CPU tensors: numpy."""
    if points.is_cuda:
        return roi_dfvs_pool_hip(points, rois, range_xy, patch_lo, patch_shape, num_dvs_points, num_fps_points, hash_size,
                                 lambda_, delta, pool_extra_width, num_boxes_per_patch)
    return roi_dfvs_pool_cpu(points, rois, range_xy, patch_lo, patch_shape, num_dvs_points, num_fps_points, lambda_, delta,
                             pool_extra_width, num_boxes_per_patch)


class RoILocalDFVSPool3dV2(nn.Module):
    """Constructor keywords of the reference (patch_ops_utils.py:60).  ``pc_range`` is the PATCH range (the caller's
    round(point-cloud range -/+ 1)), ``patch_size`` [1, 1, -1].  ``hash_size`` is accepted and unused (module docstring)."""

    def __init__(self, pc_range, patch_size, num_dvs_points=1024, num_fps_points=256, hash_size=4099, lambda_=0.22, delta=70,
                 pool_extra_width=1.0, num_boxes_per_patch=16):
        super().__init__()
        self.pc_range = np.asarray(pc_range, dtype=np.float32)
        self.patch_size = np.asarray(patch_size, dtype=np.float32)
        if float(self.patch_size[0]) != 1.0 or float(self.patch_size[1]) != 1.0:
            raise NotImplementedError("RoILocalDFVSPool3dV2: only the 1 m BEV patch grid of the shipped head is built")
        self.num_dvs_points, self.num_fps_points, self.hash_size = num_dvs_points, num_fps_points, hash_size
        self.lambda_, self.delta = lambda_, delta
        self.pool_extra_width, self.num_boxes_per_patch = pool_extra_width, num_boxes_per_patch

    def _grid(self):
        shape = np.round((self.pc_range[3:5] - self.pc_range[0:2]) / self.patch_size[:2]).astype(np.int32)
        return self.pc_range[:2], (int(shape[0]), int(shape[1]))

    def pool(self, points, boxes3d, range_xy=None):
        """points (N, 1 + 3 + C), boxes3d (B, M, 7) -> (pooled_idx, pooled_num, feats_local, xyz_global).  ``range_xy``
        [x_min, y_min, x_max, y_max]: the point filter of the head (bounds inclusive); None keeps every point of the patch range."""
        lo, shape = self._grid()
        if range_xy is None:
            range_xy = [self.pc_range[0], self.pc_range[1], self.pc_range[3], self.pc_range[4]]
        return roi_dfvs_pool(points, boxes3d, range_xy, lo, shape, self.num_dvs_points, self.num_fps_points, self.hash_size,
                             self.lambda_, self.delta, self.pool_extra_width, self.num_boxes_per_patch)

    def forward(self, points, boxes3d):
        """points (N, 4) [batch_idx, x, y, z] inside the patch range, boxes3d (B, M, 7) -> pooled_pts_idx (B, M, K) int32 rows of
        ``points``, pooled_pts_num (B, M) int32."""
        assert points.dim() == 2 and points.shape[-1] == 4
        idx, num, _, _ = self.pool(points, boxes3d)
        return idx, num
