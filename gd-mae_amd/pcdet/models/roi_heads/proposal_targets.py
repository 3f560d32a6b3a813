"""Proposal targets of the second stage (reference ``ProposalTargetLayer``, target_assigner/proposal_target_layer.py:13-230, with
the canonical transformation of ``assign_targets``, roi_head_template.py:104-127) for the whole batch, under one contract
 that restates the reference wherever it is deterministic and fixes the rest:

* valid GT rows of a sample: 0 .. k, k the last row with a non-zero entry (k = 0 without one);
* overlap = rotated BEV overlap x height overlap / max(vol_a + vol_b - overlap, 1e-6); with ``SAMPLE_ROI_BY_EACH_CLASS`` only GT
  rows of the RoI's label count; the LOWEST row with the largest overlap is assigned, row 0 with overlap 0 when there is none;
* fg: overlap >= min(REG_FG_THRESH, CLS_FG_THRESH); easy bg: < CLS_BG_THRESH_LO; hard bg: the rest below REG_FG_THRESH; lists in
  RoI order, comparisons in fp32;
* sampling from uniform numbers the host drew up front: the f = min(fg_per_image, n_fg) fg RoIs with the smallest
  (``u_fg``, RoI index) fill slots 0 .. f - 1 in that order; of the nb remaining slots the first min(hard_quota[nb], n_hard) draw
  from the hard list and the rest from the easy list (all of them from the one list that is not empty), slot j taking element
  min(int(u_bg[j] n), n - 1) with the product in fp32; without any background every slot draws from the fg list that way.

``roi_targets`` sends device tensors to ``gdmae_roi_targets`` (csrc/roi_targets.hip; no fallback) and CPU tensors to
``roi_targets_numpy``, the op-by-op statement with fp64 geometry - the split of ``pcdet.ops.patch_ops``."""
import math

import numpy as np
import torch

MAX_ROWS = 1024          # RoIs, GT rows and sampled RoIs per sample the kernel holds in LDS
FIELDS = ('rois', 'roi_scores', 'roi_labels', 'roi_indices', 'gt_iou_of_rois', 'gt_of_rois_src', 'gt_of_rois', 'reg_valid_mask',
          'rcnn_cls_labels')


def sampler_params(cfg):
    """TARGET_CONFIG -> dict of what the contract reads; ``hard_quota[nb] = int(nb * HARD_BG_RATIO)`` in Python, as the reference
    truncates it."""
    R = int(cfg.ROI_PER_IMAGE)
    kind = cfg.CLS_SCORE_TYPE
    if kind not in ('roi_iou', 'cls'):
        raise NotImplementedError(f"TARGET_CONFIG.CLS_SCORE_TYPE {kind}: only roi_iou and cls are built")
    return dict(R=R, fg_per_image=int(np.round(cfg.FG_RATIO * R)), reg_fg=float(cfg.REG_FG_THRESH), cls_fg=float(cfg.CLS_FG_THRESH),
                cls_bg=float(cfg.CLS_BG_THRESH), cls_bg_lo=float(cfg.CLS_BG_THRESH_LO),
                hard_quota=np.array([int(nb * cfg.HARD_BG_RATIO) for nb in range(R + 1)], dtype=np.int32),
                by_class=bool(cfg.get('SAMPLE_ROI_BY_EACH_CLASS', False)), cls_type=kind)


def check_sizes(M, G, R, cols):
    for name, v in (("RoIs per sample", M), ("GT rows per sample", G), ("ROI_PER_IMAGE", R)):
        if v > MAX_ROWS:
            raise NotImplementedError(f"proposal_targets: {name} = {v} > {MAX_ROWS} is not built (the lists and the sort live in LDS)")
    if cols != 7:
        raise NotImplementedError(f"proposal_targets: RoIs of {cols} columns are not built (7 only)")
    if M < 1 or G < 1:
        raise NotImplementedError("proposal_targets: needs at least one RoI row and one GT row per sample (padded rows count)")


# ------------------------------------------------------------------------------------------------------------------------------
# numpy statement (fp64 geometry)
# ------------------------------------------------------------------------------------------------------------------------------
def exact_bev_overlap(a, b):
    """Area of the intersection of the BEV rectangles of two boxes [x, y, z, dx, dy, dz, heading]: convex clipping in fp64."""
    def corners(bx):
        c, s = math.cos(bx[6]), math.sin(bx[6])
        return [(bx[0] + lx * c - ly * s, bx[1] + lx * s + ly * c)
                for lx, ly in ((-bx[3] / 2, -bx[4] / 2), (bx[3] / 2, -bx[4] / 2), (bx[3] / 2, bx[4] / 2), (-bx[3] / 2, bx[4] / 2))]
    poly, clip = corners([float(v) for v in a]), corners([float(v) for v in b])
    for i in range(4):
        p0, p1 = clip[i], clip[(i + 1) % 4]
        ex, ey = p1[0] - p0[0], p1[1] - p0[1]
        side = [ex * (q[1] - p0[1]) - ey * (q[0] - p0[0]) for q in poly]
        new = []
        for k, c in enumerate(poly):
            n, sc, sn = poly[(k + 1) % len(poly)], side[k], side[(k + 1) % len(poly)]
            if sc >= 0:
                new.append(c)
            if (sc >= 0) != (sn >= 0):
                t = sc / (sc - sn)
                new.append((c[0] + t * (n[0] - c[0]), c[1] + t * (n[1] - c[1])))
        poly = new
        if not poly:
            return 0.0
    return abs(sum(poly[k][0] * poly[(k + 1) % len(poly)][1] - poly[(k + 1) % len(poly)][0] * poly[k][1] for k in range(len(poly)))) / 2


def iou3d_fp64(a, b, bev_overlap=exact_bev_overlap):
    a, b = [float(v) for v in a[:7]], [float(v) for v in b[:7]]
    oh = max(min(a[2] + a[5] / 2, b[2] + b[5] / 2) - max(a[2] - a[5] / 2, b[2] - b[5] / 2), 0.0)
    if oh == 0.0 or a[3] * a[4] == 0.0 or b[3] * b[4] == 0.0:
        return 0.0
    o3 = bev_overlap(a, b) * oh
    return o3 / max(a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - o3, 1e-6)


def valid_gt_rows(gt):
    """gt (G, 8) -> number of valid rows: 1 + the last row with a non-zero entry (1 when there is none)."""
    nz = np.nonzero((gt != 0).any(axis=1))[0]
    return int(nz[-1]) + 1 if nz.size else 1


def match(rois, labels, gt, by_class, bev_overlap=exact_bev_overlap):
    """One sample: rois (M, 7), labels (M), gt (G, 8) -> (overlap (M) fp64, assigned GT row (M), all overlaps (M, valid rows) with
    nan where the classes differ)."""
    n = valid_gt_rows(gt)
    M = rois.shape[0]
    best, row, full = np.zeros(M), np.zeros(M, dtype=np.int64), np.full((M, n), np.nan)
    gl = gt[:n, 7].astype(np.int64)
    for r in range(M):
        seen = False
        for g in range(n):
            if by_class and gl[g] != labels[r]:
                continue
            v = full[r, g] = iou3d_fp64(rois[r], gt[g], bev_overlap)
            if not seen or v > best[r]:
                best[r], row[r], seen = v, g, True
    return best, row, full


def limit_period(v, period):
    return v - np.floor(v / period + 0.5) * period


def sample(iou32, u_fg, u_bg, P):
    """One sample: overlaps (M) fp32, u_fg (M) fp32, u_bg (R) fp32 -> (RoI index per output slot (R), dict of the counts)."""
    f32 = np.float32
    assert iou32.dtype == f32 and u_fg.dtype == f32 and u_bg.dtype == f32
    R = P['R']
    fg = np.nonzero(iou32 >= min(f32(P['reg_fg']), f32(P['cls_fg'])))[0]
    easy = np.nonzero(iou32 < f32(P['cls_bg_lo']))[0]
    hard = np.nonzero((iou32 < f32(P['reg_fg'])) & (iou32 >= f32(P['cls_bg_lo'])))[0]

    def draw(lst, j):
        n = f32(len(lst))
        p = u_bg[j] * n
        assert p.dtype == f32
        return lst[min(int(p), len(lst) - 1)]
    n_bg = len(hard) + len(easy)
    f = 0 if n_bg == 0 else min(P['fg_per_image'], len(fg))
    nb = R - f
    h = 0
    if len(hard) and len(easy):
        h = min(int(P['hard_quota'][nb]), len(hard))
    elif len(hard):
        h = nb
    order = sorted(fg, key=lambda i: (u_fg[i], i))
    out = np.zeros(R, dtype=np.int64)
    for j in range(R):
        if j < f:
            out[j] = order[j]
        elif n_bg == 0:
            out[j] = draw(fg, j)
        elif j - f < h:
            out[j] = draw(hard, j)
        else:
            out[j] = draw(easy, j)
    return out, dict(n_fg=len(fg), n_hard=len(hard), n_easy=len(easy), f=f, h=h)


def roi_targets_numpy(rois, roi_scores, roi_labels, gt_boxes, u_fg, u_bg, P, forced_indices=None, bev_overlap=exact_bev_overlap):
    """numpy arrays in, dict of numpy arrays out (``FIELDS``; integers int64, the rest fp32).  ``forced_indices`` (B, R) replaces
    the sampling step."""
    f32 = np.float32
    rois, roi_scores, gt_boxes = np.asarray(rois, f32), np.asarray(roi_scores, f32), np.asarray(gt_boxes, f32)
    roi_labels = np.asarray(roi_labels).astype(np.int64)
    B, M, cols = rois.shape
    R = P['R']
    check_sizes(M, gt_boxes.shape[1], R, cols)
    out = dict(rois=np.zeros((B, R, 7), f32), roi_scores=np.zeros((B, R), f32), roi_labels=np.zeros((B, R), np.int64),
               roi_indices=np.zeros((B, R), np.int64), gt_iou_of_rois=np.zeros((B, R), f32), gt_of_rois_src=np.zeros((B, R, 8), f32),
               gt_of_rois=np.zeros((B, R, 8), f32), reg_valid_mask=np.zeros((B, R), np.int64),
               rcnn_cls_labels=np.zeros((B, R), f32 if P['cls_type'] == 'roi_iou' else np.int64))
    reg_fg, cls_fg, cls_bg = f32(P['reg_fg']), f32(P['cls_fg']), f32(P['cls_bg'])
    for b in range(B):
        best, row, _ = match(rois[b], roi_labels[b], gt_boxes[b], P['by_class'], bev_overlap)
        iou32 = best.astype(f32)
        if forced_indices is not None:
            idx = np.asarray(forced_indices[b]).astype(np.int64)
        else:
            idx, _ = sample(iou32, np.asarray(u_fg[b], f32), np.asarray(u_bg[b], f32), P)
        v = iou32[idx]
        out['rois'][b], out['roi_scores'][b], out['roi_labels'][b], out['roi_indices'][b] = rois[b, idx], roi_scores[b, idx], roi_labels[b, idx], idx
        out['gt_iou_of_rois'][b] = v
        g = gt_boxes[b, row[idx]]
        out['gt_of_rois_src'][b] = g
        out['reg_valid_mask'][b] = v > reg_fg
        if P['cls_type'] == 'cls':
            lab = (v > cls_fg).astype(np.int64)
            lab[(v > cls_bg) & (v < cls_fg)] = -1
        else:
            lin = (v.astype(np.float64) - float(cls_bg)) / (float(cls_fg) - float(cls_bg))
            lab = np.where(v > cls_fg, 1.0, np.where(v < cls_bg, 0.0, lin)).astype(f32)
        out['rcnn_cls_labels'][b] = lab
        # canonical frame of the RoI, fp64, rounded once
        r64, g64 = rois[b, idx].astype(np.float64), g.astype(np.float64)
        ry = limit_period(r64[:, 6], 2 * np.pi)
        d = g64[:, :3] - r64[:, :3]
        ca, sa = np.cos(-ry), np.sin(-ry)
        ct = g64.copy()
        ct[:, 0] = d[:, 0] * ca - d[:, 1] * sa
        ct[:, 1] = d[:, 0] * sa + d[:, 1] * ca
        ct[:, 2] = d[:, 2]
        ct[:, 6] = limit_period(g64[:, 6] - ry, np.pi)
        out['gt_of_rois'][b] = ct
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# device path
# ------------------------------------------------------------------------------------------------------------------------------
_WORKSPACE = {}      # device -> uint8 scratch, grown on demand
_QUOTA = {}          # (device, quota bytes) -> int32 device tensor


def roi_targets_hip(rois, roi_scores, roi_labels, gt_boxes, u_fg, u_bg, P):
    """Device tensors through ``gdmae_roi_targets``: no host read, two launches."""
    from gdmae_hip import lib as L
    B, M, cols = rois.shape
    G, R = gt_boxes.shape[1], P['R']
    check_sizes(M, G, R, cols)
    assert gt_boxes.shape[2] == 8 and tuple(u_fg.shape) == (B, M) and tuple(u_bg.shape) == (B, R)
    dev = rois.device
    rois, roi_scores, gt_boxes = rois.float().contiguous(), roi_scores.float().contiguous(), gt_boxes.float().contiguous()
    labels = roi_labels.to(torch.int32).contiguous()
    u_fg, u_bg = u_fg.float().contiguous(), u_bg.float().contiguous()
    qk = (dev, P['hard_quota'].tobytes())
    if qk not in _QUOTA:
        _QUOTA[qk] = torch.from_numpy(P['hard_quota']).to(dev)
    f = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)      # noqa: E731
    o = dict(rois=f(B, R, 7), roi_scores=f(B, R), roi_labels=f(B, R, dt=torch.int32), roi_indices=f(B, R, dt=torch.int32),
             gt_iou_of_rois=f(B, R), gt_of_rois_src=f(B, R, 8), gt_of_rois=f(B, R, 8), reg_valid_mask=f(B, R, dt=torch.int32),
             rcnn_cls_labels=f(B, R))
    if B:
        need = int(L.load().gdmae_roi_targets_workspace_bytes(B, M))
        ws = _WORKSPACE.get(dev)
        if ws is None or ws.numel() < need:
            ws = _WORKSPACE[dev] = torch.empty(int(need * 1.25) + 256, dtype=torch.uint8, device=dev)
        L.call("gdmae_roi_targets", L.ptr(rois), L.ptr(roi_scores), L.ptr(labels), B, M, cols, L.ptr(gt_boxes), G, L.ptr(u_fg), L.ptr(u_bg),
               L.ptr(_QUOTA[qk]), R, P['fg_per_image'], P['reg_fg'], P['cls_fg'], P['cls_bg'], P['cls_bg_lo'], int(P['by_class']),
               1 if P['cls_type'] == 'cls' else 0, *[L.ptr(o[k]) for k in FIELDS], L.ptr(ws), ws.numel(), L.stream())
    for k in ('roi_labels', 'roi_indices', 'reg_valid_mask'):
        o[k] = o[k].long()
    if P['cls_type'] == 'cls':
        o['rcnn_cls_labels'] = o['rcnn_cls_labels'].long()
    return o


def roi_targets(rois, roi_scores, roi_labels, gt_boxes, u_fg, u_bg, P):
    """-> ``targets_dict`` of torch tensors on the inputs' device.  Device tensors: the HIP library; CPU tensors: numpy."""
    if rois.is_cuda:
        return roi_targets_hip(rois, roi_scores, roi_labels, gt_boxes, u_fg, u_bg, P)
    n = lambda t: t.detach().cpu().numpy()      # noqa: E731
    out = roi_targets_numpy(n(rois), n(roi_scores), n(roi_labels), n(gt_boxes), n(u_fg.float()), n(u_bg.float()), P)
    return {k: torch.from_numpy(v) for k, v in out.items()}
