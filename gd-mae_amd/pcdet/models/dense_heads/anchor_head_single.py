"""Anchor-based dense head of the shipped KITTI fine-tune config (tools/cfgs/kitti_models/gd_mae.yaml:191-247).

Parameter names / shapes (``conv_cls``, ``conv_box``, ``conv_dir_cls``: 1 x 1 convolutions), ``init_weights``, the
``forward_ret_dict`` / ``batch_dict`` entries, anchor ordering and every loss definition follow the reference
``AnchorHeadSingle`` / ``AnchorHeadTemplate`` (pcdet/models/dense_heads/anchor_head_single.py:7-75,
anchor_head_template.py:11-266) with ``AxisAlignedTargetAssigner`` (target_assigner/axis_aligned_target_assigner.py:36-210),
``AnchorGenerator`` (target_assigner/anchor_generator.py:17-60) and ``ResidualCoder`` (utils/box_coder_utils.py:14-78).

Two paths:

* the op-by-op torch path (``*_torch`` methods): a restatement of the reference, taken on CPU tensors and when ``fused`` is
  False.  It is the oracle of the fused path and what the golden fixture pins.
* the fused path on CUDA tensors (csrc/anchor_head.hip): the three 1 x 1 convolutions as ONE row product 128 -> 72 on the
  library GEMM (rows of the channels-last BEV map, no layout copy), target assignment for all samples and classes in three
  launches (``gdmae_anchor_targets``; the reference loops in Python over samples x classes with host syncs), the three
  losses in one pass per direction (``gdmae_anchor_loss_fwd`` / ``_bwd``), box decoding in one launch
  (``gdmae_anchor_decode``).  No host synchronisation, launch count independent of the batch size and class count.

Semantics kept from the reference, quirks included: a force-matched anchor (its IoU with some ground truth equals that ground
truth's best IoU) takes label and box of ITS OWN best ground truth, not of the one it tied with; a class value c selects the
class name ``class_names[c - 1]`` (so padding rows inside the kept range, class 0, count for the last class with a zero box).
Where the reference leaves a choice open (argmax ties on the GPU) the lowest ground-truth index wins, as on the CPU."""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from gdmae_hip import dense as gdense
from gdmae_hip import lib as L
from gdmae_hip import ops as gops

_BETA = 1.0 / 9.0          # WeightedSmoothL1Loss default (loss_utils.py:85)
_ALPHA, _GAMMA = 0.25, 2.0  # SigmoidFocalClassificationLoss as built by anchor_head_template.py:73-76


def limit_period(val, offset=0.5, period=math.pi):
    return val - torch.floor(val / period + offset) * period


def nearest_bev_rects(boxes):
    """(N, 7+) -> (N, 4) [x1, y1, x2, y2]: the axis-aligned rectangle nearest to each box (box_utils.py:272-283)."""
    rot = limit_period(boxes[:, 6], 0.5, np.pi).abs()
    dims = torch.where(rot[:, None] < np.pi / 4, boxes[:, [3, 4]], boxes[:, [4, 3]])
    return torch.cat((boxes[:, 0:2] - dims / 2, boxes[:, 0:2] + dims / 2), dim=1)


def rects_iou(a, b):
    """(N, 4), (M, 4) -> (N, M) IoU of axis-aligned rectangles in the operation order of box_utils.py:249-269."""
    x_min = torch.max(a[:, 0, None], b[None, :, 0])
    x_max = torch.min(a[:, 2, None], b[None, :, 2])
    y_min = torch.max(a[:, 1, None], b[None, :, 1])
    y_max = torch.min(a[:, 3, None], b[None, :, 3])
    x_len = torch.clamp_min(x_max - x_min, min=0)
    y_len = torch.clamp_min(y_max - y_min, min=0)
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    inter = x_len * y_len
    return inter / torch.clamp_min(area_a[:, None] + area_b[None, :] - inter, min=1e-6)


def residual_encode(boxes, anchors):
    """ResidualCoder.encode_torch (box_coder_utils.py:14-44), 7 codes, norm=True."""
    anchors = torch.cat([anchors[:, :3], torch.clamp_min(anchors[:, 3:6], 1e-5), anchors[:, 6:]], dim=-1)
    boxes = torch.cat([boxes[:, :3], torch.clamp_min(boxes[:, 3:6], 1e-5), boxes[:, 6:]], dim=-1)
    xa, ya, za, dxa, dya, dza, ra = torch.split(anchors[:, :7], 1, dim=-1)
    xg, yg, zg, dxg, dyg, dzg, rg = torch.split(boxes[:, :7], 1, dim=-1)
    diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
    return torch.cat([(xg - xa) / diagonal, (yg - ya) / diagonal, (zg - za) / dza, torch.log(dxg / dxa), torch.log(dyg / dya),
                      torch.log(dzg / dza), rg - ra], dim=-1)


def residual_decode(enc, anchors):
    """ResidualCoder.decode_torch (box_coder_utils.py:46-78), 7 codes, norm=True."""
    xa, ya, za, dxa, dya, dza, ra = torch.split(anchors, 1, dim=-1)
    xt, yt, zt, dxt, dyt, dzt, rt = torch.split(enc, 1, dim=-1)
    diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
    return torch.cat([xt * diagonal + xa, yt * diagonal + ya, zt * dza + za, torch.exp(dxt) * dxa, torch.exp(dyt) * dya,
                      torch.exp(dzt) * dza, rt + ra], dim=-1)


def generate_anchors(anchor_cfg, grid_size, point_cloud_range):
    """One (nz, ny, nx, n_size, n_rot, 7) fp32 host tensor per anchor class (anchor_generator.py:17-60,
    anchor_head_template.py:37-51), and the number of anchors per location of each."""
    out, per_loc = [], []
    rng = point_cloud_range
    for cfg in anchor_cfg:
        gs = grid_size[:2] // cfg['feature_map_stride']
        sizes, rots, heights = cfg['anchor_sizes'], cfg['anchor_rotations'], cfg['anchor_bottom_heights']
        per_loc.append(len(rots) * len(sizes) * len(heights))
        if cfg.get('align_center', False):
            xs, ys = (rng[3] - rng[0]) / gs[0], (rng[4] - rng[1]) / gs[1]
            xo, yo = xs / 2, ys / 2
        else:
            xs, ys = (rng[3] - rng[0]) / (gs[0] - 1), (rng[4] - rng[1]) / (gs[1] - 1)
            xo, yo = 0, 0
        x = torch.arange(rng[0] + xo, rng[3] + 1e-5, step=xs, dtype=torch.float32)
        y = torch.arange(rng[1] + yo, rng[4] + 1e-5, step=ys, dtype=torch.float32)
        z = x.new_tensor(heights)
        ns, nr = len(sizes), len(rots)
        rot_t, size_t = x.new_tensor(rots), x.new_tensor(sizes)
        x, y, z = torch.meshgrid([x, y, z], indexing='ij')
        a = torch.stack((x, y, z), dim=-1)[:, :, :, None, :].repeat(1, 1, 1, ns, 1)
        a = torch.cat((a, size_t.view(1, 1, 1, -1, 3).repeat([*a.shape[0:3], 1, 1])), dim=-1)
        a = a[:, :, :, :, None, :].repeat(1, 1, 1, 1, nr, 1)
        a = torch.cat((a, rot_t.view(1, 1, 1, 1, -1, 1).repeat([*a.shape[0:3], ns, 1, 1])), dim=-1)
        a = a.permute(2, 1, 0, 3, 4, 5).contiguous()
        a[..., 2] += a[..., 5] / 2                    # bottom height -> box centre
        out.append(a)
    return out, per_loc


class AnchorLossFn(torch.autograd.Function):
    """(cls, loc, dir) losses of anchor_head_template.py:100-222 from the head's (n_sites, n_cols) output rows in one launch per
    direction (+ a fixed-order finish): csrc/anchor_head.hip gdmae_anchor_loss_fwd / _bwd.  -> (3,) fp32 on the device."""

    @staticmethod
    def forward(ctx, rows, labels, reg_t, dir_t, npos, meta):
        B, n_loc, K, C, nb, cw, scales = meta
        assert rows.is_cuda and rows.dtype in (torch.bfloat16, torch.float32) and rows.is_contiguous()
        dev = rows.device
        part = torch.empty(L.load().gdmae_anchor_loss_rows() * 3, dtype=torch.float32, device=dev)
        out = torch.empty(4, dtype=torch.float32, device=dev)
        args = (L.ptr(rows), int(rows.dtype == torch.bfloat16), rows.shape[1], B, n_loc, K, C, nb, L.ptr(labels), L.ptr(reg_t), L.ptr(dir_t),
                L.ptr(npos), L.host_f32(cw), L.host_f32(scales))
        L.call("gdmae_anchor_loss_fwd", *args, L.ptr(part), L.ptr(out), L.stream())
        ctx.save_for_backward(rows, labels, reg_t, dir_t, npos)
        ctx.meta = meta
        return out[:3]

    @staticmethod
    def backward(ctx, g):
        rows, labels, reg_t, dir_t, npos = ctx.saved_tensors
        B, n_loc, K, C, nb, cw, scales = ctx.meta
        d = torch.empty_like(rows)
        gs = g.float().contiguous()
        L.call("gdmae_anchor_loss_bwd", L.ptr(rows), int(rows.dtype == torch.bfloat16), rows.shape[1], B, n_loc, K, C, nb, L.ptr(labels),
               L.ptr(reg_t), L.ptr(dir_t), L.ptr(npos), L.host_f32(cw), L.host_f32(scales), L.ptr(gs), L.ptr(d), L.stream())
        return d, None, None, None, None, None


class AnchorHeadSingle(nn.Module):
    fused = True             # False: the op-by-op torch path on CUDA tensors too (the tests' oracle on the device)

    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range,
                 predict_boxes_when_training=True, **kwargs):
        super().__init__()
        self.model_cfg, self.num_class, self.class_names = model_cfg, num_class, list(class_names)
        self.predict_boxes_when_training = predict_boxes_when_training
        tcfg = model_cfg.TARGET_ASSIGNER_CONFIG
        if model_cfg.get('USE_MULTIHEAD', False):
            raise NotImplementedError("USE_MULTIHEAD: multi-head anchor heads are outside this path")
        if tcfg.NAME != 'AxisAlignedTargetAssigner':
            raise NotImplementedError(f"TARGET_ASSIGNER_CONFIG.NAME {tcfg.NAME}: only AxisAlignedTargetAssigner is built (ATSS is not)")
        if tcfg.POS_FRACTION >= 0:
            raise NotImplementedError("POS_FRACTION >= 0 (random sampling of anchors) is not built; the shipped config uses -1")
        if tcfg.get('MATCH_HEIGHT', False):
            raise NotImplementedError("MATCH_HEIGHT: True (3-D IoU matching) is not built")
        if tcfg.get('NORM_BY_NUM_EXAMPLES', False):
            raise NotImplementedError("NORM_BY_NUM_EXAMPLES: True is not built")
        if tcfg.BOX_CODER != 'ResidualCoder' or tcfg.get('BOX_CODER_CONFIG', None):
            raise NotImplementedError("BOX_CODER: only ResidualCoder with its default arguments is built")
        if model_cfg.LOSS_CONFIG.get('REG_LOSS_TYPE', None) is not None:
            raise NotImplementedError("REG_LOSS_TYPE: only the default WeightedSmoothL1Loss is built")
        self.code_size = 7
        acfg = model_cfg.ANCHOR_GENERATOR_CONFIG
        grid_size = np.asarray(grid_size)
        anchors, per_loc = generate_anchors(acfg, grid_size, point_cloud_range)
        self.anchor_class_names = [c['class_name'] for c in acfg]
        self.matched_thresholds = [float(c['matched_threshold']) for c in acfg]
        self.unmatched_thresholds = [float(c['unmatched_threshold']) for c in acfg]
        self.num_anchors_per_location = sum(per_loc)
        self._per_loc = per_loc
        for i, a in enumerate(anchors):            # non-persistent: they move with the module, and stay out of the state dict
            self.register_buffer('anchors_%d' % i, a, persistent=False)
        self._n_anchor_sets = len(anchors)
        K = self.num_anchors_per_location
        self.conv_cls = nn.Conv2d(input_channels, K * num_class, kernel_size=1)
        self.conv_box = nn.Conv2d(input_channels, K * self.code_size, kernel_size=1)
        self.conv_dir_cls = None
        if model_cfg.get('USE_DIRECTION_CLASSIFIER', None) is not None:
            self.conv_dir_cls = nn.Conv2d(input_channels, K * model_cfg.NUM_DIR_BINS, kernel_size=1)
        self.forward_ret_dict = {}
        self._tables = {}
        self.init_weights()

    def init_weights(self):
        pi = 0.01
        nn.init.constant_(self.conv_cls.bias, -np.log((1 - pi) / pi))
        nn.init.normal_(self.conv_box.weight, mean=0, std=0.001)

    @property
    def anchors(self):
        return [getattr(self, 'anchors_%d' % i) for i in range(self._n_anchor_sets)]

    def all_anchors(self):
        """(n_anchors, 7) in the head's output order: per location class-major, then size, then rotation."""
        a = torch.cat(self.anchors, dim=-3)
        return a.view(-1, a.shape[-1])

    # ------------------------------------------------------------------------------------------------ torch path
    def assign_targets_torch(self, gt_boxes_with_classes):
        """AxisAlignedTargetAssigner.assign_targets op by op.  -> dict(box_cls_labels (B, A) int32, box_reg_targets (B, A, 7),
        reg_weights (B, A), gt_ids (B, A) int32: row of gt_boxes[b] an anchor is matched with or -1)."""
        B = gt_boxes_with_classes.shape[0]
        gt_classes, gt_boxes = gt_boxes_with_classes[:, :, -1], gt_boxes_with_classes[:, :, :-1]
        names = np.array(self.class_names)
        out = {'box_cls_labels': [], 'box_reg_targets': [], 'reg_weights': [], 'gt_ids': []}
        for k in range(B):
            cur = gt_boxes[k]
            cnt = len(cur) - 1
            while cnt > 0 and cur[cnt].sum() == 0:
                cnt -= 1
            cur = cur[:cnt + 1]
            cur_cls = gt_classes[k][:cnt + 1].int()
            rows = torch.arange(cnt + 1, device=cur.device)
            per_class = []
            for name, anchors, mt, ut in zip(self.anchor_class_names, self.anchors, self.matched_thresholds, self.unmatched_thresholds):
                mask = torch.from_numpy(names[cur_cls.cpu().numpy() - 1] == name).to(cur.device)
                fms = anchors.shape[:3]
                lab, tgt, w, gid = self._assign_single_torch(anchors.view(-1, anchors.shape[-1]), cur[mask], cur_cls[mask], rows[mask], mt, ut)
                per_class.append((lab.view(*fms, -1), tgt.view(*fms, -1, self.code_size), w.view(*fms, -1), gid.view(*fms, -1)))
            out['box_cls_labels'].append(torch.cat([p[0] for p in per_class], dim=-1).view(-1))
            out['box_reg_targets'].append(torch.cat([p[1] for p in per_class], dim=-2).view(-1, self.code_size))
            out['reg_weights'].append(torch.cat([p[2] for p in per_class], dim=-1).view(-1))
            out['gt_ids'].append(torch.cat([p[3] for p in per_class], dim=-1).view(-1))
        return {k: torch.stack(v, dim=0) for k, v in out.items()}

    def _assign_single_torch(self, anchors, gt, gt_cls, gt_rows, matched_threshold, unmatched_threshold):
        n, m = anchors.shape[0], gt.shape[0]
        dev = anchors.device
        labels = torch.ones((n,), dtype=torch.int32, device=dev) * -1
        gt_ids = torch.ones((n,), dtype=torch.int32, device=dev) * -1
        if m > 0 and n > 0:
            iou = rects_iou(nearest_bev_rects(anchors[:, 0:7]), nearest_bev_rects(gt[:, 0:7]))
            a2g_arg = iou.argmax(dim=1)
            a2g_max = iou[torch.arange(n, device=dev), a2g_arg]
            g2a_arg = iou.argmax(dim=0)
            g2a_max = iou[g2a_arg, torch.arange(m, device=dev)]
            g2a_max[g2a_max == 0] = -1
            forced = (iou == g2a_max).nonzero()[:, 0]
            force_gt = a2g_arg[forced]
            labels[forced] = gt_cls[force_gt]
            gt_ids[forced] = force_gt.int()
            pos = a2g_max >= matched_threshold
            over = a2g_arg[pos]
            labels[pos] = gt_cls[over]
            gt_ids[pos] = over.int()
            bg = (a2g_max < unmatched_threshold).nonzero()[:, 0]
        fg = (labels > 0).nonzero()[:, 0]
        if m == 0 or n == 0:
            labels[:] = 0
        else:
            labels[bg] = 0
            labels[forced] = gt_cls[force_gt]
        targets = anchors.new_zeros((n, self.code_size))
        rows_out = torch.ones((n,), dtype=torch.int32, device=dev) * -1
        if m > 0 and n > 0:
            targets[fg, :] = residual_encode(gt[a2g_arg[fg], :], anchors[fg, :])
            rows_out[fg] = gt_rows[a2g_arg[fg]].int()
        w = anchors.new_zeros((n,))
        w[labels > 0] = 1.0
        return labels, targets, w, rows_out

    def direction_bins_torch(self, reg_targets):
        """get_direction_target without the one-hot (anchor_head_template.py:144-151): (B, A) int64."""
        cfg = self.model_cfg
        rot_gt = reg_targets[..., 6] + self.all_anchors()[None, :, 6]
        off = limit_period(rot_gt - cfg.DIR_OFFSET, 0, 2 * np.pi)
        return torch.clamp(torch.floor(off / (2 * np.pi / cfg.NUM_DIR_BINS)).long(), min=0, max=cfg.NUM_DIR_BINS - 1)

    def get_loss_torch(self):
        """(cls, loc, dir) losses, each already / batch size and x its LOSS_WEIGHTS entry (anchor_head_template.py:100-213)."""
        fr, cfg = self.forward_ret_dict, self.model_cfg
        w = cfg.LOSS_CONFIG.LOSS_WEIGHTS
        cls_preds, labels = fr['cls_preds'].float(), fr['box_cls_labels']
        B = int(cls_preds.shape[0])
        cared, positives, negatives = labels >= 0, labels > 0, labels == 0
        cls_weights = (negatives * 1.0 + 1.0 * positives).float()
        if self.num_class == 1:
            labels = torch.where(positives, torch.ones_like(labels), labels)
        pos_norm = positives.sum(1, keepdim=True).float()
        cls_weights = cls_weights / torch.clamp(pos_norm, min=1.0)
        cls_targets = labels * cared.type_as(labels)
        one_hot = torch.zeros(*cls_targets.shape, self.num_class + 1, dtype=cls_preds.dtype, device=cls_preds.device)
        one_hot.scatter_(-1, cls_targets.unsqueeze(-1).long(), 1.0)
        x, t = cls_preds.view(B, -1, self.num_class), one_hot[..., 1:]
        p = torch.sigmoid(x)
        alpha_w = t * _ALPHA + (1 - t) * (1 - _ALPHA)
        pt = t * (1.0 - p) + (1.0 - t) * p
        bce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-torch.abs(x)))
        cls_loss = (alpha_w * torch.pow(pt, _GAMMA) * bce * cls_weights.unsqueeze(-1)).sum() / B * w['cls_weight']

        box_preds, targets = fr['box_preds'].float(), fr['box_reg_targets']
        reg_weights = positives.float() / torch.clamp(pos_norm, min=1.0)
        bp = box_preds.view(B, -1, box_preds.shape[-1] // self.num_anchors_per_location)
        ps = torch.sin(bp[..., 6:7]) * torch.cos(targets[..., 6:7])            # sin(a - b) = sin a cos b - cos a sin b
        ts = torch.cos(bp[..., 6:7]) * torch.sin(targets[..., 6:7])
        bp_s, tg_s = torch.cat([bp[..., :6], ps], dim=-1), torch.cat([targets[..., :6], ts], dim=-1)
        tg_s = torch.where(torch.isnan(tg_s), bp_s, tg_s)
        diff = (bp_s - tg_s) * bp_s.new_tensor(np.array(w['code_weights'], dtype=np.float32))
        n = torch.abs(diff)
        sl1 = torch.where(n < _BETA, 0.5 * n ** 2 / _BETA, n - 0.5 * _BETA)
        loc_loss = (sl1 * reg_weights.unsqueeze(-1)).sum() / B * w['loc_weight']

        dir_loss = None
        if fr.get('dir_cls_preds', None) is not None:
            bins = self.direction_bins_torch(targets)
            logits = fr['dir_cls_preds'].float().view(B, -1, cfg.NUM_DIR_BINS)
            dw = positives.type_as(logits)
            dw = dw / torch.clamp(dw.sum(-1, keepdim=True), min=1.0)
            dir_loss = (F.cross_entropy(logits.permute(0, 2, 1), bins, reduction='none') * dw).sum() / B * w['dir_weight']
        return cls_loss, loc_loss, dir_loss

    def generate_predicted_boxes_torch(self, batch_size, cls_preds, box_preds, dir_cls_preds=None):
        cfg = self.model_cfg
        anchors = self.all_anchors()
        A = anchors.shape[0]
        batch_anchors = anchors.view(1, A, 7).repeat(batch_size, 1, 1)
        batch_cls = cls_preds.view(batch_size, A, -1).float()
        boxes = residual_decode(box_preds.float().view(batch_size, A, -1), batch_anchors)
        if dir_cls_preds is not None:
            labels = torch.max(dir_cls_preds.float().view(batch_size, A, -1), dim=-1)[1]
            period = 2 * np.pi / cfg.NUM_DIR_BINS
            rot = limit_period(boxes[..., 6] - cfg.DIR_OFFSET, cfg.DIR_LIMIT_OFFSET, period)
            boxes = torch.cat([boxes[..., :6], (rot + cfg.DIR_OFFSET + period * labels.to(boxes.dtype)).unsqueeze(-1)], dim=-1)
        return batch_cls, boxes

    def _forward_torch(self, data_dict):
        x = data_dict['spatial_features_2d']
        x = x.float() if x.dtype != self.conv_cls.weight.dtype else x
        fr = self.forward_ret_dict
        fr['cls_preds'] = self.conv_cls(x).permute(0, 2, 3, 1).contiguous()
        fr['box_preds'] = self.conv_box(x).permute(0, 2, 3, 1).contiguous()
        fr['dir_cls_preds'] = self.conv_dir_cls(x).permute(0, 2, 3, 1).contiguous() if self.conv_dir_cls is not None else None
        if self.training:
            fr.update(self.assign_targets_torch(data_dict['gt_boxes']))
        if not self.training or self.predict_boxes_when_training:
            data_dict['batch_cls_preds'], data_dict['batch_box_preds'] = self.generate_predicted_boxes_torch(
                data_dict['batch_size'], fr['cls_preds'], fr['box_preds'], fr['dir_cls_preds'])
            data_dict['cls_preds_normalized'] = False
        return data_dict

    # ------------------------------------------------------------------------------------------------ fused path (HIP)
    def _device_tables(self, dev):
        """Small per-device tables the kernels read anchor geometry from - filled from the generated anchor tensors, so the values are
        the torch path's bits: rectangle edges per (anchor slot, column) / (anchor slot, row), centres, and per-slot z / size / rotation."""
        key = (dev.type, dev.index)
        if key in self._tables:
            return self._tables[key]
        sets = [a.cpu() for a in self.anchors]
        if any(a.shape[0] != 1 for a in sets) or len({tuple(a.shape[1:3]) for a in sets}) != 1:
            raise NotImplementedError("anchor sets with several bottom heights or different feature-map strides")
        H, W = sets[0].shape[1:3]
        a = torch.cat(sets, dim=-3)[0].reshape(H, W, -1, 7)             # (H, W, K, 7)
        K = a.shape[2]
        rect = nearest_bev_rects(a.reshape(-1, 7)).view(H, W, K, 4)
        xr = rect[0][:, :, [0, 2]].permute(1, 0, 2).contiguous()          # (K, W, 2): x1, x2
        yr = rect[:, 0][:, :, [1, 3]].permute(1, 0, 2).contiguous()          # (K, H, 2): y1, y2
        assert torch.equal(rect[..., [0, 2]], xr.permute(1, 0, 2)[None].expand(H, W, K, 2))
        assert torch.equal(rect[..., [1, 3]], yr.permute(1, 0, 2)[:, None].expand(H, W, K, 2))
        slot_cls = [ci for ci, n in enumerate(self._per_loc) for _ in range(n)]
        t = {'H': H, 'W': W, 'K': K,
             'xr': xr.to(dev), 'yr': yr.to(dev), 'xc': a[0, :, 0, 0].contiguous().to(dev), 'yc': a[:, 0, 0, 1].contiguous().to(dev),
             'slot': a[0, 0, :, 2:7].contiguous().to(dev),               # (K, 5): z, dx, dy, dz, rotation
             'slot_cls': torch.tensor(slot_cls, dtype=torch.int32, device=dev),
             'name_idx': [self.class_names.index(n) if n in self.class_names else -1 for n in self.anchor_class_names]}
        self._tables[key] = t
        return t

    def assign_targets_hip(self, gt_boxes):
        """gt_boxes (B, n_max, 8) on the device -> box_cls_labels (B, A) int32, gt_ids (B, A) int32, box_reg_targets (B, A, 7) fp32,
        dir_bins (B, A) int32 (-1 where no box is regressed), num_pos (B) int32.  Three launches, no host transfer."""
        gt = gt_boxes.float().contiguous()
        assert gt.is_cuda, "AnchorHeadSingle.assign_targets_hip runs in libgdmae_hip.so"
        B, n_max, box_dim = gt.shape
        dev, cfg = gt.device, self.model_cfg
        t = self._device_tables(dev)
        H, W, K = t['H'], t['W'], t['K']
        A = H * W * K
        n_cls = len(self.anchor_class_names)
        labels = torch.empty(B, A, dtype=torch.int32, device=dev)
        gt_ids = torch.empty(B, A, dtype=torch.int32, device=dev)
        reg = torch.empty(B, A, 7, dtype=torch.float32, device=dev)
        bins = torch.empty(B, A, dtype=torch.int32, device=dev)
        npos = torch.empty(B, dtype=torch.int32, device=dev)
        ws = torch.empty(L.load().gdmae_anchor_targets_workspace_bytes(B, n_cls, n_max), dtype=torch.uint8, device=dev)
        L.call("gdmae_anchor_targets", L.ptr(gt), B, n_max, box_dim, H, W, K, n_cls, len(self.class_names), L.host_i32(t['name_idx']),
               L.ptr(t['slot_cls']), L.ptr(t['xr']), L.ptr(t['yr']), L.ptr(t['xc']), L.ptr(t['yc']), L.ptr(t['slot']),
               L.host_f32(self.matched_thresholds), L.host_f32(self.unmatched_thresholds), float(cfg.get('DIR_OFFSET', 0.0)),
               int(cfg.get('NUM_DIR_BINS', 2)), L.ptr(labels), L.ptr(gt_ids), L.ptr(reg), L.ptr(bins), L.ptr(npos), L.ptr(ws), L.stream())
        return {'box_cls_labels': labels, 'gt_ids': gt_ids, 'box_reg_targets': reg, 'dir_bins': bins, 'num_pos': npos}

    def _packed_weights(self):
        convs = [self.conv_cls, self.conv_box] + ([self.conv_dir_cls] if self.conv_dir_cls is not None else [])
        w = torch.cat([c.weight.view(c.out_channels, -1) for c in convs], dim=0)
        b = torch.cat([c.bias for c in convs], dim=0)
        pad = (-w.shape[0]) % 8                                  # the library GEMM takes widths in multiples of 8
        if pad:
            w, b = torch.cat([w, w.new_zeros(pad, w.shape[1])]), torch.cat([b, b.new_zeros(pad)])
        return w, b

    def _forward_hip(self, data_dict):
        x = data_dict['spatial_features_2d']
        B, Cin, H, W = x.shape
        cfg, fr = self.model_cfg, self.forward_ret_dict
        K, C = self.num_anchors_per_location, self.num_class
        nb = cfg.NUM_DIR_BINS if self.conv_dir_cls is not None else 0
        if self.conv_dir_cls is None:
            raise NotImplementedError("the fused anchor head needs USE_DIRECTION_CLASSIFIER (the shipped config)")
        w, b = self._packed_weights()
        if not x.is_contiguous(memory_format=torch.channels_last):       # SSTBEVBackbone's row kernels leave channels-last maps; anything
            x = x.contiguous(memory_format=torch.channels_last)          # else is moved once, explicitly
        rows = x.permute(0, 2, 3, 1).view(B * H * W, Cin)                # the map's own storage as (sites, channels) rows
        if not torch.is_autocast_enabled():
            rows = rows.float()
        y = gops.linear(rows, w, b)                                      # (B H W, 72): [cls K*C | box K*7 | dir K*nb]
        n_cls, n_box = K * C, K * 7
        fr['rows'] = y
        fr['cls_preds'] = y[:, :n_cls].view(B, H, W, n_cls)
        fr['box_preds'] = y[:, n_cls:n_cls + n_box].view(B, H, W, n_box)
        fr['dir_cls_preds'] = y[:, n_cls + n_box:n_cls + n_box + K * nb].view(B, H, W, K * nb)
        if self.training:
            fr.update(self.assign_targets_hip(data_dict['gt_boxes']))
        if not self.training or self.predict_boxes_when_training:
            t = self._device_tables(x.device)
            A = H * W * K
            yd = y.detach()
            cls_out = torch.empty(B, A, C, dtype=torch.float32, device=x.device)
            boxes = torch.empty(B, A, 7, dtype=torch.float32, device=x.device)
            L.call("gdmae_anchor_decode", L.ptr(yd), int(yd.dtype == torch.bfloat16), yd.shape[1], B, H, W, K, C, nb, L.ptr(t['xc']),
                   L.ptr(t['yc']), L.ptr(t['slot']), float(cfg.DIR_OFFSET), float(cfg.DIR_LIMIT_OFFSET), L.ptr(cls_out), L.ptr(boxes),
                   L.stream())
            data_dict['batch_cls_preds'], data_dict['batch_box_preds'] = cls_out, boxes
            data_dict['cls_preds_normalized'] = False
        return data_dict

    def _get_loss_hip(self):
        fr, cfg = self.forward_ret_dict, self.model_cfg
        w = cfg.LOSS_CONFIG.LOSS_WEIGHTS
        y = fr['rows']
        B = fr['box_cls_labels'].shape[0]
        K = self.num_anchors_per_location
        meta = (B, y.shape[0] // B, K, self.num_class, int(cfg.NUM_DIR_BINS), [float(v) for v in w['code_weights']],
                [float(w['cls_weight']) / B, float(w['loc_weight']) / B, float(w['dir_weight']) / B])
        out = AnchorLossFn.apply(y, fr['box_cls_labels'], fr['box_reg_targets'], fr['dir_bins'], fr['num_pos'], meta)
        return out[0], out[1], out[2]

    # ------------------------------------------------------------------------------------------------ module interface
    def _use_hip(self, x):
        return bool(self.fused and gdense.FUSE_SHORTCUT and x.is_cuda)

    def forward(self, data_dict):
        self.forward_ret_dict = {}
        if self._use_hip(data_dict['spatial_features_2d']):
            return self._forward_hip(data_dict)
        return self._forward_torch(data_dict)

    def get_loss(self, tb_dict=None):
        """-> (rpn_loss, tb_dict) with rpn_loss_cls / rpn_loss_loc / rpn_loss_dir as device scalars (the detector reads them once,
        and only when its ``sync_loss_scalar`` is set; the reference calls .item() three times here)."""
        tb_dict = {} if tb_dict is None else tb_dict
        cls_loss, loc_loss, dir_loss = self._get_loss_hip() if 'rows' in self.forward_ret_dict else self.get_loss_torch()
        tb_dict.update({'rpn_loss_cls': cls_loss.detach(), 'rpn_loss_loc': loc_loss.detach()})
        box_loss = loc_loss
        if dir_loss is not None:
            tb_dict['rpn_loss_dir'] = dir_loss.detach()
            box_loss = box_loss + dir_loss
        return cls_loss + box_loss, tb_dict
