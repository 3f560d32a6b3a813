"""The reference ``RoIHeadTemplate`` (pcdet/models/roi_heads/roi_head_template.py:11-254): the box coder, ``proposal_layer`` for
RoIs a first stage already produced, ``generate_predicted_boxes``, and for second-stage training ``proposal_targets`` (the proposal
target layer and the canonical transformation of ``assign_targets`` for the whole batch, ``proposal_targets.py``) and
``rcnn_losses`` (``get_box_cls_layer_loss`` / ``get_box_reg_layer_loss`` op by op in torch).  The reference's own entry points
``assign_targets`` / ``get_loss`` draw random numbers between host reads and keep raising by name: training goes through
``gdmae_hip.two_stage.SecondStageTrainer``."""
import numpy as np
import torch
import torch.nn as nn
from torch.nn import functional as F

from ..dense_heads.anchor_head_single import residual_decode, residual_encode
from . import proposal_targets as pt

_BETA = 1.0 / 9.0          # WeightedSmoothL1Loss default (loss_utils.py:85)


class ResidualCoder:
    """ResidualCoder with its default arguments and ``norm=True`` (utils/box_coder_utils.py:5-78): the anchor head's coder."""
    code_size = 7

    def __init__(self, code_size=7, encode_angle_by_sincos=False, norm=True, **kwargs):
        if code_size != 7 or encode_angle_by_sincos or not norm or kwargs:
            raise NotImplementedError("BOX_CODER_CONFIG: only ResidualCoder(code_size=7, norm=True) is built")

    @staticmethod
    def encode_torch(boxes, anchors):
        return residual_encode(boxes, anchors)

    @staticmethod
    def decode_torch(box_encodings, anchors):
        return residual_decode(box_encodings, anchors)


def rotate_points_along_z(points, angle):
    """points (B, N, 3 + C), angle (B) -> rotated about z, angle increasing x ==> y (utils/common_utils.py:99-121)."""
    cosa, sina = torch.cos(angle), torch.sin(angle)
    zeros, ones = angle.new_zeros(points.shape[0]), angle.new_ones(points.shape[0])
    rot = torch.stack((cosa, sina, zeros, -sina, cosa, zeros, zeros, zeros, ones), dim=1).view(-1, 3, 3).float()
    return torch.cat((torch.matmul(points[:, :, 0:3], rot), points[:, :, 3:]), dim=-1)


def smooth_l1(diff, beta):
    """WeightedSmoothL1Loss.smooth_l1_loss (loss_utils.py:101-109)."""
    n = torch.abs(diff)
    return n if beta < 1e-5 else torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)


def boxes_to_corners_3d(boxes3d):
    """(N, 7) -> (N, 8, 3) corners in the reference's order (utils/box_utils.py:28-53)."""
    template = boxes3d.new_tensor(([1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1],
                                   [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1])) / 2
    corners3d = boxes3d[:, None, 3:6].repeat(1, 8, 1) * template[None, :, :]
    corners3d = rotate_points_along_z(corners3d.view(-1, 8, 3), boxes3d[:, 6]).view(-1, 8, 3)
    return corners3d + boxes3d[:, None, 0:3]


def corner_loss_lidar(pred_bbox3d, gt_bbox3d):
    """get_corner_loss_lidar with p = 2 (loss_utils.py:241-270): (N, 7), (N, 7) -> (N)."""
    pred = boxes_to_corners_3d(pred_bbox3d)
    gt = boxes_to_corners_3d(gt_bbox3d)
    flip = gt_bbox3d.clone()
    flip[:, 6] += np.pi
    gt_flip = boxes_to_corners_3d(flip)
    dist = torch.min(torch.norm(pred - gt, dim=2), torch.norm(pred - gt_flip, dim=2))
    return smooth_l1(dist, beta=1.0).mean(dim=1)


class RoIHeadTemplate(nn.Module):
    def __init__(self, num_class, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        tcfg = self.model_cfg.TARGET_CONFIG
        if tcfg.BOX_CODER != 'ResidualCoder':
            raise NotImplementedError(f"BOX_CODER {tcfg.BOX_CODER}: only ResidualCoder is built")
        self.box_coder = ResidualCoder(**tcfg.get('BOX_CODER_CONFIG', {}))
        self.forward_ret_dict = None

    @torch.no_grad()
    def proposal_layer(self, batch_dict, nms_config):
        """RoIs of a first stage that predicts boxes itself (CenterHead with ``predict_boxes_when_training``) pass through
        (roi_head_template.py:64-65); selecting RoIs from ``batch_cls_preds`` by NMS here is not built."""
        if batch_dict.get('rois', None) is not None:
            return batch_dict
        raise NotImplementedError("proposal_layer: RoI selection by NMS (no 'rois' in batch_dict) is not built")

    def assign_targets(self, batch_dict):
        raise NotImplementedError("second-stage training (ProposalTargetLayer / assign_targets) is not built")

    def get_loss(self, tb_dict=None):
        raise NotImplementedError("second-stage training (rcnn losses / get_loss) is not built")

    @torch.no_grad()
    def proposal_targets(self, batch_dict, u_fg, u_bg):
        """``targets_dict`` of the reference's ``assign_targets`` (with ``roi_indices`` and ``gt_of_rois_src``) for the RoIs, labels,
        scores and ``gt_boxes (B, G, 8)`` of ``batch_dict``; ``u_fg (B, M)`` / ``u_bg (B, ROI_PER_IMAGE)`` uniform numbers in [0, 1)
        that decide the sampling.  Device tensors: ``gdmae_roi_targets``, no host read; CPU tensors: the numpy statement."""
        P = pt.sampler_params(self.model_cfg.TARGET_CONFIG)
        return pt.roi_targets(batch_dict['rois'], batch_dict['roi_scores'], batch_dict['roi_labels'], batch_dict['gt_boxes'], u_fg, u_bg, P)

    def rcnn_losses(self, ret):
        """(rcnn_loss, tb_dict) from a ``forward_ret_dict``: ``get_box_cls_layer_loss`` + ``get_box_reg_layer_loss``
        (roi_head_template.py:129-224).  Shapes stay fixed: where the reference gathers the fg rows by a boolean mask (and reads
        their count on the host) the rows are masked instead, which sums the same terms; without a fg row the regression and the
        corner loss are 0.  ``tb_dict`` holds floats, fetched in one read at the end."""
        cfg = self.model_cfg.LOSS_CONFIG
        w = cfg.LOSS_WEIGHTS
        code_size = self.box_coder.code_size
        rcnn_cls, rcnn_reg = ret['rcnn_cls'], ret['rcnn_reg']
        labels = ret['rcnn_cls_labels'].view(-1)
        if cfg.CLS_LOSS == 'BinaryCrossEntropy':
            batch_loss_cls = F.binary_cross_entropy(torch.sigmoid(rcnn_cls.view(-1)), labels.float(), reduction='none')
        elif cfg.CLS_LOSS == 'CrossEntropy':
            batch_loss_cls = F.cross_entropy(rcnn_cls, labels.long(), reduction='none', ignore_index=-1)
        else:
            raise NotImplementedError(f"LOSS_CONFIG.CLS_LOSS {cfg.CLS_LOSS}: only BinaryCrossEntropy and CrossEntropy are built")
        cls_valid = (labels >= 0).float()
        loss_cls = (batch_loss_cls * cls_valid).sum() / torch.clamp(cls_valid.sum(), min=1.0) * w['rcnn_cls_weight']

        if cfg.REG_LOSS != 'WeightedSmoothL1Loss':
            raise NotImplementedError(f"LOSS_CONFIG.REG_LOSS {cfg.REG_LOSS}: only WeightedSmoothL1Loss is built")
        fg = ret['reg_valid_mask'].view(-1) > 0
        fg_sum = torch.clamp(fg.sum(), min=1).float()
        gt_ct = ret['gt_of_rois'][..., 0:code_size].reshape(-1, code_size)
        gt_src = ret['gt_of_rois_src'][..., 0:code_size].reshape(-1, code_size)
        rois = ret['rois'].detach().reshape(-1, code_size)
        n = gt_ct.shape[0]
        anchor = rois.clone()
        anchor[:, 0:3] = 0
        anchor[:, 6] = 0
        target = self.box_coder.encode_torch(gt_ct, anchor)
        pred = rcnn_reg.view(n, -1)
        target = torch.where(torch.isnan(target), pred, target)
        diff = (pred - target) * pred.new_tensor(np.asarray(w['code_weights'], dtype=np.float32))
        loss_reg = (smooth_l1(diff, _BETA) * fg.unsqueeze(-1).float()).sum() / fg_sum * w['rcnn_reg_weight']
        loss_corner = loss_reg.new_zeros(())
        if cfg.CORNER_LOSS_REGULARIZATION:
            fg_reg = torch.where(fg.unsqueeze(-1), pred, torch.zeros_like(pred))         # rows outside the mean stay finite
            local = rois.clone()
            local[:, 0:3] = 0
            boxes = self.box_coder.decode_torch(fg_reg, local)
            boxes = rotate_points_along_z(boxes.unsqueeze(dim=1), rois[:, 6]).squeeze(dim=1)
            boxes = torch.cat((boxes[:, 0:3] + rois[:, 0:3], boxes[:, 3:]), dim=-1)
            per_roi = corner_loss_lidar(boxes[:, 0:7], gt_src[:, 0:7])
            loss_corner = (per_roi * fg.float()).sum() / fg_sum * w['rcnn_corner_weight']
        loss = loss_cls + loss_reg + loss_corner
        vals = torch.stack((loss_cls, loss_reg, loss_corner, loss)).detach().tolist()
        return loss, dict(zip(('rcnn_loss_cls', 'rcnn_loss_reg', 'rcnn_loss_corner', 'rcnn_loss'), vals))

    def generate_predicted_boxes(self, batch_size, rois, cls_preds, box_preds):
        """rois (B, N, 7), cls_preds (B N, num_class), box_preds (B N, 7) -> batch_cls_preds (B, N, num_class),
        batch_box_preds (B, N, 7): residuals decoded in the RoI's canonical frame, rotated back and shifted."""
        code_size = self.box_coder.code_size
        batch_cls_preds = cls_preds.view(batch_size, -1, cls_preds.shape[-1])
        batch_box_preds = box_preds.view(batch_size, -1, code_size)
        roi_ry = rois[:, :, 6].view(-1)
        roi_xyz = rois[:, :, 0:3].view(-1, 3)
        local_rois = rois[:, :, :code_size].clone().detach()
        local_rois[:, :, 0:3] = 0
        batch_box_preds = self.box_coder.decode_torch(batch_box_preds, local_rois).view(-1, code_size)
        batch_box_preds = rotate_points_along_z(batch_box_preds.unsqueeze(dim=1), roi_ry).squeeze(dim=1)
        batch_box_preds[:, 0:3] += roi_xyz
        return batch_cls_preds, batch_box_preds.view(batch_size, -1, code_size)
