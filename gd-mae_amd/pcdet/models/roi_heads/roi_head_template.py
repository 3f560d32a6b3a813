"""Eval-mode subset of the reference ``RoIHeadTemplate`` (pcdet/models/roi_heads/roi_head_template.py:11-102, 226-254): the box
coder, ``proposal_layer`` for RoIs a first stage already produced, and ``generate_predicted_boxes``.  The proposal target layer
and the rcnn losses (second-stage training) are not built and raise by name."""
import torch
import torch.nn as nn

from ..dense_heads.anchor_head_single import residual_decode, residual_encode


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
