"""``GraphRCNNHead`` in eval mode (reference pcdet/models/roi_heads/graphrcnn_head.py:12-302) with the reference's module and
``state_dict`` names, so that a reference-trained ``gd_mae_ts`` checkpoint loads by key + shape.

RoI point pooling runs through ``pcdet.ops.patch_ops`` (device tensors: the HIP kernels of csrc/roi_pool.hip in one call for
the whole batch; CPU tensors: the numpy statement of the same contract).  The graph network, the shared layer and the two
heads are plain torch modules in fp32 - the exact mode, as for the other detectors.

Training runs through ``forward_train`` (proposal targets from ``gdmae_roi_targets``, then the same pooling, graph network and
heads with autograd), driven by ``gdmae_hip.two_stage.SecondStageTrainer``; ``forward`` in training mode keeps raising.

Not built, raised by name: ``IMG_CONFIG`` (the image branch), ``USE_FEATS_DIS: True`` and a non-None ``NMS_CONFIG.TEST`` /
``NMS_CONFIG.TRAIN`` (RoI selection inside the head)."""
import numpy as np
import torch
import torch.nn as nn
from torch.nn import functional as F

from ...ops.patch_ops import patch_ops_utils
from ..model_utils import network_utils
from .roi_head_template import RoIHeadTemplate


def _is_none(v):
    return v is None or v == 'None'          # the shipped yaml spells the empty NMS sections as the string None


class ShortcutLayer(nn.Module):
    def __init__(self, input_channels, hidden_channels=256, dropout=0.1):
        super().__init__()
        self.conv1 = nn.Conv1d(input_channels, hidden_channels, kernel_size=1)
        self.conv2 = nn.Conv1d(hidden_channels, input_channels, kernel_size=1)
        self.norm1 = nn.BatchNorm1d(input_channels)
        self.norm2 = nn.BatchNorm1d(input_channels)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.dropout3 = nn.Dropout(dropout)
        self.activation = F.relu

    def forward(self, x):
        """(B, C, N) -> (B, C, N)"""
        x = x + self.dropout1(x)
        x = self.norm1(x)
        x2 = self.conv2(self.dropout2(self.activation(self.conv1(x))))
        x = x + self.dropout3(x2)
        return self.norm2(x)


class AttnGNNLayer(nn.Module):
    def __init__(self, input_channels, model_cfg):
        super().__init__()
        self.model_cfg = model_cfg
        self.out_channel = model_cfg.OUT_DIM
        mlps = model_cfg.MLPS
        if model_cfg.USE_FEATS_DIS:
            raise NotImplementedError("ATTN_GNN_CONFIG.USE_FEATS_DIS: True (neighbours by feature distance) is not built")
        self.k = model_cfg.K
        self.edge_layes = nn.ModuleList()
        in_channels = input_channels
        for c in mlps:
            self.edge_layes.append(nn.Sequential(nn.Conv2d(in_channels * 2, c, kernel_size=1, bias=False), nn.BatchNorm2d(c), nn.ReLU()))
            in_channels = c
        in_channels = sum(mlps)
        self.calib = nn.Sequential(nn.Conv1d(in_channels, model_cfg.CALIB_DIM, kernel_size=1, bias=False),
                                   nn.BatchNorm1d(model_cfg.CALIB_DIM), nn.ReLU(),
                                   nn.Conv1d(model_cfg.CALIB_DIM, in_channels, kernel_size=1))
        self.expansion = network_utils.make_fc_layers(model_cfg.EXP_MLPS, in_channels, linear=False)
        in_channels = model_cfg.EXP_MLPS[-1]
        self.reduction = nn.Sequential(nn.Conv1d(in_channels, self.out_channel, kernel_size=1, bias=False),
                                       nn.BatchNorm1d(self.out_channel), nn.ReLU()) if model_cfg.USE_REDUCTION else None
        self.shortcut = ShortcutLayer(input_channels=self.out_channel, hidden_channels=self.out_channel,
                                      dropout=0.1) if model_cfg.USE_SHORT_CUT else None

    @staticmethod
    def knn(x, k=8):
        """x (T, 3, K) -> indices (T, K, k) of the k nearest points (the point itself included)."""
        inner = -2 * torch.matmul(x.transpose(2, 1), x)
        xx = torch.sum(x ** 2, dim=1, keepdim=True)
        return (-xx - inner - xx.transpose(2, 1)).topk(k=k, dim=-1)[1]

    @staticmethod
    def get_graph_feature(x, idx):
        """x (T, C, K), idx (T, K, k) -> edge features (T, 2 C, K, k): [neighbour - centre, centre]."""
        T, C, K = x.shape
        k = idx.shape[-1]
        flat = (idx + torch.arange(0, T, device=x.device).view(-1, 1, 1) * K).view(-1)
        x = x.transpose(2, 1).contiguous()
        feature = x.view(T * K, -1)[flat, :].view(T, K, k, C)
        x = x.view(T, K, 1, C).repeat(1, 1, k, 1)
        return torch.cat((feature - x, x), dim=3).permute(0, 3, 1, 2).contiguous()

    def forward(self, xyz, feats):
        B, M, K, _ = xyz.shape
        xyz = xyz.view(B * M, K, -1).permute(0, 2, 1).contiguous()
        feats = feats.view(B * M, K, -1).permute(0, 2, 1).contiguous()
        idx = self.knn(xyz, self.k)
        x = torch.cat([xyz, feats], dim=1)
        x_list = []
        for edge_layer in self.edge_layes:
            x = edge_layer(self.get_graph_feature(x, idx)).max(dim=-1)[0]
            x_list.append(x)
        x = torch.cat(x_list, dim=1)
        x = torch.sigmoid(self.calib(x)) * x
        x = self.expansion(x).max(dim=-1)[0].view(B, M, -1).permute(0, 2, 1)
        if self.reduction is not None:
            x = self.reduction(x)
        if self.shortcut is not None:
            x = self.shortcut(x)
        return x


class GraphRCNNHead(RoIHeadTemplate):
    def __init__(self, input_channels, model_cfg, point_cloud_range, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.pc_range = np.asarray(point_cloud_range, dtype=np.float32)
        patch_range = np.round(np.concatenate([self.pc_range[:3] - 1, self.pc_range[3:] + 1]))
        patch_size = np.array([1.0, 1.0, -1.0], dtype=np.float32)
        dfvs = model_cfg.DFVS_CONFIG
        self.roilocal_dfvs_pool3d_layer = patch_ops_utils.RoILocalDFVSPool3dV2(
            pc_range=patch_range, patch_size=patch_size, num_dvs_points=dfvs.NUM_DVS_POINTS, num_fps_points=dfvs.NUM_FPS_POINTS,
            hash_size=dfvs.HASH_SIZE, lambda_=dfvs.LAMBDA, delta=dfvs.DELTA, pool_extra_width=dfvs.POOL_EXTRA_WIDTH,
            num_boxes_per_patch=dfvs.NUM_BOXES_PER_PATCH)
        if model_cfg.get('IMG_CONFIG', None) is not None:
            raise NotImplementedError("ROI_HEAD.IMG_CONFIG (the image branch of GraphRCNNHead) is not built")
        if not _is_none(model_cfg.NMS_CONFIG.get('TEST', None)):
            raise NotImplementedError("ROI_HEAD.NMS_CONFIG.TEST (RoI selection by NMS inside the head) is not built")
        gnn_cfg = type(model_cfg.ATTN_GNN_CONFIG)(model_cfg.ATTN_GNN_CONFIG)       # the reference pops IN_DIM from the shared cfg
        input_channels = gnn_cfg.pop('IN_DIM')
        self.attn_gnn_layer = AttnGNNLayer(input_channels, gnn_cfg)
        self.shared_fc_layer = nn.Sequential(nn.Conv1d(self.attn_gnn_layer.out_channel, 256, kernel_size=1, bias=False),
                                             nn.BatchNorm1d(256), nn.ReLU())
        self.cls_layers = nn.Conv1d(256, self.num_class, kernel_size=1, bias=True)
        self.reg_layers = nn.Conv1d(256, self.box_coder.code_size, kernel_size=1, bias=True)
        self.init_weights()

    def init_weights(self):
        """xavier_normal_ on every convolution, zero biases, N(0, 0.001) for ``reg_layers`` (graphrcnn_head.py:181-199)."""
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                nn.init.xavier_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.reg_layers.weight, mean=0, std=0.001)

    def roipool3d_gpu(self, batch_dict):
        """-> feats_local (B M, K, 3 + C + 6), xyz_global (B M, K, 3), pooled_num (B M) for ``batch_dict['rois']``: one pooling
        call for the whole batch (the reference loops over the samples, graphrcnn_head.py:201-244)."""
        r = self.pc_range
        _, num, feats, glob = self.roilocal_dfvs_pool3d_layer.pool(batch_dict['points'], batch_dict['rois'][..., :7],
                                                                   range_xy=[r[0], r[1], r[3], r[4]])
        return feats, glob, num.view(-1)

    def forward(self, batch_dict):
        if self.training:
            raise NotImplementedError("GraphRCNNHead: training mode (proposal target layer, rcnn losses) is not built; call .eval()")
        self.proposal_layer(batch_dict, nms_config=self.model_cfg.NMS_CONFIG['TEST'])
        B, M, _ = batch_dict['rois'].shape
        roi_feats_local, _, roi_points_num = self.roipool3d_gpu(batch_dict)
        roi_feats_local = roi_feats_local * (roi_points_num > 0).unsqueeze(-1).unsqueeze(-1)
        pooled_features = self.pooled_to_features(roi_feats_local, B, M)
        rcnn_cls, rcnn_reg = self.heads(pooled_features, B, M)
        batch_cls_preds, batch_box_preds = self.generate_predicted_boxes(
            batch_size=batch_dict['batch_size'], rois=batch_dict['rois'], cls_preds=rcnn_cls, box_preds=rcnn_reg)
        roi_scores = batch_dict['roi_scores'] if batch_dict.get('cls_preds_normalized', False) else torch.sigmoid(batch_dict['roi_scores'])
        batch_dict['batch_cls_preds'] = torch.pow(torch.sigmoid(batch_cls_preds), 0.5) * torch.pow(roi_scores.unsqueeze(-1), 0.5)
        batch_dict['batch_box_preds'] = batch_box_preds
        batch_dict['cls_preds_normalized'] = True
        return batch_dict

    def forward_train(self, batch_dict, u_fg, u_bg):
        """One training forward (graphrcnn_head.py:254-301 with ``self.training``): proposal targets for the first stage's RoIs
        (``u_fg (B, M)``, ``u_bg (B, ROI_PER_IMAGE)`` decide the sampling), ``rois`` / ``roi_labels`` replaced by the sampled ones,
        pooling, graph network, heads; the result is left in ``forward_ret_dict`` for ``rcnn_losses`` (the reference's keys, and
        ``pooled_feats_local``: what the graph network was fed)."""
        if not _is_none(self.model_cfg.NMS_CONFIG.get('TRAIN', None)):
            raise NotImplementedError("ROI_HEAD.NMS_CONFIG.TRAIN (RoI selection by NMS inside the head) is not built")
        self.proposal_layer(batch_dict, nms_config=None)
        targets_dict = self.proposal_targets(batch_dict, u_fg, u_bg)
        batch_dict['rois'] = targets_dict['rois']
        batch_dict['roi_labels'] = targets_dict['roi_labels']
        B, M, _ = batch_dict['rois'].shape
        with torch.no_grad():
            roi_feats_local, _, roi_points_num = self.roipool3d_gpu(batch_dict)
            roi_feats_local = roi_feats_local * (roi_points_num > 0).unsqueeze(-1).unsqueeze(-1)
        rcnn_cls, rcnn_reg = self.heads(self.pooled_to_features(roi_feats_local, B, M), B, M)
        targets_dict['rcnn_cls'] = rcnn_cls
        targets_dict['rcnn_reg'] = rcnn_reg
        targets_dict['batch_size'] = batch_dict['batch_size']
        targets_dict['pooled_feats_local'] = roi_feats_local
        self.forward_ret_dict = targets_dict
        return batch_dict

    def pooled_to_features(self, roi_feats_local, B, M):
        """feats_local (B M, K, 3 + C + 6) -> (B, OUT_DIM, M) through the graph network."""
        f = roi_feats_local.view(B, M, -1, roi_feats_local.shape[-1])
        return self.attn_gnn_layer(f[..., :3], f[..., 3:])

    def heads(self, pooled_features, B, M):
        """(B, OUT_DIM, M) -> rcnn_cls (B M, num_class), rcnn_reg (B M, 7)."""
        shared = self.shared_fc_layer(pooled_features)
        rcnn_cls = self.cls_layers(shared).permute(0, 2, 1).contiguous().view(B * M, -1)
        rcnn_reg = self.reg_layers(shared).permute(0, 2, 1).contiguous().view(B * M, -1)
        return rcnn_cls, rcnn_reg
