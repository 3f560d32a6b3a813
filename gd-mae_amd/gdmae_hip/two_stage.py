"""Second-stage training of the two-stage detector (``GraphRCNN`` + ``GraphRCNNHead``, tools/cfgs/waymo_models/gd_mae_ts.yaml):

    trainer = SecondStageTrainer(model, rng=np.random.RandomState(0))
    ret, tb_dict, disp_dict = trainer(batch_dict)          # batch_dict: points, batch_size, gt_boxes (B, G, 8)
    ret['loss'].backward()

as the reference's ``GraphRCNN.forward`` returns in training (detectors/graph_rcnn.py:11-39) under the shipped
``FREEZE_LAYERS``: every module in front of the RoI head is frozen - run in eval mode under ``torch.no_grad()``, parameters with
``requires_grad = False``; the reference's ``FrozenBatchNorm`` is the running-statistics affine map, which is what eval mode
computes - and the RoI head trains (BatchNorm on batch statistics).  The loss is the rcnn loss alone, as in the reference when
``FREEZE_LAYERS`` is set.  Joint training of both stages (``FREEZE_LAYERS: None``) is not built and raises by name.

The proposal targets are sampled on the device from uniform numbers drawn here (``u_fg`` per RoI, then ``u_bg`` per sampled
slot); ``model.train()(batch_dict)`` itself keeps raising."""
import numpy as np
import torch
import torch.nn as nn


class SecondStageTrainer(nn.Module):
    def __init__(self, model, rng=None):
        super().__init__()
        head = getattr(model, 'roi_head', None)
        if head is None or not hasattr(head, 'forward_train'):
            raise NotImplementedError(f"SecondStageTrainer: {type(model).__name__} has no RoI head with forward_train")
        frozen = model.model_cfg.get('FREEZE_LAYERS', None)
        first = [m for m in model.module_list if m is not head]
        missing = [type(m).__name__ for m in first if frozen is None or type(m).__name__ not in frozen]
        if missing:
            raise NotImplementedError(f"SecondStageTrainer: FREEZE_LAYERS {frozen} does not cover {missing}; joint training of both "
                                      "stages is not built")
        self.model = model
        self.rng = rng if rng is not None else np.random.RandomState()
        self._first = first
        for m in first:
            for p in m.parameters():
                p.requires_grad = False
        self.train()

    def train(self, mode=True):
        """The RoI head follows ``mode``; the frozen first stage stays in eval mode."""
        super().train(mode)
        for m in self._first:
            m.eval()
        return self

    def trainable_parameters(self):
        return list(self.model.roi_head.parameters())

    def draw(self, B, M, R, device):
        """``u_fg (B, M)`` then ``u_bg (B, R)`` from ``rng`` as float32, copied to ``device``."""
        u_fg = self.rng.random_sample((B, M)).astype(np.float32)
        u_bg = self.rng.random_sample((B, R)).astype(np.float32)
        # a float64 draw just below 1 rounds to 1.0f: keep the contract's [0, 1)
        top = np.nextafter(np.float32(1), np.float32(0))
        return torch.from_numpy(np.minimum(u_fg, top)).to(device), torch.from_numpy(np.minimum(u_bg, top)).to(device)

    def forward(self, batch_dict, u_fg=None, u_bg=None):
        head = self.model.roi_head
        have = [k in batch_dict for k in ('rois', 'roi_scores', 'roi_labels')]
        if any(have) and not all(have):
            raise ValueError("SecondStageTrainer: give rois, roi_scores and roi_labels together, or none of them")
        with torch.no_grad():
            for m in self._first:
                if all(have) and m is getattr(self.model, 'dense_head', None):
                    continue                                   # the caller's RoIs stand in for the first stage's head
                batch_dict = m(batch_dict)
        B, M = batch_dict['rois'].shape[:2]
        if u_fg is None or u_bg is None:
            if u_fg is not None or u_bg is not None:
                raise ValueError("SecondStageTrainer: give u_fg and u_bg together, or neither")
            u_fg, u_bg = self.draw(B, M, int(head.model_cfg.TARGET_CONFIG.ROI_PER_IMAGE), batch_dict['rois'].device)
        head.forward_train(batch_dict, u_fg, u_bg)
        loss, tb_dict = head.rcnn_losses(head.forward_ret_dict)
        return {'loss': loss}, tb_dict, {}
