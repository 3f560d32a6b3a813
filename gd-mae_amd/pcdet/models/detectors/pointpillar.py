"""``PointPillar`` detector wrapper of the shipped KITTI fine-tune config (tools/cfgs/kitti_models/gd_mae.yaml:54-55): module loop,
``dense_head.get_loss()`` and the template's ``post_processing`` (reference pcdet/models/detectors/pointpillar.py:4-36).
``sync_loss_scalar`` as in ``CenterPoint``: the reference reads four loss scalars with ``.item()`` every step; here they are read
in one transfer, and not at all when it is False (the step is then free of host syncs)."""
import torch

from .detector3d_template import Detector3DTemplate


class PointPillar(Detector3DTemplate):
    sync_loss_scalar = True

    def __init__(self, model_cfg, num_class, dataset, logger):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset, logger=logger)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        for m in self.module_list:
            batch_dict = m(batch_dict)
        if self.training:
            loss, tb_dict, disp_dict = self.get_training_loss()
            return {'loss': loss}, tb_dict, disp_dict
        return self.post_processing(batch_dict)

    def get_training_loss(self):
        loss_rpn, tb_dict = self.dense_head.get_loss()
        tb_dict = {'loss_rpn': loss_rpn.detach(), **tb_dict}
        if self.sync_loss_scalar:
            keys = list(tb_dict)
            vals = torch.stack([tb_dict[k].float().reshape(()) for k in keys]).tolist()      # one device-to-host read
            tb_dict = dict(zip(keys, vals))
        return loss_rpn, tb_dict, {}
