"""``GraphRCNN``: the two-stage detector of tools/cfgs/waymo_models/gd_mae_ts.yaml in eval mode (reference
pcdet/models/detectors/graph_rcnn.py:4-25): module loop, then ``post_processing`` (its ``NMS: False`` branch for the shipped
config).  ``FREEZE_LAYERS`` is accepted: freezing the first stage is a training concern and has no effect in eval.
Training mode of this module keeps raising; the second stage trains through ``gdmae_hip.two_stage.SecondStageTrainer``,
which reads ``FREEZE_LAYERS``."""
from .detector3d_template import Detector3DTemplate


class GraphRCNN(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset, logger):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset, logger=logger)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        if self.training:
            raise NotImplementedError("GraphRCNN: second-stage training (rcnn losses) is not built; call .eval()")
        for m in self.module_list:
            batch_dict = m(batch_dict)
        return self.post_processing(batch_dict)
