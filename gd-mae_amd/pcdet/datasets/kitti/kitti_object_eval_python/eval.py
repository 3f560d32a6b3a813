"""``get_official_eval_result`` where OpenPCDet's ``KittiDataset.evaluation`` looks for it
(``from .kitti_object_eval_python import eval as kitti_eval``): the official KITTI AP table computed by this package
(gdmae_hip/evaluation.py) - on the device when there is one, by the numpy statement otherwise.  No numba."""
import torch

from gdmae_hip import evaluation


def get_official_eval_result(gt_annos, dt_annos, current_classes, PR_detail_dict=None):
    if torch.cuda.is_available():
        return evaluation.kitti_eval(gt_annos, dt_annos, current_classes, PR_detail_dict=PR_detail_dict)
    return evaluation.kitti_eval_numpy(gt_annos, dt_annos, current_classes, PR_detail_dict=PR_detail_dict)
