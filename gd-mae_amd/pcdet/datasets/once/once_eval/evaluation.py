"""``get_evaluation_results`` where OpenPCDet's ``ONCEDataset.evaluation`` looks for it
(``from .once_eval.evaluation import get_evaluation_results``): the ONCE AP table computed by this package
(gdmae_hip/evaluation.py) - on the device when there is one, by the numpy statement otherwise.  No numba."""
import torch

from gdmae_hip import evaluation

iou_threshold_dict = dict(evaluation.ONCE_IOU_THRESHOLDS)
superclass_iou_threshold_dict = dict(evaluation.ONCE_SUPERCLASS_IOU_THRESHOLDS)


def get_evaluation_results(gt_annos, pred_annos, classes, use_superclass=True, iou_thresholds=None, num_pr_points=50,
                           difficulty_mode='Overall&Distance', ap_with_heading=True, num_parts=100, print_ok=False):
    fn = evaluation.once_eval if torch.cuda.is_available() else evaluation.once_eval_numpy
    return fn(gt_annos, pred_annos, classes, use_superclass=use_superclass, iou_thresholds=iou_thresholds, num_pr_points=num_pr_points,
              difficulty_mode=difficulty_mode, ap_with_heading=ap_with_heading, num_parts=num_parts, print_ok=print_ok)
