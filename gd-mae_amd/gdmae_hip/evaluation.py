"""The recall record of an evaluation loop on the device (reference ``Detector3DTemplate.generate_recall_record``,
detector3d_template.py:318-358, and the bookkeeping of ``eval_one_epoch``, tools/eval_utils/eval_utils.py:30-35 and 103-110), for the
padded tensors of ``engine.detect``.

    rec = RecallRecord(cfg.MODEL.POST_PROCESSING.RECALL_THRESH_LIST, device)
    for batch_dict in loader:
        out = engine.detect(batch_dict, recall=rec)      # adds to rec.counters on the device, no host read
    rec.result()                                         # {'gt_num': .., 'recall_roi_0.3': .., 'recall_rcnn_0.3': .., ...}: ONE host read
    rec.ret_dict()                                       # {'recall/roi_0.3': .., 'recall/rcnn_0.3': .., ...}

The contract, stated once in numpy by ``recall_record_numpy``:

* valid GT rows of a sample: 0 .. k, k the last row with a non-zero entry; none if no row has one.  An all-zero row in between counts
  in ``gt_num`` and is never recalled;
* IoU = rotated BEV overlap x clamped height overlap / max(vol_a + vol_b - overlap, 1e-6), the operations of ``boxes_iou3d_gpu``;
* a GT row is recalled at t when its largest IoU over the predicted rows (rcnn) / the RoI rows (roi) is > t, compared in fp32; rows
  at or beyond ``pred_num[b]`` / ``roi_num[b]`` do not exist; the largest IoU over no rows is 0;
* ``gt_num`` grows by the valid count whether or not there are predictions; the roi counters move only when RoIs are given.

``update`` sends device tensors to ``gdmae_recall_record`` (csrc/recall_record.hip: two launches, no atomics, no fallback)."""
from __future__ import annotations

import numpy as np
import torch

MAX_THRESHOLDS = 8


def counter_names(thresh_list):
    """Keys of the reference's ``recall_dict`` in the order of ``RecallRecord.counters``: the thresholds formatted by ``str``."""
    return ['gt_num'] + ['recall_roi_%s' % str(t) for t in thresh_list] + ['recall_rcnn_%s' % str(t) for t in thresh_list]


def valid_gt_rows(gt):
    """gt (G, cols) -> number of valid rows: 1 + the last row with a non-zero entry, 0 when there is none."""
    nz = np.nonzero((np.asarray(gt) != 0).any(axis=1))[0]
    return int(nz[-1]) + 1 if nz.size else 0


def recall_record_numpy(pred_boxes, pred_num, gt_boxes, thresh_list, rois=None, roi_num=None, bev_overlap=None):
    """The statement with fp64 geometry.  numpy arrays in -> (counters (1 + 2 T) int64, best_iou (B, G, 2) fp64: [.., 0] over the RoI
    rows, [.., 1] over the predicted rows).  ``bev_overlap(a, b)``: the BEV overlap of two boxes (default: the package's exact fp64
    convex clipping)."""
    from pcdet.models.roi_heads import proposal_targets as pt
    bev_overlap = bev_overlap or pt.exact_bev_overlap
    f32 = np.float32
    pred_boxes, gt_boxes = np.asarray(pred_boxes, f32), np.asarray(gt_boxes, f32)
    B, G = gt_boxes.shape[:2]
    T = len(thresh_list)
    counters, best = np.zeros(1 + 2 * T, np.int64), np.zeros((B, G, 2), np.float64)
    sides = [(1, pred_boxes, pred_num)] + ([(0, np.asarray(rois, f32), roi_num)] if rois is not None else [])
    for b in range(B):
        nv = valid_gt_rows(gt_boxes[b])
        counters[0] += nv
        for col, rows, num in sides:
            n = rows.shape[1] if num is None else min(max(int(num[b]), 0), rows.shape[1])
            for g in range(nv):
                best[b, g, col] = max([pt.iou3d_fp64(rows[b, p], gt_boxes[b, g], bev_overlap) for p in range(n)], default=0.0)
            for i, t in enumerate(thresh_list):
                counters[1 + (T if col else 0) + i] += int((best[b, :nv, col].astype(f32) > f32(t)).sum())
    return counters, best


class RecallRecord:
    """``counters`` (1 + 2 T) int64 on ``device`` = [gt_num, roi_t0 .., rcnn_t0 ..]: a public tensor, accumulated over ``update`` calls
    and read by ``result`` only (a distributed caller may ``all_reduce`` it first)."""

    def __init__(self, thresh_list, device):
        self.thresh_list = list(thresh_list)
        if not 1 <= len(self.thresh_list) <= MAX_THRESHOLDS:
            raise ValueError(f"RecallRecord: {len(self.thresh_list)} thresholds (1 .. {MAX_THRESHOLDS})")
        self.counters = torch.zeros(1 + 2 * len(self.thresh_list), dtype=torch.int64, device=device)

    def reset(self):
        self.counters.zero_()

    def update(self, pred_boxes, pred_num, gt_boxes, rois=None, roi_num=None):
        """pred_boxes (B, n, >= 7), pred_num (B) or None (all n rows), gt_boxes (B, G, >= 7), optionally rois (B, M, >= 7) with roi_num
        the same way: adds the batch to ``counters`` -> best_iou (B, G, 2) fp32 on the device.  No host read."""
        from . import lib as L
        given = [t for t in (pred_boxes, pred_num, gt_boxes, rois, roi_num) if t is not None]
        if not all(t.is_cuda for t in given) or not self.counters.is_cuda:
            raise NotImplementedError("RecallRecord.update: CPU tensors (the record is computed in libgdmae_hip.so, no CPU fallback)")
        if pred_boxes.dim() != 3 or gt_boxes.dim() != 3 or gt_boxes.shape[0] != pred_boxes.shape[0] or (rois is not None and (
                rois.dim() != 3 or rois.shape[0] != pred_boxes.shape[0])):
            raise ValueError("RecallRecord.update: pred_boxes (B, n, >= 7), gt_boxes (B, G, >= 7), rois (B, M, >= 7)")
        if roi_num is not None and rois is None:
            raise ValueError("RecallRecord.update: roi_num without rois")
        B, n, pc = pred_boxes.shape
        G, gc = gt_boxes.shape[1:]
        for num in (pred_num, roi_num):
            if num is not None and tuple(num.shape) != (B,):
                raise ValueError("RecallRecord.update: pred_num / roi_num of shape (B)")
        f = lambda t: t.float().contiguous()                         # noqa: E731
        i = lambda t: None if t is None else t.to(torch.int32).contiguous()      # noqa: E731
        pred_boxes, gt_boxes, pred_num, roi_num = f(pred_boxes), f(gt_boxes), i(pred_num), i(roi_num)
        M, rc = (0, 7)
        if rois is not None:
            rois = f(rois)
            M, rc = rois.shape[1:]
        best = torch.empty(B, G, 2, dtype=torch.float32, device=gt_boxes.device)
        L.call("gdmae_recall_record", L.ptr(pred_boxes), L.ptr(pred_num), B, n, pc, L.ptr(rois), L.ptr(roi_num), M, rc, L.ptr(gt_boxes), G, gc,
               L.host_f32(self.thresh_list), len(self.thresh_list), L.ptr(self.counters), L.ptr(best), L.stream())
        return best

    def result(self):
        """The reference's ``recall_dict`` summed over the updates (Python ints).  ONE host read."""
        return dict(zip(counter_names(self.thresh_list), self.counters.tolist()))

    def ret_dict(self):
        """``recall/roi_t`` and ``recall/rcnn_t`` = count / max(gt_num, 1), as ``eval_one_epoch`` reports them.  ONE host read."""
        r = self.result()
        gt_num = max(r['gt_num'], 1)
        out = {}
        for t in self.thresh_list:
            out['recall/roi_%s' % str(t)] = r['recall_roi_%s' % str(t)] / gt_num
            out['recall/rcnn_%s' % str(t)] = r['recall_rcnn_%s' % str(t)] / gt_num
        return out


def post_cfg_record(post_cfg, recall, batch_dict):
    """What ``engine.detect(batch_dict, recall=...)`` decides before it runs: -> the record to update, or None (no record given, no
    ``gt_boxes`` in the batch, or ``RECALL_MODE`` other than ``normal``).  The record's thresholds must be ``RECALL_THRESH_LIST``."""
    if recall is None or 'gt_boxes' not in batch_dict or post_cfg.get('RECALL_MODE', 'normal') != 'normal':
        return None
    if [float(t) for t in post_cfg.RECALL_THRESH_LIST] != [float(t) for t in recall.thresh_list]:
        raise ValueError(f"detect: the record's thresholds {recall.thresh_list} are not POST_PROCESSING.RECALL_THRESH_LIST "
                         f"{list(post_cfg.RECALL_THRESH_LIST)}")
    return recall


def evaluate(engine, batches, keep_predictions=True):
    """The loop of ``eval_one_epoch`` without dataset code: ``engine.detect`` with one record over ``batches`` (an iterable of
    ``batch_dict``) -> (pred_dicts: the per-sample list over all batches, or None; ``ret_dict``).  With ``keep_predictions`` False the
    loop makes no host read beyond those ``detect`` itself makes; the record is read once at the end."""
    rec = None
    pred_dicts = [] if keep_predictions else None
    to_list = engine.model.padded_to_pred_dicts          # Detector3DTemplate: rows 0 .. num[b] - 1 of every sample, ONE host read
    for bd in batches:
        if rec is None:
            rec = RecallRecord(engine.model.model_cfg.POST_PROCESSING.RECALL_THRESH_LIST, bd['points'].device)
        out = engine.detect(bd, recall=rec)
        if keep_predictions:
            pred_dicts += to_list(out)
    return pred_dicts, (rec.ret_dict() if rec is not None else {})
