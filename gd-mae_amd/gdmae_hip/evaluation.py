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

``update`` sends device tensors to ``gdmae_recall_record`` (csrc/recall_record.hip: two launches, no atomics, no fallback).

The second part of this module is the official KITTI AP table (``kitti_eval``, ``KittiEval``, ``kitti_eval_numpy``), the
third the KITTI annos of the detections on the device (``KittiDetections``, ``kitti_prediction_dicts``, ``evaluate_kitti``,
``kitti_annos_numpy``), the fourth the ONCE AP table and its record (``once_eval``, ``OnceEval``, ``once_eval_numpy``,
``OnceDetections``, ``once_prediction_dicts``, ``evaluate_once``)."""
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


# ------------------------------------------------------------------------------------------------------------------------------------
# The official KITTI AP table (reference pcdet/datasets/kitti/kitti_object_eval_python/eval.py ``get_official_eval_result``)
#
#     result_str, ret_dict = kitti_eval(gt_annos, dt_annos, class_names)             # libgdmae_hip.so, ONE host read
#     result_str, ret_dict = kitti_eval_numpy(gt_annos, dt_annos, class_names)       # the statement: fp64 geometry, numpy, CPU
#
# A "combo" is (metric, class, difficulty, overlap set) in that order: index ((m * C + c) * 3 + l) * 2 + k, metric 0 bbox, 1 bev, 2 3d.
# ------------------------------------------------------------------------------------------------------------------------------------
KITTI_CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting', 'Truck']
KITTI_MIN_HEIGHT = [40, 25, 25]
KITTI_MAX_OCCLUSION = [0, 1, 2]
KITTI_MAX_TRUNCATION = [0.15, 0.3, 0.5]
# (overlap set, metric, class): the two official sets
KITTI_MIN_OVERLAPS = np.stack([np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.7], [0.7, 0.5, 0.5, 0.7, 0.5, 0.7], [0.7, 0.5, 0.5, 0.7, 0.5, 0.7]]),
                               np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5]])], axis=0)
KITTI_SAMPLE_PTS = 41
KITTI_MAX_ROWS = 1024                  # detections / GT rows per frame (csrc/kitti_eval.hip: 16 mask bits per lane)
KITTI_NO_DETECTION = -10000000


def kitti_class_ints(class_names):
    if not isinstance(class_names, (list, tuple)):
        class_names = [class_names]
    return [KITTI_CLASS_NAMES.index(c) if isinstance(c, str) else int(c) for c in class_names]


def kitti_compute_aos(dt_annos):
    """The reference's decision: the first detection anno with rows decides, by ``alpha[0] != -10``."""
    for anno in dt_annos:
        if anno['alpha'].shape[0] != 0:
            return bool(anno['alpha'][0] != -10)
    return False


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64)


def _cat(parts, width=None, dtype=None):
    parts = [np.asarray(p).reshape((-1,) if width is None else (-1, width)) for p in parts]
    out = np.concatenate(parts, axis=0) if parts else np.zeros((0,) if width is None else (0, width))
    return out if dtype is None else out.astype(dtype)


def _per_row(annos, keys, widths, fn):
    """fn(columns ..) -> (3, rows) on the rows of all frames.  One call on the concatenated columns when every frame holds a column
    in the same dtype (concatenation then changes no value and no comparison); frame by frame otherwise, so that no frame's values
    are widened before they are compared."""
    cols = [[np.asarray(a[k]).reshape((-1,) if w is None else (-1, w)) for a in annos] for k, w in zip(keys, widths)]
    if not annos:
        return np.zeros((3, 0), bool)
    if all(len({c.dtype for c in col}) == 1 for col in cols):
        return fn(*[np.concatenate(col, axis=0) for col in cols])
    return np.concatenate([fn(*parts) for parts in zip(*cols)], axis=1)


class _LowerNames:
    """``names.lower() == word`` for a whole column of names: on the code points of the fixed-width array when all of them are ASCII
    (``np.char.lower`` is a Python call per name), through ``np.char.lower`` otherwise."""

    def __init__(self, raw):
        raw = np.ascontiguousarray(raw)
        self.width = raw.dtype.itemsize // 4
        self.codes = raw.view(np.uint32).reshape(len(raw), self.width).copy()
        self.lowered = None
        if self.codes.size and int(self.codes.max()) > 127:
            self.lowered = np.char.lower(raw)
        else:
            self.codes[(self.codes >= 65) & (self.codes <= 90)] += 32

    def __eq__(self, word):
        if self.lowered is not None:
            return self.lowered == word
        if len(word) > self.width or not word:
            return np.zeros(len(self.codes), bool)
        n = min(len(word) + 1, self.width)                      # the word and, where the column is wider, its end
        want = np.zeros(n, np.uint32)
        want[:len(word)] = [ord(ch) for ch in word]
        return (self.codes[:, :n] == want[None, :]).all(axis=1)


def kitti_clean_data(gt_annos, dt_annos, classes):
    """``clean_data`` of the reference for every (class, difficulty) at once, vectorised over the rows of all frames (the comparisons
    run on the annos' own dtype, see ``_per_row``) -> dict: gt_off / dt_off / dc_off (F + 1) int64, ignored_gt (C, 3, NG) /
    ignored_dt (C, 3, ND) int8, num_valid (C, 3) int64, dc_rows (NG) bool (``name == "DontCare"``, exact case)."""
    if len(gt_annos) != len(dt_annos):
        raise ValueError(f"kitti_eval: {len(gt_annos)} GT annos and {len(dt_annos)} detection annos")
    return dict(kitti_clean_gt(gt_annos, classes), **kitti_clean_dt(dt_annos, classes))


def _anno_names(annos):
    return np.concatenate([np.asarray(a['name'], dtype=str).reshape(-1) for a in annos] + [np.zeros(0, dtype=str)])


def kitti_clean_gt(gt_annos, classes):
    """The GT half of ``kitti_clean_data``: gt_off, dc_off, ignored_gt, num_valid, dc_rows."""
    C = len(classes)
    gt_raw = _anno_names(gt_annos)
    gt_name = _LowerNames(gt_raw)
    gt_count = [len(a['name']) for a in gt_annos]
    gt_off = _offsets(gt_count)
    dc_rows = gt_raw == "DontCare"
    dc_count = np.bincount(np.repeat(np.arange(len(gt_annos)), gt_count)[dc_rows], minlength=len(gt_annos))
    NG = int(gt_off[-1])
    gt_ignore = _per_row(gt_annos, ('occluded', 'truncated', 'bbox'), (None, None, 4), lambda occ, tr, bb: np.stack(
        [(occ > KITTI_MAX_OCCLUSION[l]) | (tr > KITTI_MAX_TRUNCATION[l]) | ((bb[:, 3] - bb[:, 1]) <= KITTI_MIN_HEIGHT[l]) for l in range(3)]))
    ignored_gt = np.full((C, 3, NG), -1, np.int8)
    for c, cls in enumerate(classes):
        name = KITTI_CLASS_NAMES[cls].lower()
        own = gt_name == name
        neighbour = gt_name == {'pedestrian': 'person_sitting', 'car': 'van'}.get(name, '')       # rows that count as "ignored 1"
        for l in range(3):
            ignored_gt[c, l][own & ~gt_ignore[l]] = 0
            ignored_gt[c, l][neighbour | (own & gt_ignore[l])] = 1
    return dict(gt_off=gt_off, dc_off=_offsets(dc_count), ignored_gt=ignored_gt, num_valid=(ignored_gt == 0).sum(axis=2).astype(np.int64),
                dc_rows=dc_rows)


def kitti_clean_dt(dt_annos, classes):
    """The detection half of ``kitti_clean_data``: dt_off, ignored_dt (what csrc/kitti_annos.hip decides on the device)."""
    C = len(classes)
    dt_name = _LowerNames(_anno_names(dt_annos))
    dt_off = _offsets([len(a['name']) for a in dt_annos])
    dt_small = _per_row(dt_annos, ('bbox',), (4,), lambda bb: np.stack([np.abs(bb[:, 3] - bb[:, 1]) < KITTI_MIN_HEIGHT[l] for l in range(3)]))
    ignored_dt = np.full((C, 3, int(dt_off[-1])), -1, np.int8)
    for c, cls in enumerate(classes):
        own_dt = dt_name == KITTI_CLASS_NAMES[cls].lower()
        for l in range(3):
            ignored_dt[c, l][own_dt] = 0
            ignored_dt[c, l][dt_small[l]] = 1
    return dict(dt_off=dt_off, ignored_dt=ignored_dt)


def kitti_combos(classes, num_valid):
    """-> (combo_cl, combo_metric int32, combo_min fp64, combo_num_gt int32), each (3 * C * 3 * 2) in combo order."""
    C = len(classes)
    mo = KITTI_MIN_OVERLAPS[:, :, classes]
    cl, me, mn, ng = [], [], [], []
    for m in range(3):
        for c in range(C):
            for l in range(3):
                for k in range(2):
                    cl.append(c * 3 + l), me.append(m), mn.append(mo[k, m, c]), ng.append(num_valid[c, l])
    return np.array(cl, np.int32), np.array(me, np.int32), np.array(mn, np.float64), np.array(ng, np.int32)


def kitti_get_thresholds(scores_desc, num_gt, num_sample_pts=KITTI_SAMPLE_PTS):
    """``get_thresholds`` on scores already in descending order, the reference's sequence of fp64 operations."""
    current_recall, out, n = 0, [], len(scores_desc)
    for i in range(n):
        l_recall = (i + 1) / num_gt
        r_recall = (i + 2) / num_gt if i < n - 1 else l_recall
        if (r_recall - current_recall) < (current_recall - l_recall) and i < n - 1:
            continue
        out.append(scores_desc[i])
        current_recall += 1 / (num_sample_pts - 1.0)
    return out


def kitti_curves(n_thresholds, pr_counts, pr_sim, n_classes, compute_aos):
    """(K) counts, (K, 41, 3) tp / fp / fn, (K, 41) similarity sums -> precision, recall, aos, each (3, C, 3, 2, 41) fp64: the
    quotients where a threshold exists, 0 behind the count, then the reverse running maximum over ``i:`` with numpy's 0 / 0."""
    pts = KITTI_SAMPLE_PTS
    tp, fp, fn = (np.asarray(pr_counts)[..., i].astype(np.float64) for i in range(3))
    mask = np.arange(pts)[None, :] < np.asarray(n_thresholds).reshape(-1, 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        curves = [tp / (tp + fp), tp / (tp + fn), np.asarray(pr_sim, np.float64) / (tp + fp) if compute_aos else np.zeros_like(tp)]
    out = []
    for x in curves:
        x = np.where(mask, x, 0.0)
        x = np.maximum.accumulate(x[:, ::-1], axis=1)[:, ::-1]
        out.append(np.where(mask, x, 0.0).reshape(3, n_classes, 3, 2, pts))
    out[2][1:] = 0.0                                          # the reference computes the orientation curve with the bbox metric only
    return tuple(out)


def kitti_map(prec):
    sums = 0
    for i in range(0, prec.shape[-1], 4):
        sums = sums + prec[..., i]
    return sums / 11 * 100


def kitti_map_r40(prec):
    sums = 0
    for i in range(1, prec.shape[-1]):
        sums = sums + prec[..., i]
    return sums / 40 * 100


def kitti_format_result(classes, precision, aos, compute_aos, PR_detail_dict=None):
    """precision / aos (3, C, 3, 2, 41) -> (the reference's result text, its ``ret_dict``); fills ``PR_detail_dict``."""
    mo = KITTI_MIN_OVERLAPS[:, :, classes]
    ap, ap40 = [kitti_map(precision[m]) for m in range(3)], [kitti_map_r40(precision[m]) for m in range(3)]
    aos_ap, aos_ap40 = (kitti_map(aos[0]), kitti_map_r40(aos[0])) if compute_aos else (None, None)
    if PR_detail_dict is not None:
        PR_detail_dict['bbox'] = precision[0]
        if compute_aos:
            PR_detail_dict['aos'] = aos[0]
        PR_detail_dict['bev'], PR_detail_dict['3d'] = precision[1], precision[2]
    row = lambda tag, v, j, i, digits: "%s AP:" % tag + ", ".join(f"{v[j, d, i]:.{digits}f}" for d in range(3)) + "\n"      # noqa: E731
    result, ret = '', {}
    for j, cls in enumerate(classes):
        name = KITTI_CLASS_NAMES[cls]
        for i in range(mo.shape[0]):
            for head, tab, ao in (("AP", ap, aos_ap), ("AP_R40", ap40, aos_ap40)):
                result += f"{name} {head}@" + "{:.2f}, {:.2f}, {:.2f}:".format(*mo[i, :, j]) + "\n"
                result += row("bbox", tab[0], j, i, 4) + row("bev ", tab[1], j, i, 4) + row("3d  ", tab[2], j, i, 4)
                if compute_aos:
                    result += row("aos ", ao, j, i, 2)
            if i == 0:
                if compute_aos:
                    for d, diff in enumerate(('easy', 'moderate', 'hard')):
                        ret['%s_aos/%s_R40' % (name, diff)] = aos_ap40[j, d, 0]
                for key, m in (('3d', 2), ('bev', 1), ('image', 0)):
                    for d, diff in enumerate(('easy', 'moderate', 'hard')):
                        ret['%s_%s/%s_R40' % (name, key, diff)] = ap40[m][j, d, 0]
    return result, ret


def kitti_geometry(annos, with_score):
    """Concatenated rows of all frames in the annos' dtypes: bbox (n, 4), geo (n, 7) = location, dimensions, rotation_y, alpha, score."""
    geo = np.concatenate([_cat([a['location'] for a in annos], 3), _cat([a['dimensions'] for a in annos], 3),
                          _cat([a['rotation_y'] for a in annos])[:, None]], axis=1)
    out = dict(bbox=_cat([a['bbox'] for a in annos], 4), geo=geo, alpha=_cat([a['alpha'] for a in annos]))
    if with_score:
        out['score'] = _cat([a['score'] for a in annos])
    return out


def kitti_statement_overlaps(gt, dt, dc_box, bev_overlap):
    """One frame, fp64: gt / dt dicts of bbox (n, 4) and geo (n, 7) -> (overlaps (3, D, G), detection x DontCare image overlaps (D, NC), criterion 0)."""
    G, D = gt['bbox'].shape[0], dt['bbox'].shape[0]
    ov = np.zeros((3, D, G), np.float64)
    a, b = dt['bbox'].astype(np.float64)[:, None, :], gt['bbox'].astype(np.float64)[None, :, :]

    def image(a, b, iou):
        iw = np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0])
        ih = np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1])
        area = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
        ua = area + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) - iw * ih if iou else area + 0 * iw
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where((iw > 0) & (ih > 0), iw * ih / ua, 0.0)
    ov[0] = image(a, b, True)
    dg, gg = dt['geo'].astype(np.float64), gt['geo'].astype(np.float64)
    rect = lambda r: [r[0], r[2], 0.0, r[3], r[5], 0.0, -r[6]]      # noqa: E731   (x, z, l, w): rotation_y turns clockwise in (x, z)
    for j in range(D):
        for i in range(G):
            inter = bev_overlap(rect(dg[j]), rect(gg[i]))
            if inter > 0:
                ov[1, j, i] = inter / (dg[j, 3] * dg[j, 5] + gg[i, 3] * gg[i, 5] - inter)
                ih = min(dg[j, 1], gg[i, 1]) - max(dg[j, 1] - dg[j, 4], gg[i, 1] - gg[i, 4])
                if ih > 0:
                    inc = ih * inter
                    ov[2, j, i] = inc / (dg[j, 3] * dg[j, 4] * dg[j, 5] + gg[i, 3] * gg[i, 4] * gg[i, 5] - inc)
    return ov, image(a, dc_box.astype(np.float64)[None, :, :], False)


def _first_pass(enough, score, flag_gt, flag_pred, sentinel):
    """The first greedy pass of both evaluators on one frame (KITTI ``compute_statistics_jit(compute_fp=False)``, ONCE
    ``accumulate_scores``): enough (G, P) bool, "this pair overlaps enough" -> the true positives' scores per GT row, -inf elsewhere.
    A flag is -1 (not of this combo), 0 (counts) or 1 (ignored); a score at or below ``sentinel`` never matches."""
    G, P = enough.shape
    out, assigned = np.full(G, -np.inf, np.float32), np.zeros(P, bool)
    live = (flag_pred != -1) & (score > sentinel)
    for g in range(G):
        if flag_gt[g] == -1:
            continue
        cand = live & ~assigned & enough[g]
        if not cand.any():
            continue
        j = int(np.argmax(np.where(cand, score, -np.inf)))      # the highest score; among equal scores the lowest index (strict >)
        assigned[j] = True
        if not (flag_gt[g] == 1 or flag_pred[j] == 1):
            out[g] = score[j]
    return out


def _second_pass(ov, enough, score, flag_gt, flag_pred, thresholds):
    """The second greedy pass of both evaluators on one frame (KITTI ``compute_statistics_jit(compute_fp=True)``, ONCE
    ``compute_statistics``) for all T thresholds at once: ov / enough (G, P) -> tp, fn (T) int64, keep, assigned (T, P) bool (at or
    above the threshold; taken by a GT row), picked (G, T) int64 (the prediction of a true positive, -1 elsewhere).  Per GT row the
    reference's loop over the predictions ends with the flag-0 candidate of the largest overlap (the first of equals), and only
    without one with the FIRST flag-1 candidate.  False positives are the caller's: the two evaluators count them differently."""
    G, P = ov.shape
    T = len(thresholds)
    keep = ~(score[None, :] < np.asarray(thresholds, np.float32)[:, None])
    c0, c1 = keep & (flag_pred == 0)[None, :], keep & (flag_pred == 1)[None, :]
    assigned, picked = np.zeros((T, P), bool), np.full((G, T), -1, np.int64)
    tp, fn, rows = np.zeros(T, np.int64), np.zeros(T, np.int64), np.arange(T)
    for g in range(G):
        if flag_gt[g] == -1 or P == 0:
            fn += int(flag_gt[g] == 0)
            continue
        m0 = c0 & ~assigned & enough[g][None, :]
        has0 = m0.any(axis=1)
        j0 = np.argmax(np.where(m0, ov[g][None, :], -1.0), axis=1)
        m1 = c1 & ~assigned & enough[g][None, :]
        has1 = m1.any(axis=1) & ~has0
        j = np.where(has0, j0, np.argmax(m1, axis=1))
        found = has0 | has1
        if flag_gt[g] == 0:
            fn += ~found
        assigned[rows[found], j[found]] = True
        is_tp = has0 & (flag_gt[g] == 0)
        tp += is_tp
        picked[g, is_tp] = j[is_tp]
    return tp, fn, keep, assigned, picked


def _kitti_second_pass(ov, score, gt_alpha, dt_alpha, ign_gt, ign_dt, dc_max, min_ov, thresholds, compute_aos):
    """``_second_pass`` on one frame's (D, G) overlaps -> tp, fp, fn (T) int64, sim (T) fp64.  A detection left over is no false
    positive where it lies on a DontCare box (``dc_max``, metric 0); the similarity is summed over the GT rows in their order."""
    tp, fn, keep, assigned, picked = _second_pass(ov.T, ov.T > min_ov, score, ign_gt, ign_dt, thresholds)
    left = keep & (ign_dt == 0)[None, :] & ~assigned
    if dc_max is not None:
        left &= ~(dc_max > min_ov)[None, :]
    sim = np.zeros(len(thresholds), np.float64)
    for g in range(picked.shape[0] if compute_aos else 0):   # a Python loop: np.sum's pairwise order changes the last bits
        hit = picked[g] >= 0
        sim[hit] += (1.0 + np.cos(float(gt_alpha[g]) - dt_alpha[picked[g][hit]].astype(np.float64))) / 2.0
    return tp, left.sum(axis=1).astype(np.int64), fn, sim


def kitti_eval_numpy(gt_annos, dt_annos, class_names, PR_detail_dict=None, bev_overlap=None, stages=False):
    """The contract of ``kitti_eval``, stated once: the reference's steps with fp64 geometry (``bev_overlap(a, b)``: the intersection
    area of two BEV rectangles, default the package's exact convex clipping) and fp32 scores.  -> (result_str, ret_dict), with
    ``stages`` also a dict of the intermediate results: overlaps / dc_max (per frame, (3, D, G) / (D) fp64), matched (K, NG) fp32,
    thresholds (K, 41) fp32, n_thresholds (K), pr_counts (K, 41, 3) int64, pr_sim (K, 41) fp64, precision / recall / aos
    (3, C, 3, 2, 41), compute_aos, clean (``kitti_clean_data``)."""
    from pcdet.models.roi_heads import proposal_targets as pt
    bev_overlap = bev_overlap or pt.exact_bev_overlap
    classes = kitti_class_ints(class_names)
    compute_aos = kitti_compute_aos(dt_annos)
    cd = kitti_clean_data(gt_annos, dt_annos, classes)
    F, C = len(gt_annos), len(classes)
    go, do = cd['gt_off'], cd['dt_off']
    NG = int(go[-1])
    gt, dt = kitti_geometry(gt_annos, False), kitti_geometry(dt_annos, True)
    score = dt['score'].astype(np.float32)
    fr = lambda t, off, f: {k: v[off[f]:off[f + 1]] for k, v in t.items()}      # noqa: E731
    overlaps, dc_maxes = [], []
    for f in range(F):
        g = fr(gt, go, f)
        o, d = kitti_statement_overlaps(g, fr(dt, do, f), g['bbox'][cd['dc_rows'][go[f]:go[f + 1]]], bev_overlap)
        overlaps.append(o), dc_maxes.append(d.max(axis=1) if d.shape[1] else np.zeros(d.shape[0]))
    combo_cl, combo_metric, combo_min, combo_ngt = kitti_combos(classes, cd['num_valid'])
    K, pts = len(combo_cl), KITTI_SAMPLE_PTS
    ig, idt = cd['ignored_gt'].reshape(C * 3, -1), cd['ignored_dt'].reshape(C * 3, -1)
    matched = np.full((K, NG), -np.inf, np.float32)
    thresholds, n_thr = np.zeros((K, pts), np.float32), np.zeros(K, np.int64)
    pr_counts, pr_sim = np.zeros((K, pts, 3), np.int64), np.zeros((K, pts), np.float64)
    for k in range(K):
        cl, m, mn = combo_cl[k], combo_metric[k], combo_min[k]
        for f in range(F):
            matched[k, go[f]:go[f + 1]] = _first_pass(overlaps[f][m].T > mn, score[do[f]:do[f + 1]], ig[cl, go[f]:go[f + 1]],
                                                      idt[cl, do[f]:do[f + 1]], KITTI_NO_DETECTION)
        tps = np.sort(matched[k][matched[k] > -np.inf])[::-1]
        th = kitti_get_thresholds(tps, int(combo_ngt[k]))
        n_thr[k] = len(th)
        thresholds[k, :len(th)] = th
        for f in range(F):
            tp, fp, fn, sim = _kitti_second_pass(
                overlaps[f][m], score[do[f]:do[f + 1]], gt['alpha'][go[f]:go[f + 1]], dt['alpha'][do[f]:do[f + 1]], ig[cl, go[f]:go[f + 1]],
                idt[cl, do[f]:do[f + 1]], dc_maxes[f] if m == 0 else None, mn, th, compute_aos and m == 0)
            n = len(th)
            pr_counts[k, :n, 0] += tp
            pr_counts[k, :n, 1] += fp
            pr_counts[k, :n, 2] += fn
            pr_sim[k, :n] += sim
    precision, recall, aos = kitti_curves(n_thr, pr_counts, pr_sim, C, compute_aos)
    result, ret = kitti_format_result(classes, precision, aos, compute_aos, PR_detail_dict)
    if not stages:
        return result, ret
    return result, ret, dict(overlaps=overlaps, dc_max=dc_maxes, matched=matched, thresholds=thresholds, n_thresholds=n_thr, pr_counts=pr_counts,
                             pr_sim=pr_sim, precision=precision, recall=recall, aos=aos, compute_aos=compute_aos, clean=cd)


class _StagedEval:
    """The device run that ``KittiEval`` and ``OnceEval`` share: per-frame limits and pair offsets, uploads and allocations on
    ``self.device``, and the two calls of the entry point (``self._call``, the subclass's argument list) with the descending sort of
    the first pass's scores between them."""

    def _frames(self, who, max_rows, gt_off, pred_off, pred_rows):
        for what, off in (("GT rows", gt_off), (pred_rows, pred_off)):
            if self.F and int(np.diff(off).max()) > max_rows:
                raise ValueError(f"{who}: a frame with {int(np.diff(off).max())} {what} (at most {max_rows})")
        self.pair_off = _offsets(np.diff(gt_off) * np.diff(pred_off))
        self.NG, self.ND, self.NP = int(gt_off[-1]), int(pred_off[-1]), int(self.pair_off[-1])

    def _up(self, a, t):
        return torch.from_numpy(np.ascontiguousarray(a, t)).to(self.device)

    def _empty(self, *shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=self.device)

    def _run(self, L, workspace_bytes):
        with torch.cuda.device(self.device):
            ws_bytes = workspace_bytes(self.F, self.K)
            ws = self._empty(max(ws_bytes, 1), dtype=torch.uint8)
            self._call(L, 1, None, None, 0)
            self._sorted = torch.sort(self._matched, dim=1, descending=True).values.contiguous()
            self._call(L, 2, self._sorted, ws, ws_bytes)


class KittiEval(_StagedEval):
    """The stages of ``kitti_eval`` as device tensors (csrc/kitti_eval.hip: five launches and one ``torch.sort`` between the two
    calls; no host read until ``curves``).  Geometry, boxes, alpha and SCORES are uploaded as fp32: scores are compared as fp32 values
    (two scores that differ only beyond fp32 are a tie, and the lowest detection index wins it, as the reference's strict ``>`` does
    for equal scores); an overlap is an fp32 value that is widened to fp64 against ``min_overlap``.  The per-box flags come from
    ``kitti_clean_data`` on the host, on the annos' own dtypes.  ``dt_annos`` may be a ``KittiDetections`` record: the
    detection arrays and their flags are then the record's device tensors, and the host runs the GT half only."""

    def __init__(self, gt_annos, dt_annos, class_names, device="cuda"):
        from . import lib as L
        device = torch.device(device)
        if device.type != "cuda":
            raise NotImplementedError("kitti_eval: CPU device (the statistics are computed in libgdmae_hip.so, no CPU fallback; "
                                      "kitti_eval_numpy is the CPU path)")
        self.classes = kitti_class_ints(class_names)
        record = dt_annos if isinstance(dt_annos, KittiDetections) else None
        if record is not None:
            # the detection side stays on the device: the record's tensors, its flags and the host copy of its offsets
            if len(gt_annos) != record.F:
                raise ValueError(f"kitti_eval: {len(gt_annos)} GT annos and {record.F} detection frames")
            device = record.device
            done = record.finish(self.classes)
            self.compute_aos = record.compute_aos()
            cd = self.clean = dict(kitti_clean_gt(gt_annos, self.classes), dt_off=done['dt_off'], ignored_dt=None)
        else:
            self.compute_aos = kitti_compute_aos(dt_annos)
            cd = self.clean = kitti_clean_data(gt_annos, dt_annos, self.classes)
        self.F, self.C, self.device = len(gt_annos), len(self.classes), device
        go, do = cd['gt_off'], cd['dt_off']
        self._frames("kitti_eval", KITTI_MAX_ROWS, go, do, "detections")
        gt = kitti_geometry(gt_annos, False)
        cl, me, mn, ng = kitti_combos(self.classes, cd['num_valid'])
        self.K = len(cl)
        self._host = [np.ascontiguousarray(o, np.int32) for o in (go, do, cd['dc_off'])]          # kept alive: read by the entry point
        up, e, f32 = self._up, self._empty, np.float32
        if record is not None:
            dt_side = [done['bbox'], done['geo'], done['alpha'], done['score']]
            ignored_dt = done['ignored_dt']
        else:
            dt = kitti_geometry(dt_annos, True)
            dt_side = [up(dt['bbox'], f32), up(dt['geo'], f32), up(dt['alpha'], f32), up(dt['score'], f32)]
            ignored_dt = up(cd['ignored_dt'], np.int8)
        self._in = [up(o, np.int32) for o in self._host] + [up(self.pair_off, np.int64)] + [
            up(gt['bbox'], f32), up(gt['geo'], f32), up(gt['alpha'], f32)] + dt_side + [
            up(gt['bbox'][cd['dc_rows']], f32), up(cd['ignored_gt'], np.int8), ignored_dt,
            up(cl, np.int32), up(me, np.int32), up(mn, np.float64), up(ng, np.int32)]
        self._overlaps, self._dc_max, self._matched = e(3, self.NP), e(self.ND), e(self.K, self.NG)
        self._thresholds, self._n_thr = e(self.K, KITTI_SAMPLE_PTS), e(self.K, dtype=torch.int32)
        self._pr_counts, self._pr_sim = e(self.K, KITTI_SAMPLE_PTS, 3, dtype=torch.int64), e(self.K, KITTI_SAMPLE_PTS, dtype=torch.float64)
        self._curves = None
        self._run(L, L.load().gdmae_kitti_eval_workspace_bytes)

    def _call(self, L, stage, sorted_scores, ws, ws_bytes):
        hp = lambda a: a.ctypes.data      # noqa: E731
        L.call("gdmae_kitti_eval", stage, self.F, self.K, *[hp(h) for h in self._host], *[L.ptr(t) for t in self._in], int(self.compute_aos),
               L.ptr(self._overlaps), L.ptr(self._dc_max), L.ptr(self._matched), L.ptr(sorted_scores), L.ptr(self._thresholds),
               L.ptr(self._n_thr), L.ptr(self._pr_counts), L.ptr(self._pr_sim), L.ptr(ws), ws_bytes, L.stream())

    def overlaps(self):
        """-> (overlaps (3, NP) fp32: bbox, bev, 3d, per frame GT-major from ``pair_off[f]``; dc_max (ND) fp32).  Device tensors."""
        return self._overlaps, self._dc_max

    def frame_overlaps(self, f):
        """numpy (3, D_f, G_f) of frame f, the layout of the statement (a host read: for tests and analysis)."""
        G, D = (int(self.clean[k][f + 1] - self.clean[k][f]) for k in ('gt_off', 'dt_off'))
        return self._overlaps[:, int(self.pair_off[f]):int(self.pair_off[f + 1])].cpu().numpy().reshape(3, G, D).transpose(0, 2, 1)

    def matched_scores(self):
        """(K, NG) fp32: the score of the first pass's true positive per (combo, GT row), -inf elsewhere."""
        return self._matched

    def thresholds(self):
        """-> (thresholds (K, 41) fp32, 0 behind the count; counts (K) int32)."""
        return self._thresholds, self._n_thr

    def pr(self):
        """-> (tp / fp / fn (K, 41, 3) int64, similarity sums (K, 41) fp64)."""
        return self._pr_counts, self._pr_sim

    def curves(self):
        """-> precision, recall, aos as (metric, class, 3, 2, 41) fp64 numpy arrays.  The ONE host read (cached)."""
        if self._curves is None:
            pts = KITTI_SAMPLE_PTS
            packed = torch.cat([self._n_thr.double(), self._pr_counts.double().reshape(-1), self._pr_sim.reshape(-1)]).cpu().numpy()
            n_thr = packed[:self.K].astype(np.int64)
            counts = packed[self.K:self.K * (1 + 3 * pts)].astype(np.int64).reshape(self.K, pts, 3)
            self._curves = kitti_curves(n_thr, counts, packed[self.K * (1 + 3 * pts):].reshape(self.K, pts), self.C, self.compute_aos)
        return self._curves


def kitti_eval(gt_annos, dt_annos, class_names, PR_detail_dict=None, device="cuda"):
    """Drop-in for the reference's ``get_official_eval_result`` on the device -> (result_str, ret_dict)."""
    ev = KittiEval(gt_annos, dt_annos, class_names, device)
    precision, _, aos = ev.curves()
    return kitti_format_result(ev.classes, precision, aos, ev.compute_aos, PR_detail_dict)


# ------------------------------------------------------------------------------------------------------------------------------------
# KITTI annos of the detections (reference KittiDataset.generate_prediction_dicts)
#
#     det = KittiDetections(class_names, device)                      # a padded device store, `rows` rows per frame
#     for batch_dict in loader:
#         det.update(engine.detect(batch_dict), batch_dict)           # device copies and one small H2D copy of the calibration
#     result_str, ret_dict = kitti_eval(gt_annos, det, class_names)   # ONE read of the per-frame counts, ONE gdmae_kitti_annos launch
#     det.to_annos()                                                  # the reference's list of dicts (one more read)
# ------------------------------------------------------------------------------------------------------------------------------------
KITTI_CALIB_FLOATS = 36                # P2 (3, 4), R0 (3, 3), V2C (3, 4), image height, image width, one pad
KITTI_MAX_NAMES = 16                   # csrc/kitti_annos.hip: entries of the label -> class map
KITTI_LABEL_LINE = '%s -1 -1 %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f'


def _calib_matrices(calib):
    """calib: an object with P2 / R0 / V2C (the reference's ``Calibration``) or a dict with P2 / R0 / Tr_velo2cam -> fp32 arrays."""
    if isinstance(calib, dict):
        P2, R0, V2C = calib['P2'], calib['R0'], calib['Tr_velo2cam']
    else:
        P2, R0, V2C = calib.P2, calib.R0, calib.V2C
    f = lambda a, s: np.asarray(a, np.float32).reshape(s)      # noqa: E731
    return f(P2, (3, 4)), f(R0, (3, 3)), f(V2C, (3, 4))


def kitti_pack_calib(calib, image_shape=None):
    """-> (36) fp32, the row of ``gdmae_kitti_annos``; ``image_shape`` = (height, width), zeros when it is filled in on the device"""
    P2, R0, V2C = _calib_matrices(calib)
    h, w = (0, 0) if image_shape is None else (int(image_shape[0]), int(image_shape[1]))
    return np.concatenate([P2.reshape(-1), R0.reshape(-1), V2C.reshape(-1), np.array([h, w, 0], np.float32)]).astype(np.float32)


def kitti_annos_template(n=0):
    """the reference's ``get_template_prediction``"""
    return {'name': np.zeros(n), 'truncated': np.zeros(n), 'occluded': np.zeros(n), 'alpha': np.zeros(n), 'bbox': np.zeros([n, 4]),
            'dimensions': np.zeros([n, 3]), 'location': np.zeros([n, 3]), 'rotation_y': np.zeros(n), 'score': np.zeros(n),
            'boxes_lidar': np.zeros([n, 7])}


def _host(t, dtype):
    return np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype)


def kitti_annos_numpy(pred_boxes, pred_scores, pred_labels, calib, image_shape, class_names):
    """The contract of ``gdmae_kitti_annos`` for one sample, stated once: the reference's formulas in fp64 on the fp32 inputs, every
    result rounded once to fp32.  pred_boxes (n, >= 7) lidar boxes, pred_scores (n), pred_labels (n) 1-based -> the reference's dict.
    Every sum runs left to right as written (no BLAS), which is the order of csrc/kitti_annos.hip."""
    boxes = _host(pred_boxes, np.float32)
    boxes = np.ascontiguousarray(boxes.reshape(-1, boxes.shape[-1] if boxes.ndim == 2 else 7)[:, :7])
    scores, labels = _host(pred_scores, np.float32).reshape(-1), _host(pred_labels, np.int64).reshape(-1)
    n = scores.shape[0]
    if n == 0:
        return kitti_annos_template(0)
    P, R, V = (m.astype(np.float64) for m in _calib_matrices(calib))
    b = boxes.astype(np.float64)
    x, y, z, l, w, h, heading = (b[:, i] for i in range(7))           # dimensions (dx, dz, dy) are the reference's l, h, w
    zb = z - h / 2.0
    cam = [V[i, 0] * x + V[i, 1] * y + V[i, 2] * zb + V[i, 3] for i in range(3)]
    loc = [R[i, 0] * cam[0] + R[i, 1] * cam[1] + R[i, 2] * cam[2] for i in range(3)]
    ry = -heading - np.pi / 2.0
    c, s = np.cos(ry), np.sin(ry)
    us, vs = [], []
    with np.errstate(divide='ignore', invalid='ignore'):
        for k in range(8):
            xc = (l if (k & 3) < 2 else -l) / 2.0
            zc = (w if (k & 3) in (0, 3) else -w) / 2.0
            yc = 0.0 * h if k < 4 else -h
            X, Y, Z = loc[0] + (xc * c + zc * s), loc[1] + yc, loc[2] + (-xc * s + zc * c)
            us.append((P[0, 0] * X + P[0, 1] * Y + P[0, 2] * Z + P[0, 3]) / Z)        # divided by the corner's rect z, as the reference does
            vs.append((P[1, 0] * X + P[1, 1] * Y + P[1, 2] * Z + P[1, 3]) / Z)
    us, vs = np.stack(us, axis=1), np.stack(vs, axis=1)
    xmax, ymax = float(int(image_shape[1]) - 1), float(int(image_shape[0]) - 1)
    clip = lambda v, hi: np.minimum(np.maximum(v, 0.0), hi)      # noqa: E731
    bbox = np.stack([clip(us.min(axis=1), xmax), clip(vs.min(axis=1), ymax), clip(us.max(axis=1), xmax), clip(vs.max(axis=1), ymax)], axis=1)
    f32 = np.float32
    out = kitti_annos_template(n)
    out['name'] = np.array(class_names)[labels - 1]
    out['alpha'] = (-np.arctan2(-y, x) + ry).astype(f32)
    out['bbox'] = bbox.astype(f32)
    out['dimensions'] = np.stack([boxes[:, 3], boxes[:, 5], boxes[:, 4]], axis=1)
    out['location'] = np.stack(loc, axis=1).astype(f32)
    out['rotation_y'] = ry.astype(f32)
    out['score'] = scores
    out['boxes_lidar'] = boxes
    return out


def kitti_class_map(class_names):
    """label - 1 -> KITTI class int as ``kitti_clean_data`` compares names (lower case); -1 for a name that is no KITTI class"""
    lower = [c.lower() for c in KITTI_CLASS_NAMES]
    return [lower.index(str(n).lower()) if str(n).lower() in lower else -1 for n in class_names]


def kitti_label_lines(anno):
    """the lines of the reference's label file for one anno dict"""
    bbox, loc, dims = anno['bbox'], anno['location'], anno['dimensions']
    return [KITTI_LABEL_LINE % (anno['name'][i], anno['alpha'][i], bbox[i][0], bbox[i][1], bbox[i][2], bbox[i][3], dims[i][1], dims[i][2],
                                dims[i][0], loc[i][0], loc[i][1], loc[i][2], anno['rotation_y'][i], anno['score'][i]) for i in range(len(bbox))]


def _write_label_file(output_path, anno):
    import os
    with open(os.path.join(str(output_path), '%s.txt' % anno['frame_id']), 'w') as f:
        for line in kitti_label_lines(anno):
            print(line, file=f)


def kitti_annos_launch(boxes, scores, labels, num, calib, dt_off, n_det, class_map, classes, out=None):
    """One ``gdmae_kitti_annos`` launch on device tensors in the layout of ``detect``: boxes (F, rows, >= 7) fp32, scores (F, rows)
    fp32, labels (F, rows) int64, num (F) int32, calib (F, 36) fp32, dt_off (F + 1) int32 -> dict of the compact outputs (``out``: the
    tensors to write into).  No host read."""
    from . import lib as L
    F, rows, cols = boxes.shape
    if rows > KITTI_MAX_ROWS or rows < 1:
        raise ValueError(f"kitti_annos: rows {rows} (1 .. {KITTI_MAX_ROWS})")
    if not 1 <= len(class_map) <= KITTI_MAX_NAMES or not 1 <= len(classes) <= len(KITTI_CLASS_NAMES):
        raise ValueError(f"kitti_annos: {len(class_map)} class names (1 .. {KITTI_MAX_NAMES}), {len(classes)} evaluated classes (1 .. 6)")
    if tuple(scores.shape) != (F, rows) or tuple(labels.shape) != (F, rows) or tuple(num.shape) != (F,) or tuple(calib.shape) != (
            F, KITTI_CALIB_FLOATS) or tuple(dt_off.shape) != (F + 1,) or cols < 7:
        raise ValueError("kitti_annos: boxes (F, rows, >= 7), scores / labels (F, rows), num (F), calib (F, 36), dt_off (F + 1)")
    for t, dtype in ((boxes, torch.float32), (scores, torch.float32), (labels, torch.int64), (num, torch.int32), (calib, torch.float32),
                     (dt_off, torch.int32)):
        if t.dtype != dtype or not t.is_cuda:
            raise ValueError("kitti_annos: fp32 boxes / scores / calib, int64 labels, int32 num / dt_off, all on the device")
        if not t.is_contiguous():                                                # the entry reads rows of boxes.shape[2] floats
            raise ValueError("kitti_annos: a tensor that is not contiguous (a column slice of wider boxes, a strided view)")
    dev, C = boxes.device, len(classes)
    if out is None:
        e = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device=dev)      # noqa: E731
        out = dict(bbox=e(n_det, 4), geo=e(n_det, 7), alpha=e(n_det), score=e(n_det), ignored_dt=e(C, 3, n_det, dtype=torch.int8),
                   boxes_lidar=e(n_det, 7), label=e(n_det, dtype=torch.int32))
    if F and n_det:
        with torch.cuda.device(dev):
            L.call("gdmae_kitti_annos", L.ptr(boxes), cols, L.ptr(scores), L.ptr(labels), L.ptr(num), L.ptr(calib), L.ptr(dt_off), F, rows,
                   n_det, L.host_i32(class_map), len(class_map), L.host_i32(classes), C, L.ptr(out['bbox']), L.ptr(out['geo']),
                   L.ptr(out['alpha']), L.ptr(out['score']), L.ptr(out['ignored_dt']), L.ptr(out['boxes_lidar']), L.ptr(out['label']),
                   L.stream())
    return out


class _DetectionStore:
    """What ``KittiDetections`` and ``OnceDetections`` share: the padded device store (``rows`` rows per frame, the frames grown by
    doubling) of boxes (cap, rows, 7) fp32, scores (cap, rows) fp32, labels (cap, rows) int64, num (cap) int32 and the subclass's
    ``EXTRA`` per-frame fp32 tensors (name -> width).  A subclass names its row limit, the two hints of its CPU refusals, its
    allocator and ``_invalidate`` (what it caches of the store's content)."""
    MAX_ROWS, CPU_DEVICE, CPU_TENSORS, EXTRA = None, "", "", {}
    ALLOC = staticmethod(torch.empty)

    def __init__(self, class_names, device, rows):
        self._who = type(self).__name__
        self.class_names = [str(c) for c in class_names]
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NotImplementedError(f"{self._who}: CPU device ({self.CPU_DEVICE})")
        if not 1 <= rows <= self.MAX_ROWS:
            raise ValueError(f"{self._who}: rows {rows} (1 .. {self.MAX_ROWS})")
        self.rows, self.F, self.frame_ids = int(rows), 0, []
        self._cap, self._store = 0, None

    def _reserve(self, need):
        if need <= self._cap:
            return
        cap = self._cap
        while cap < need:
            cap = max(2 * cap, 1)
        e = lambda *s, dtype=torch.float32: self.ALLOC(*s, dtype=dtype, device=self.device)      # noqa: E731
        new = dict(boxes=e(cap, self.rows, 7), scores=e(cap, self.rows), labels=e(cap, self.rows, dtype=torch.int64),
                   num=e(cap, dtype=torch.int32), **{k: e(cap, width) for k, width in self.EXTRA.items()})
        if self._store is not None and self.F:
            for k, t in new.items():
                t[:self.F].copy_(self._store[k][:self.F])
        self._cap, self._store = cap, new

    def widen(self, rows):
        """Reallocates the store with ``rows`` (> the present) rows per frame and copies what it holds: device copies, no host read."""
        if not self.rows < rows <= self.MAX_ROWS:
            raise ValueError(f"{self._who}.widen: rows {rows} ({self.rows + 1} .. {self.MAX_ROWS})")
        old, old_rows = self._store, self.rows
        self.rows, self._cap, self._store = int(rows), 0, None
        self._reserve(max(self.F, 1 if old is None else old['num'].shape[0]))
        if old is not None and self.F:
            for k in ('boxes', 'scores', 'labels'):
                self._store[k][:self.F, :old_rows].copy_(old[k][:self.F])
            for k in ('num', *self.EXTRA):
                self._store[k][:self.F].copy_(old[k][:self.F])
        self._invalidate()

    def _checked(self, out):
        """the padded dict of ``detect`` -> (boxes, scores, labels, num) after the shape and device checks of ``update``"""
        boxes, scores, labels, num = out['pred_boxes'], out['pred_scores'], out['pred_labels'], out['num']
        if boxes.dim() != 3 or boxes.shape[2] < 7 or tuple(scores.shape) != tuple(boxes.shape[:2]) or tuple(labels.shape) != tuple(
                boxes.shape[:2]) or tuple(num.shape) != (boxes.shape[0],):
            raise ValueError(f"{self._who}.update: pred_boxes (B, n, >= 7), pred_scores / pred_labels (B, n), num (B)")
        if scores.shape[1] > self.rows:
            raise ValueError(f"{self._who}.update: n {scores.shape[1]} rows per sample in a store of rows {self.rows}")
        if not all(t.is_cuda for t in (boxes, scores, labels, num)):
            raise NotImplementedError(f"{self._who}.update: CPU tensors ({self.CPU_TENSORS})")
        return boxes, scores, labels, num

    def _append(self, boxes, scores, labels, num, ids):
        """copies the checked batch behind the frames held -> the slice of its frames in the store"""
        B, n = scores.shape
        self._reserve(self.F + B)
        s, at = self._store, slice(self.F, self.F + B)
        if n:
            s['boxes'][at, :n].copy_(boxes[..., :7])
            s['scores'][at, :n].copy_(scores)
            s['labels'][at, :n].copy_(labels)
        s['num'][at].copy_(num)
        self.frame_ids += list(ids)
        self.F += B
        self._invalidate()
        return at

    def _counts_in_range(self, counts):
        if counts.size and (counts.min() < 0 or counts.max() > self.rows):
            raise ValueError(f"{self._who}: a frame count outside 0 .. {self.rows}")


class KittiDetections(_DetectionStore):
    """The detections of an evaluation loop as a padded device store (``rows`` rows per frame, grown by doubling) and, after
    ``finish``, as the compact device tensors ``KittiEval`` reads.  ``update`` makes no host read and no launch of this library;
    ``finish`` makes the one host read (the per-frame counts) and the one ``gdmae_kitti_annos`` launch."""

    MAX_ROWS, EXTRA = KITTI_MAX_ROWS, {'calib': KITTI_CALIB_FLOATS}
    CPU_DEVICE = "the annos are computed in libgdmae_hip.so, no CPU fallback; kitti_annos_numpy is the CPU path"
    CPU_TENSORS = "no CPU fallback; kitti_annos_numpy is the CPU path"

    def __init__(self, class_names, device, rows=500, frames=0):
        super().__init__(class_names, device, rows)
        if not 1 <= len(self.class_names) <= KITTI_MAX_NAMES:
            raise ValueError(f"KittiDetections: {len(self.class_names)} class names (1 .. {KITTI_MAX_NAMES})")
        self.class_map = kitti_class_map(self.class_names)
        self._pinned = []
        self._host_num = []                      # per update: the counts when the caller knows them on the host, else None
        self._reserve(int(frames))
        self._invalidate()

    def _invalidate(self):
        self._counts, self._first, self._done, self._annos, self._aos = None, None, {}, None, None

    def update(self, out, batch_dict, host_num=None):
        """out: the padded dict of ``detect`` (pred_boxes (B, n, >= 7), pred_scores (B, n), pred_labels (B, n), num (B)); batch_dict:
        ``calib`` (B calibrations), ``image_shape`` (B, 2) = (height, width), ``frame_id`` (B).  No host read."""
        boxes, scores, labels, num = self._checked(out)
        B = scores.shape[0]
        calibs, shapes, ids = batch_dict['calib'], batch_dict['image_shape'], batch_dict['frame_id']
        if len(calibs) != B or len(shapes) != B or len(ids) != B:
            raise ValueError(f"KittiDetections.update: {B} samples, {len(calibs)} calibrations, {len(shapes)} image shapes, {len(ids)} frame ids")
        on_device = isinstance(shapes, torch.Tensor) and shapes.is_cuda          # an image_shape already uploaded is not read back
        packed = np.stack([kitti_pack_calib(calibs[b], None if on_device else _host(shapes[b], np.int64)) for b in range(B)])
        pinned = torch.from_numpy(packed).pin_memory()                           # one small H2D copy that does not wait for the device
        at = self._append(boxes, scores, labels, num, ids)
        calib = self._store['calib']
        calib[at].copy_(pinned, non_blocking=True)
        self._pinned.append(pinned)                                              # alive until the copy has run (``counts`` waits)
        if on_device:
            calib[at, 33:35].copy_(shapes[:, :2])
        self._host_num.append(None if host_num is None else [int(v) for v in host_num])

    def _alpha_row(self, row):
        x, y, heading = float(np.float32(row[0])), float(np.float32(row[1])), float(np.float32(row[6]))
        return -np.arctan2(-y, x) + (-heading - np.pi / 2.0)

    def counts(self):
        """(F) int64 per-frame counts on the host: THE host read (cached).  The same read brings the lidar box of the first detection,
        from which ``compute_aos`` is decided."""
        if self._counts is None:
            s, F = self._store, self.F
            if F == 0:
                self._counts, self._first = np.zeros(0, np.int64), None
            elif all(h is not None for h in self._host_num):
                self._counts = np.array([v for h in self._host_num for v in h], np.int64)
            else:
                num = s['num'][:F]
                first = (num > 0).to(torch.int32).argmax().reshape(1)            # selected on the device: indexing with it would read it
                packed = torch.cat([num.double(), s['boxes'][:F, 0].index_select(0, first)[0].double()]).cpu().numpy()
                self._counts = packed[:F].astype(np.int64)
                self._first = packed[F:]
                self._pinned = []
            self._counts_in_range(self._counts)
        return self._counts

    def finish(self, classes=None):
        """-> dict: dt_off (F + 1) int64 on the host; on the device bbox (ND, 4), geo (ND, 7), alpha (ND), score (ND), ignored_dt
        (C, 3, ND) int8 for the evaluated KITTI class ints ``classes`` (default: the record's own names that are KITTI classes),
        boxes_lidar (ND, 7), label (ND) int32.  Cached per class list until the next ``update``."""
        if classes is None:
            classes = [c for c in dict.fromkeys(self.class_map) if c >= 0] or [0]
        key = tuple(int(c) for c in classes)
        if key not in self._done:
            dt_off = _offsets(self.counts())
            nd = int(dt_off[-1])
            s, F = self._store, self.F
            pinned = torch.from_numpy(dt_off.astype(np.int32)).pin_memory()             # an upload that does not wait for the device
            off_dev = torch.empty(F + 1, dtype=torch.int32, device=self.device)
            off_dev.copy_(pinned, non_blocking=True)
            if F:
                out = kitti_annos_launch(s['boxes'][:F], s['scores'][:F], s['labels'][:F], s['num'][:F], s['calib'][:F], off_dev, nd,
                                         self.class_map, list(key))
            else:
                e = lambda *sh, dtype=torch.float32: torch.empty(*sh, dtype=dtype, device=self.device)      # noqa: E731
                out = dict(bbox=e(0, 4), geo=e(0, 7), alpha=e(0), score=e(0), ignored_dt=e(len(key), 3, 0, dtype=torch.int8),
                           boxes_lidar=e(0, 7), label=e(0, dtype=torch.int32))
            self._done[key] = dict(out, dt_off=dt_off, dt_off_device=off_dev, dt_off_pinned=pinned)
        return self._done[key]

    def compute_aos(self):
        """``kitti_compute_aos`` on ``to_annos()``: the first detection's ``alpha != -10``.  Decided on the host from the row that
        came with the counts (the statement's fp64 value; the device's fp32 value is within an ulp of its rounding), and only when that
        value is within 1e-5 of -10 by reading the device's own."""
        if self._aos is None:
            counts = self.counts()
            nz = np.nonzero(counts)[0]
            if nz.size == 0:
                self._aos = False
            else:
                if self._first is None:
                    self._first = self._store['boxes'][int(nz[0]), 0].double().cpu().numpy()
                a = self._alpha_row(self._first)
                self._aos = bool(self.finish()['alpha'][0].item() != -10) if abs(a + 10.0) < 1e-5 else True
        return self._aos

    def to_annos(self):
        """The reference's list of anno dicts (fp32 arrays, ``frame_id``; a frame without detections: the empty template).  One more
        host read (cached)."""
        if self._annos is None:
            d = self.finish()
            off = d['dt_off']
            flat = torch.cat([d['bbox'], d['geo'], d['alpha'][:, None], d['score'][:, None], d['boxes_lidar'],
                              d['label'].to(torch.float32)[:, None]], dim=1).cpu().numpy()          # labels are small integers: exact in fp32
            self._pinned = []
            label = flat[:, 20].astype(np.int64)
            names = np.array(self.class_names)
            annos = []
            for f in range(self.F):
                a, b = int(off[f]), int(off[f + 1])
                anno = kitti_annos_template(b - a)
                if b > a:
                    r = flat[a:b]
                    anno.update(name=names[label[a:b] - 1], alpha=r[:, 11].copy(), bbox=r[:, 0:4].copy(), dimensions=r[:, 7:10].copy(),
                                location=r[:, 4:7].copy(), rotation_y=r[:, 10].copy(), score=r[:, 12].copy(), boxes_lidar=r[:, 13:20].copy())
                anno['frame_id'] = self.frame_ids[f]
                annos.append(anno)
            self._annos = annos
        return self._annos

    def write_label_files(self, output_path):
        """One ``<frame_id>.txt`` per frame in the reference's format."""
        for anno in self.to_annos():
            _write_label_file(output_path, anno)


def kitti_prediction_dicts(batch_dict, pred_dicts, class_names, output_path=None):
    """Drop-in for the reference's ``KittiDataset.generate_prediction_dicts``: ``pred_dicts`` is the per-sample list of pred_boxes
    (n, >= 7), pred_scores (n), pred_labels (n).  Device tensors are padded and go through one ``gdmae_kitti_annos`` launch and one
    read (the counts are the tensors' shapes); CPU tensors go through ``kitti_annos_numpy``."""
    if pred_dicts and all(isinstance(d['pred_scores'], torch.Tensor) and d['pred_scores'].is_cuda for d in pred_dicts):
        counts = [int(d['pred_scores'].shape[0]) for d in pred_dicts]
        n, B, dev = max(counts), len(pred_dicts), pred_dicts[0]['pred_scores'].device
        if n > KITTI_MAX_ROWS:
            raise ValueError(f"kitti_prediction_dicts: a sample with {n} detections (at most {KITTI_MAX_ROWS})")
        out = {'pred_boxes': torch.zeros(B, n, 7, device=dev), 'pred_scores': torch.zeros(B, n, device=dev),
               'pred_labels': torch.zeros(B, n, dtype=torch.int64, device=dev), 'num': torch.tensor(counts, dtype=torch.int32).to(dev)}
        for b, d in enumerate(pred_dicts):
            if counts[b]:
                out['pred_boxes'][b, :counts[b]] = d['pred_boxes'][:, :7]
                out['pred_scores'][b, :counts[b]] = d['pred_scores']
                out['pred_labels'][b, :counts[b]] = d['pred_labels']
        det = KittiDetections(class_names, dev, rows=max(n, 1), frames=B)
        det.update(out, batch_dict, host_num=counts)
        annos = det.to_annos()
    else:
        annos = []
        for b, d in enumerate(pred_dicts):
            anno = kitti_annos_numpy(d['pred_boxes'], d['pred_scores'], d['pred_labels'], batch_dict['calib'][b],
                                     _host(batch_dict['image_shape'][b], np.int64), class_names)
            anno['frame_id'] = batch_dict['frame_id'][b]
            annos.append(anno)
    if output_path is not None:
        for anno in annos:
            _write_label_file(output_path, anno)
    return annos


def evaluate_kitti(engine, batches, gt_annos, class_names, keep_annos=False):
    """The loop of ``evaluate`` with a ``KittiDetections`` record, then ``kitti_eval`` from the record -> (result_str, ret_dict, the
    reference's anno list or None).  Between ``detect`` and the AP table the host reads the per-frame counts once.  ``engine`` is
    anything with ``detect(batch_dict)`` (all three engines).  The store starts with 500 rows per frame (KITTI's ``NMS_POST_MAXSIZE``) or
    the first batch's width if that is larger, and is widened on the device when a later batch is wider; beyond 1024 rows
    ``KittiDetections`` refuses by name."""
    det = None
    for bd in batches:
        out = engine.detect(bd)
        n = int(out['pred_scores'].shape[1])
        if det is None:
            det = KittiDetections(class_names, out['pred_scores'].device, rows=max(500, n))
        elif n > det.rows:
            det.widen(n)
        det.update(out, bd)
    if det is None:
        raise ValueError("evaluate_kitti: no batches")
    result, ret = kitti_eval(gt_annos, det, class_names)
    return result, ret, (det.to_annos() if keep_annos else None)


# ------------------------------------------------------------------------------------------------------------------------------------
# The ONCE AP table (reference pcdet/datasets/once/once_eval/evaluation.py ``get_evaluation_results``)
#
#     ret_str, ret_dict = once_eval(gt_annos, pred_annos, classes)                   # libgdmae_hip.so, ONE host read
#     ret_str, ret_dict = once_eval_numpy(gt_annos, pred_annos, classes)             # the statement: fp64 geometry, numpy, CPU
#
# Annos are per-frame dicts: name (n), boxes_3d (n, 7) = (x, y, z, l, w, h, rot) in lidar coordinates, score (n) on the prediction
# side.  A "combo" is (class, distance band), index class * bands + band.
# ------------------------------------------------------------------------------------------------------------------------------------
ONCE_IOU_THRESHOLDS = {'Car': 0.7, 'Bus': 0.7, 'Truck': 0.7, 'Pedestrian': 0.3, 'Cyclist': 0.5}
ONCE_SUPERCLASS_IOU_THRESHOLDS = {'Vehicle': 0.7, 'Pedestrian': 0.3, 'Cyclist': 0.5}
ONCE_DIFFICULTY_MODES = {'Overall': ['overall'], 'Distance': ['0-30m', '30-50m', '50m-inf'],
                         'Overall&Distance': ['overall', '0-30m', '30-50m', '50m-inf']}
ONCE_MAX_ROWS = 1024                   # predictions / GT rows per frame (csrc/once_eval.hip: 16 mask bits per lane)
ONCE_MAX_PR_POINTS = 63                # num_pr_points + 1 thresholds, one lane each
ONCE_THRESHOLD_SLOTS = 64
ONCE_MAX_CODES = 32                    # name codes: the bits of an accept mask
ONCE_VEHICLE_NAMES = frozenset(('Car', 'Bus', 'Truck'))
ONCE_THRESHOLD_EPS = 1e-6              # the slack of the threshold rule's comparison


def once_classes(classes, use_superclass):
    """The evaluated classes: with ``use_superclass`` Car / Bus / Truck (all three, if any) become one leading ``Vehicle``."""
    if not use_superclass:
        return list(classes)
    given = ONCE_VEHICLE_NAMES.intersection(classes)
    assert not given or given == ONCE_VEHICLE_NAMES, "Car/Bus/Truck must all exist for vehicle detection"      # the reference's message
    return ['Vehicle'] + [c for c in classes if c not in ONCE_VEHICLE_NAMES]


def once_name_codes(classes, use_superclass):
    """-> (names: code -> name, the LAST code is "any other name"; accept (C) uint32: bit ``code`` set where a row with that code
    belongs to the evaluated class).  ``Vehicle`` under the superclass rule accepts every code but Pedestrian's and Cyclist's, the
    "other" code included; every other class accepts its own name only."""
    names = list(dict.fromkeys(['Pedestrian', 'Cyclist'] + [str(c) for c in classes]))
    if len(names) + 1 > ONCE_MAX_CODES:
        raise ValueError(f"once_eval: {len(names)} distinct class names (at most {ONCE_MAX_CODES - 1})")
    every = (1 << (len(names) + 1)) - 1
    accept = [every & ~0b11 if (use_superclass and c == 'Vehicle') else 1 << names.index(str(c)) for c in classes]
    return names, np.array(accept, np.uint32)


def _once_names(anno):
    """the ``name`` column as strings; a zero-row column may be of any dtype (the reference's empty template holds floats)"""
    name = np.asarray(anno['name']).reshape(-1)
    return name.astype(str) if name.size else np.zeros(0, dtype='<U1')


def once_codes_of(name_lists, names):
    """per-frame name arrays -> (rows) int32 codes in ``names``, ``len(names)`` for any other name"""
    flat = np.concatenate([np.zeros(0, dtype='<U1')] + list(name_lists))
    codes = np.full(flat.shape[0], len(names), np.int32)
    for i, n in enumerate(names):
        codes[flat == n] = i
    return codes


def once_boxes(annos):
    """(rows, 7) fp32: the boxes of all frames as the device compares them"""
    return _cat([np.asarray(a['boxes_3d']).reshape(-1, 7) for a in annos], 7, np.float32)


def once_band_of(boxes):
    """(n, 7) fp32 -> (n) band: 0 below 30 m, 1 below 50 m, 2 from 50 m, 3 in none; the distance in fp64 on the fp32 values"""
    b = np.asarray(boxes, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore'):
        dist = np.sqrt(b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1] + b[:, 2] * b[:, 2])
        return np.where(dist < 30, 0, np.where((dist >= 30) & (dist < 50), 1, np.where(dist >= 50, 2, 3))).astype(np.int64)


def once_flags(codes, boxes, accept, difficulty_mode):
    """-> (C, bands, n) int8: 1 outside the band (of ANY class: the reference writes the band after the class), else -1 other class,
    else 0 accepted"""
    bands = ONCE_DIFFICULTY_MODES[difficulty_mode]
    band = once_band_of(boxes)
    out = np.full((len(accept), len(bands), codes.shape[0]), -1, np.int8)
    for c, mask in enumerate(accept):
        own = ((int(mask) >> codes.astype(np.int64)) & 1).astype(bool)
        for b, tag in enumerate(bands):
            inside = np.ones_like(own) if tag == 'overall' else band == ('0-30m', '30-50m', '50m-inf').index(tag)
            out[c, b] = np.where(inside, np.where(own, 0, -1), 1)      # the band is written last in ``filter_data``: it overrides the class
    return out


def once_heading_rejected(rot_gt, rot_pred):
    """The reference's rule, literally: d = |a - b|, 2 pi - d where d >= pi, rejected where d > pi / 2 (nothing wraps beyond 2 pi)."""
    d = abs(float(rot_gt) - float(rot_pred))
    if d >= np.pi:
        d = 2 * np.pi - d
    return d > np.pi / 2


def once_statement_overlaps(gt, pred, with_heading, bev_overlap):
    """One frame: gt (G, 7), pred (P, 7) fp32 -> (G, P) fp64 3-D IoU: exact rotated intersection x clipped height overlap over the
    union; 0 for a pair whose union is 0 and, with the heading rule, for a rejected pair."""
    g64, p64 = np.asarray(gt, np.float32).astype(np.float64), np.asarray(pred, np.float32).astype(np.float64)
    out = np.zeros((g64.shape[0], p64.shape[0]), np.float64)
    turned = lambda b: [b[0], b[1], b[2], b[3], b[4], b[5], -b[6]]      # noqa: E731   rot turns clockwise in (x, y) (the reference's rbbox_to_corners)
    for i, g in enumerate(g64):
        for j, p in enumerate(p64):
            if with_heading and once_heading_rejected(g[6], p[6]):
                continue
            ih = min(g[2] + g[5] * 0.5, p[2] + p[5] * 0.5) - max(g[2] - g[5] * 0.5, p[2] - p[5] * 0.5)
            if not ih > 0:
                continue
            inter = bev_overlap(turned(g), turned(p))
            if not inter > 0:
                continue
            i3 = inter * ih
            union = g[3] * g[4] * g[5] + p[3] * p[4] * p[5] - i3
            if union != 0:
                out[i, j] = i3 / union
    return out


def once_overlaps_enough(iou, threshold):
    """the one comparison of an IoU with its class threshold: strictly above"""
    return iou > threshold


def once_get_thresholds(scores_desc, num_gt, num_pr_points):
    """The score thresholds of one combo from its true positives' scores in descending order: the fp64 operations of the reference's
    ``get_thresholds`` in its order (csrc/once_eval.hip ``k_oe_thresholds`` is the same loop).  The true positive of rank r reaches
    the recall r / num_gt.  A running level climbs in steps of 1 / num_pr_points; a rank is passed over while the middle between its
    recall and the next rank's is still below the level (the last rank never is), otherwise its score is taken once for the level
    and again for every further step that stays within ``ONCE_THRESHOLD_EPS`` of that middle.  The count never exceeds
    ``num_pr_points + 1`` because true positives never outnumber ``num_gt``; a broken bound raises."""
    step, level, taken, ranks = 1 / num_pr_points, 0, [], len(scores_desc)
    for rank, score in enumerate(scores_desc, start=1):
        reached = rank / num_gt
        twice_middle = ((rank + 1) / num_gt if rank < ranks else reached) + reached
        if rank < ranks and twice_middle < 2 * level:
            continue
        while True:
            taken.append(score)
            level += step
            assert len(taken) <= 4 * (num_pr_points + 1), "once_eval: the threshold rule does not end"
            if not twice_middle + ONCE_THRESHOLD_EPS > 2 * level:
                break
    assert len(taken) <= num_pr_points + 1, f"once_eval: {len(taken)} thresholds for num_pr_points {num_pr_points} (at most num_pr_points + 1)"
    return taken


def once_false_positives(kept, flag_pred, assigned):
    """kept / assigned (T, P) bool, flag_pred (P) -> (T): the flag-0 predictions at or above the threshold that no GT row took"""
    return (kept & (flag_pred == 0)[None, :] & ~assigned).sum(axis=1).astype(np.int64)


def _once_second_pass(ov, enough, score, flag_gt, flag_pred, thresholds):
    """``_second_pass`` on one frame's (G, P) overlaps -> tp, fp, fn (T) int64"""
    tp, fn, keep, assigned, _ = _second_pass(ov, enough, score, flag_gt, flag_pred, thresholds)
    return tp, once_false_positives(keep, flag_pred, assigned), fn


def once_curves(n_thresholds, counts, n_classes, n_bands, num_pr_points):
    """(K) counts, (K, >= num_pr_points + 1, 3) tp / fp / fn -> precision, recall, each (C, bands, num_pr_points + 1) fp64: the
    quotients where a threshold exists, 0 behind the count, then the reverse running maximum over ``th_idx:`` with numpy's 0 / 0."""
    pts = num_pr_points + 1
    n_thresholds = np.asarray(n_thresholds).reshape(-1)
    if n_thresholds.size and int(n_thresholds.max()) > pts:
        raise AssertionError(f"once_eval: {int(n_thresholds.max())} thresholds for num_pr_points {num_pr_points} (at most num_pr_points + 1)")
    tp, fp, fn = (np.asarray(counts)[:, :pts, i].astype(np.float64) for i in range(3))
    mask = np.arange(pts)[None, :] < n_thresholds[:, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        curves = [tp / (tp + fp), tp / (tp + fn)]
    out = []
    for x in curves:
        x = np.where(mask, x, 0.0)
        x = np.maximum.accumulate(x[:, ::-1], axis=1)[:, ::-1]
        out.append(np.where(mask, x, 0.0).reshape(n_classes, n_bands, pts))
    return tuple(out)


def once_format_result(classes, precision, num_pr_points, difficulty_mode, print_ok=False):
    """precision (C, bands, num_pr_points + 1) -> (the reference's table text, its ``ret_dict``)"""
    tags = ONCE_DIFFICULTY_MODES[difficulty_mode]
    ap = np.zeros(precision.shape[:-1], np.float64)
    for column in np.moveaxis(precision[..., 1:], -1, 0):             # in index order: the sum is part of the contract's bits
        ap = ap + column
    ap = ap / num_pr_points * 100
    rows = [(str(cls), 'AP_%s' % cls, ap[c]) for c, cls in enumerate(classes)] + [('mAP', 'AP_mean', ap.mean(axis=0))]
    line = lambda head, cells: "|" + "|".join([head] + cells) + "|\n"      # noqa: E731   every cell is 12 wide, left-aligned
    text = "\n" + line(f"AP@{str(num_pr_points):<9}", [f"{tag:<12}" for tag in tags])
    ret = {}
    for head, key, values in rows:
        text += line(f"{head:<12}", [f"{v:<12.2f}" for v in values])
        ret.update({f"{key}/{tag}": v for tag, v in zip(tags, values)})
    if print_ok:
        print(text)
    return text, ret


def _once_options(classes, use_superclass, iou_thresholds, num_pr_points, difficulty_mode, n_gt, n_pred):
    if iou_thresholds is None:
        iou_thresholds = ONCE_SUPERCLASS_IOU_THRESHOLDS if use_superclass else ONCE_IOU_THRESHOLDS
    assert n_gt == n_pred, "the number of GT must match predictions"
    assert difficulty_mode in ONCE_DIFFICULTY_MODES, "difficulty mode is not supported"
    classes = once_classes(classes, use_superclass)
    return classes, np.array([float(iou_thresholds[c]) for c in classes], np.float64)


def once_eval_numpy(gt_annos, pred_annos, classes, use_superclass=True, iou_thresholds=None, num_pr_points=50,
                    difficulty_mode='Overall&Distance', ap_with_heading=True, num_parts=100, print_ok=False, stages=False,
                    bev_overlap=None):
    """The contract of ``once_eval``, stated once: the reference's steps with fp64 geometry on the fp32 values of the annos
    (``bev_overlap(a, b)``: the intersection area of two BEV rectangles, default the package's exact convex clipping) and fp32
    scores.  ``num_parts`` is accepted and ignored.  -> (ret_str, ret_dict), with ``stages`` also a dict of the intermediate results:
    overlaps (per frame (G, P) fp64), flag_gt (C, bands, NG) / flag_pred (C, bands, ND) int8, num_valid (K), matched (K, NG) fp32,
    thresholds (K, 64) fp32, n_thresholds (K), counts (K, 64, 3) int64, precision / recall (C, bands, num_pr_points + 1), gt_off,
    pred_off, classes."""
    from pcdet.models.roi_heads import proposal_targets as pt
    bev_overlap = bev_overlap or pt.exact_bev_overlap
    classes, thr = _once_options(classes, use_superclass, iou_thresholds, num_pr_points, difficulty_mode, len(gt_annos), len(pred_annos))
    names, accept = once_name_codes(classes, use_superclass)
    tags = ONCE_DIFFICULTY_MODES[difficulty_mode]
    F, C, B = len(gt_annos), len(classes), len(tags)
    gt_names, pred_names = [_once_names(a) for a in gt_annos], [_once_names(a) for a in pred_annos]
    go, po = _offsets([len(n) for n in gt_names]), _offsets([len(n) for n in pred_names])
    gt_box, pred_box = once_boxes(gt_annos), once_boxes(pred_annos)
    score = _cat([a['score'] for a in pred_annos], None, np.float32)
    flag_gt = once_flags(once_codes_of(gt_names, names), gt_box, accept, difficulty_mode)
    flag_pred = once_flags(once_codes_of(pred_names, names), pred_box, accept, difficulty_mode)
    overlaps = [once_statement_overlaps(gt_box[go[f]:go[f + 1]], pred_box[po[f]:po[f + 1]], ap_with_heading, bev_overlap)
                for f in range(F)]
    K, NG, slots = C * B, int(go[-1]), ONCE_THRESHOLD_SLOTS
    fg, fp_ = flag_gt.reshape(K, -1), flag_pred.reshape(K, -1)
    num_valid = (fg == 0).sum(axis=1).astype(np.int64)
    matched = np.full((K, NG), -np.inf, np.float32)
    thresholds, n_thr, counts = np.zeros((K, slots), np.float32), np.zeros(K, np.int64), np.zeros((K, slots, 3), np.int64)
    for k in range(K):
        mn = thr[k // B]
        enough = [once_overlaps_enough(o, mn) for o in overlaps]
        for f in range(F):
            matched[k, go[f]:go[f + 1]] = _first_pass(enough[f], score[po[f]:po[f + 1]], fg[k, go[f]:go[f + 1]], fp_[k, po[f]:po[f + 1]],
                                                      -1)                 # the reference's sentinel
        tps = np.sort(matched[k][matched[k] > -np.inf])[::-1]
        th = once_get_thresholds(tps, int(num_valid[k]), num_pr_points)
        n = n_thr[k] = len(th)
        thresholds[k, :n] = th
        for f in range(F):
            tp, fp, fn = _once_second_pass(overlaps[f], enough[f], score[po[f]:po[f + 1]], fg[k, go[f]:go[f + 1]], fp_[k, po[f]:po[f + 1]], th)
            counts[k, :n, 0] += tp
            counts[k, :n, 1] += fp
            counts[k, :n, 2] += fn
    precision, recall = once_curves(n_thr, counts, C, B, num_pr_points)
    ret_str, ret_dict = once_format_result(classes, precision, num_pr_points, difficulty_mode, print_ok)
    if not stages:
        return ret_str, ret_dict
    return ret_str, ret_dict, dict(overlaps=overlaps, flag_gt=flag_gt, flag_pred=flag_pred, num_valid=num_valid, matched=matched,
                                   thresholds=thresholds, n_thresholds=n_thr, counts=counts, precision=precision, recall=recall, gt_off=go,
                                   pred_off=po, classes=classes)


class OnceEval(_StagedEval):
    """The stages of ``once_eval`` as device tensors (csrc/once_eval.hip: five launches and one ``torch.sort`` between the two calls;
    no host read until ``curves``).  Boxes and SCORES are uploaded as fp32 and compared as fp32 values; an overlap is an fp32 value
    that is widened to fp64 against the class threshold.  The host only maps names to codes: the flags are the device's.
    ``pred_annos`` may be a ``OnceDetections`` record: the prediction side is then the record's device tensors."""

    def __init__(self, gt_annos, pred_annos, classes, device="cuda", use_superclass=True, iou_thresholds=None, num_pr_points=50,
                 difficulty_mode='Overall&Distance', ap_with_heading=True, num_parts=100, print_ok=False):
        from . import lib as L
        device = torch.device(device)
        if device.type != "cuda":
            raise NotImplementedError("once_eval: CPU device (the statistics are computed in libgdmae_hip.so, no CPU fallback; "
                                      "once_eval_numpy is the CPU path)")
        record = pred_annos if isinstance(pred_annos, OnceDetections) else None
        n_pred = record.F if record is not None else len(pred_annos)
        self.classes, thr = _once_options(classes, use_superclass, iou_thresholds, num_pr_points, difficulty_mode, len(gt_annos), n_pred)
        if not 1 <= int(num_pr_points) <= ONCE_MAX_PR_POINTS:
            raise ValueError(f"once_eval: num_pr_points {num_pr_points} (1 .. {ONCE_MAX_PR_POINTS}: one lane per threshold)")
        self.num_pr_points, self.difficulty_mode, self.print_ok = int(num_pr_points), difficulty_mode, print_ok
        self.names, accept = once_name_codes(self.classes, use_superclass)
        self.F, self.C, self.B = len(gt_annos), len(self.classes), len(ONCE_DIFFICULTY_MODES[difficulty_mode])
        self.K = self.C * self.B
        gt_names = [_once_names(a) for a in gt_annos]
        go = _offsets([len(n) for n in gt_names])
        if record is not None:
            device = record.device
            po = _offsets(record.counts())
        else:
            pred_names = [_once_names(a) for a in pred_annos]
            po = _offsets([len(n) for n in pred_names])
        self.gt_off, self.pred_off, self.device = go, po, device
        self._frames("once_eval", ONCE_MAX_ROWS, go, po, "predictions")
        self._host = [np.ascontiguousarray(o, np.int32) for o in (go, po)]                    # kept alive: read by the entry point
        up, e = self._up, self._empty
        if record is not None:
            pred_side = list(record.compact(self.names))
        else:
            pred_side = [up(once_boxes(pred_annos), np.float32), up(_cat([a['score'] for a in pred_annos], None, np.float32), np.float32),
                         up(once_codes_of(pred_names, self.names), np.int32)]
        pred_box, pred_score, pred_code = pred_side
        self._in = [up(o, np.int32) for o in self._host] + [up(self.pair_off, np.int64), up(once_boxes(gt_annos), np.float32), pred_box,
                                                            pred_score, up(once_codes_of(gt_names, self.names), np.int32), pred_code,
                                                            up(accept.view(np.int32), np.int32), up(thr, np.float64)]
        slots = ONCE_THRESHOLD_SLOTS
        self._overlaps, self._matched = e(self.NP), e(self.K, self.NG)
        self._flag_gt, self._flag_pred = e(self.C, self.B, self.NG, dtype=torch.int8), e(self.C, self.B, self.ND, dtype=torch.int8)
        self._num_valid, self._thresholds, self._n_thr = e(self.K, dtype=torch.int32), e(self.K, slots), e(self.K, dtype=torch.int32)
        self._counts = e(self.K, slots, 3, dtype=torch.int64)
        self._mode = list(ONCE_DIFFICULTY_MODES).index(difficulty_mode)
        self._heading = int(bool(ap_with_heading))
        self._curves = None
        if self.F == 0:                                                     # nothing to launch: no thresholds, every AP is 0
            self._num_valid.zero_(), self._thresholds.zero_(), self._n_thr.zero_(), self._counts.zero_()
            self._sorted = self._matched
            return
        self._run(L, L.load().gdmae_once_eval_workspace_bytes)

    def _call(self, L, stage, sorted_scores, ws, ws_bytes):
        L.call("gdmae_once_eval", stage, self.F, self.C, self._mode, self.num_pr_points, self._heading,
               *[h.ctypes.data for h in self._host], *[L.ptr(t) for t in self._in], L.ptr(self._overlaps), L.ptr(self._flag_gt),
               L.ptr(self._flag_pred), L.ptr(self._matched), L.ptr(sorted_scores), L.ptr(self._num_valid), L.ptr(self._thresholds),
               L.ptr(self._n_thr), L.ptr(self._counts), L.ptr(ws), ws_bytes, L.stream())

    def overlaps(self):
        """(NP) fp32: the 3-D IoU, per frame GT-major from ``pair_off[f]``.  A device tensor."""
        return self._overlaps

    def frame_overlaps(self, f):
        """numpy (G_f, P_f) of frame f, the layout of the statement (a host read: for tests and analysis)."""
        G, P = int(self.gt_off[f + 1] - self.gt_off[f]), int(self.pred_off[f + 1] - self.pred_off[f])
        return self._overlaps[int(self.pair_off[f]):int(self.pair_off[f + 1])].cpu().numpy().reshape(G, P)

    def flags(self):
        """-> (flag_gt (C, bands, NG), flag_pred (C, bands, ND)) int8: 1 outside the band, else -1 other class, else 0 accepted."""
        return self._flag_gt, self._flag_pred

    def matched_scores(self):
        """(K, NG) fp32: the score of the first pass's true positive per (combo, GT row), -inf elsewhere."""
        return self._matched

    def thresholds(self):
        """-> (thresholds (K, 64) fp32, 0 behind the count; counts (K) int32; num_valid_gt (K) int32)."""
        return self._thresholds, self._n_thr, self._num_valid

    def counts(self):
        """(K, 64, 3) int64: tp / fp / fn per (combo, threshold)."""
        return self._counts

    def curves(self):
        """-> precision, recall as (C, bands, num_pr_points + 1) fp64 numpy arrays.  The ONE host read (cached)."""
        if self._curves is None:
            packed = torch.cat([self._n_thr.to(torch.int64), self._counts.reshape(-1)]).cpu().numpy()
            self._curves = once_curves(packed[:self.K], packed[self.K:].reshape(self.K, ONCE_THRESHOLD_SLOTS, 3), self.C, self.B,
                                       self.num_pr_points)
        return self._curves

    def result(self):
        """-> (ret_str, ret_dict) of the reference"""
        return once_format_result(self.classes, self.curves()[0], self.num_pr_points, self.difficulty_mode, self.print_ok)


def once_eval(gt_annos, pred_annos, classes, use_superclass=True, iou_thresholds=None, num_pr_points=50,
              difficulty_mode='Overall&Distance', ap_with_heading=True, num_parts=100, print_ok=False, device="cuda"):
    """Drop-in for the reference's ``get_evaluation_results`` on the device -> (ret_str, ret_dict).  ``pred_annos``: the
    reference's list of dicts or a ``OnceDetections`` record."""
    return OnceEval(gt_annos, pred_annos, classes, device, use_superclass=use_superclass, iou_thresholds=iou_thresholds,
                    num_pr_points=num_pr_points, difficulty_mode=difficulty_mode, ap_with_heading=ap_with_heading, num_parts=num_parts,
                    print_ok=print_ok).result()


# ------------------------------------------------------------------------------------------------------------------------------------
# ONCE annos of the detections (reference ONCEDataset.generate_prediction_dicts).  ONCE predictions are the lidar boxes
# themselves: no kernel of this library, device copies and torch indexing only.
#
#     det = OnceDetections(class_names, device)
#     for batch_dict in loader:
#         det.update(engine.detect(batch_dict), batch_dict)           # device copies, no host read
#     ret_str, ret_dict = once_eval(gt_annos, det, class_names)       # ONE read of the per-frame counts, ONE of the counts table
# ------------------------------------------------------------------------------------------------------------------------------------
def once_annos_template(n=0):
    """the reference's ``get_template_prediction``"""
    return {'name': np.zeros(n), 'score': np.zeros(n), 'boxes_3d': np.zeros((n, 7))}


class OnceDetections(_DetectionStore):
    """The detections of an evaluation loop as a padded device store (``rows`` rows per frame, frames grown by doubling).  ``update``
    makes no host read; ``counts`` makes the one host read; ``compact`` and ``to_annos`` index with offsets built on the host."""

    MAX_ROWS, ALLOC = ONCE_MAX_ROWS, staticmethod(torch.zeros)
    CPU_DEVICE = "a device store; once_prediction_dicts is the CPU path"
    CPU_TENSORS = "once_prediction_dicts is the CPU path"

    def __init__(self, class_names, device, rows=500, frames=0):
        super().__init__(class_names, device, rows)
        if not self.class_names:
            raise ValueError("OnceDetections: no class names")
        self._reserve(int(frames))
        self._invalidate()

    def _invalidate(self):
        self._counts = self._annos = self._index = None

    def update(self, out, batch_dict=None):
        """out: the padded dict of ``detect`` (pred_boxes (B, n, >= 7), pred_scores (B, n), pred_labels (B, n), num (B)); batch_dict:
        ``frame_id`` (B), optional.  No host read."""
        boxes, scores, labels, num = self._checked(out)
        B = scores.shape[0]
        ids = list(batch_dict['frame_id']) if batch_dict is not None and 'frame_id' in batch_dict else list(range(self.F, self.F + B))
        if len(ids) != B:
            raise ValueError(f"OnceDetections.update: {B} samples, {len(ids)} frame ids")
        self._append(boxes, scores, labels, num, ids)

    def counts(self):
        """(F) int64 per-frame counts on the host: THE host read (cached until the next ``update``)."""
        if self._counts is None:
            self._counts = self._store['num'][:self.F].cpu().numpy().astype(np.int64) if self.F else np.zeros(0, np.int64)
            self._counts_in_range(self._counts)
        return self._counts

    def _rows_index(self):
        """the flat store rows (frame * rows + row) of the compact table, built on the host from the counts and uploaded"""
        counts = self.counts()
        if self._index is None:
            off = _offsets(counts)
            idx = np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1], counts) + np.repeat(np.arange(self.F, dtype=np.int64) * self.rows, counts)
            pinned = torch.from_numpy(idx).pin_memory()                              # an upload that does not wait for the device
            self._index = (torch.empty(idx.shape[0], dtype=torch.int64, device=self.device).copy_(pinned, non_blocking=True), pinned)
        return self._index[0]

    def compact(self, names):
        """-> boxes (ND, 7) fp32, scores (ND) fp32, codes (ND) int32 on the device: the rows below ``num`` of every frame in order, the
        labels mapped to their codes in ``names`` (``len(names)`` for a name that is not in it).  No host read beyond ``counts``."""
        idx = self._rows_index()
        table = torch.tensor([names.index(c) if c in names else len(names) for c in self.class_names], dtype=torch.int32).to(self.device)
        s, F = self._store, self.F
        labels = s['labels'][:F].reshape(-1).index_select(0, idx)
        codes = table.index_select(0, (labels - 1).clamp_(0, len(self.class_names) - 1))
        return (s['boxes'][:F].reshape(-1, 7).index_select(0, idx).contiguous(), s['scores'][:F].reshape(-1).index_select(0, idx).contiguous(),
                codes.contiguous())

    def to_annos(self):
        """The reference's list of dicts: name, score (n) fp32, boxes_3d (n, 7) fp32, frame_id.  One more host read (cached)."""
        if self._annos is None:
            off = _offsets(self.counts())
            idx = self._rows_index()
            s, F = self._store, self.F
            flat = torch.cat([s['boxes'][:F].reshape(-1, 7).index_select(0, idx), s['scores'][:F].reshape(-1).index_select(0, idx)[:, None],
                              s['labels'][:F].reshape(-1).index_select(0, idx).to(torch.float32)[:, None]], dim=1).cpu().numpy()
            names = np.array(self.class_names)
            annos = []
            for f in range(F):
                r = flat[int(off[f]):int(off[f + 1])]
                anno = once_annos_template(0)
                if r.shape[0]:
                    anno = {'name': names[r[:, 8].astype(np.int64) - 1], 'score': r[:, 7].copy(), 'boxes_3d': r[:, :7].copy()}
                anno['frame_id'] = self.frame_ids[f]
                annos.append(anno)
            self._annos = annos
        return self._annos


def once_prediction_dicts(batch_dict, pred_dicts, class_names, output_path=None):
    """Drop-in for the reference's ``ONCEDataset.generate_prediction_dicts``: ``pred_dicts`` is the per-sample list of pred_boxes
    (n, >= 7), pred_scores (n), pred_labels (n) (1-based) -> the list of dicts name / score / boxes_3d (fp32) / frame_id."""
    if output_path is not None:
        raise NotImplementedError("once_prediction_dicts: output_path (the reference does not write ONCE result files either)")
    names = np.array([str(c) for c in class_names])
    annos = []
    for b, d in enumerate(pred_dicts):
        scores = _host(d['pred_scores'], np.float32).reshape(-1)
        anno = once_annos_template(0)
        if scores.shape[0]:
            boxes = _host(d['pred_boxes'], np.float32)
            anno = {'name': names[_host(d['pred_labels'], np.int64).reshape(-1) - 1], 'score': scores.copy(),
                    'boxes_3d': np.ascontiguousarray(boxes.reshape(scores.shape[0], -1)[:, :7])}
        anno['frame_id'] = batch_dict['frame_id'][b]
        annos.append(anno)
    return annos


def evaluate_once(engine, batches, gt_annos, class_names, keep_annos=False, **options):
    """The loop of ``evaluate_kitti`` with a ``OnceDetections`` record, then ``once_eval`` from the record -> (ret_str, ret_dict, the
    reference's anno list or None).  ``options``: those of ``once_eval`` (``use_superclass``, ``iou_thresholds``, ...).  The store
    starts with 500 rows per frame (ONCE's ``NMS_POST_MAXSIZE``) or the first batch's width if that is larger, and is widened on the
    device when a later batch is wider; beyond 1024 rows ``OnceDetections`` refuses by name."""
    det = None
    for bd in batches:
        out = engine.detect(bd)
        n = int(out['pred_scores'].shape[1])
        if det is None:
            det = OnceDetections(class_names, out['pred_scores'].device, rows=max(500, n))
        elif n > det.rows:
            det.widen(n)
        det.update(out, bd)
    if det is None:
        raise ValueError("evaluate_once: no batches")
    ret_str, ret_dict = once_eval(gt_annos, det, class_names, **options)
    return ret_str, ret_dict, (det.to_annos() if keep_annos else None)
