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

The second half of this module is the official KITTI AP table (``kitti_eval``, ``KittiEval``, ``kitti_eval_numpy``)."""
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
    C = len(classes)
    names = lambda annos: np.concatenate([np.asarray(a['name'], dtype=str).reshape(-1) for a in annos] + [np.zeros(0, dtype=str)])      # noqa: E731
    gt_raw, dt_raw = names(gt_annos), names(dt_annos)
    gt_name, dt_name = _LowerNames(gt_raw), _LowerNames(dt_raw)
    gt_count = [len(a['name']) for a in gt_annos]
    gt_off, dt_off = _offsets(gt_count), _offsets([len(a['name']) for a in dt_annos])
    dc_rows = gt_raw == "DontCare"
    dc_count = np.bincount(np.repeat(np.arange(len(gt_annos)), gt_count)[dc_rows], minlength=len(gt_annos))
    NG, ND = int(gt_off[-1]), int(dt_off[-1])
    gt_ignore = _per_row(gt_annos, ('occluded', 'truncated', 'bbox'), (None, None, 4), lambda occ, tr, bb: np.stack(
        [(occ > KITTI_MAX_OCCLUSION[l]) | (tr > KITTI_MAX_TRUNCATION[l]) | ((bb[:, 3] - bb[:, 1]) <= KITTI_MIN_HEIGHT[l]) for l in range(3)]))
    dt_small = _per_row(dt_annos, ('bbox',), (4,), lambda bb: np.stack([np.abs(bb[:, 3] - bb[:, 1]) < KITTI_MIN_HEIGHT[l] for l in range(3)]))
    ignored_gt, ignored_dt = np.full((C, 3, NG), -1, np.int8), np.full((C, 3, ND), -1, np.int8)
    for c, cls in enumerate(classes):
        name = KITTI_CLASS_NAMES[cls].lower()
        own = gt_name == name
        neighbour = gt_name == {'pedestrian': 'person_sitting', 'car': 'van'}.get(name, '')       # rows that count as "ignored 1"
        own_dt = dt_name == name
        for l in range(3):
            ignored_gt[c, l][own & ~gt_ignore[l]] = 0
            ignored_gt[c, l][neighbour | (own & gt_ignore[l])] = 1
            ignored_dt[c, l][own_dt] = 0
            ignored_dt[c, l][dt_small[l]] = 1
    return dict(gt_off=gt_off, dt_off=dt_off, dc_off=_offsets(dc_count), ignored_gt=ignored_gt, ignored_dt=ignored_dt,
                num_valid=(ignored_gt == 0).sum(axis=2).astype(np.int64), dc_rows=dc_rows)


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


def _statement_first_pass(ov, score, ign_gt, ign_dt, min_ov):
    """``compute_statistics_jit(compute_fp=False)`` on one frame: ov (D, G) -> the true positives' scores per GT row, -inf elsewhere."""
    D, G = ov.shape
    out, assigned = np.full(G, -np.inf, np.float32), np.zeros(D, bool)
    live = (ign_dt != -1) & (score > KITTI_NO_DETECTION)
    for g in range(G):
        if ign_gt[g] == -1:
            continue
        cand = live & ~assigned & (ov[:, g] > min_ov)
        if not cand.any():
            continue
        j = int(np.argmax(np.where(cand, score, -np.inf)))      # the highest score; among equal scores the lowest index (strict >)
        assigned[j] = True
        if not (ign_gt[g] == 1 or ign_dt[j] == 1):
            out[g] = score[j]
    return out


def _statement_second_pass(ov, score, gt_alpha, dt_alpha, ign_gt, ign_dt, dc_max, min_ov, thresholds, compute_aos):
    """``compute_statistics_jit(compute_fp=True)`` on one frame for all T thresholds at once -> tp, fp, fn (T) int64, sim (T) fp64.
    Per GT row the reference's loop over the detections ends with the non-ignored candidate of the largest overlap (the first of
    equals), and only without one with the FIRST candidate among the ``ignored 1`` detections."""
    D, G = ov.shape
    T = len(thresholds)
    keep = ~(score[None, :] < np.asarray(thresholds, np.float32)[:, None])
    c0, c1 = keep & (ign_dt == 0)[None, :], keep & (ign_dt == 1)[None, :]
    assigned = np.zeros((T, D), bool)
    tp, fn, sim, rows = np.zeros(T, np.int64), np.zeros(T, np.int64), np.zeros(T, np.float64), np.arange(T)
    for g in range(G):
        if ign_gt[g] == -1 or D == 0:
            fn += int(ign_gt[g] == 0)
            continue
        over = (ov[:, g] > min_ov)[None, :]
        m0 = c0 & ~assigned & over
        has0 = m0.any(axis=1)
        j0 = np.argmax(np.where(m0, ov[:, g][None, :], -1.0), axis=1)
        m1 = c1 & ~assigned & over
        has1 = m1.any(axis=1) & ~has0
        j = np.where(has0, j0, np.argmax(m1, axis=1))
        found = has0 | has1
        if ign_gt[g] == 0:
            fn += ~found
        assigned[rows[found], j[found]] = True
        is_tp = has0 & (ign_gt[g] == 0)
        tp += is_tp
        if compute_aos:
            sim += np.where(is_tp, (1.0 + np.cos(float(gt_alpha[g]) - dt_alpha[j].astype(np.float64))) / 2.0, 0.0)
    left = c0 & ~assigned
    if dc_max is not None:
        left &= ~(dc_max > min_ov)[None, :]
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
            matched[k, go[f]:go[f + 1]] = _statement_first_pass(overlaps[f][m], score[do[f]:do[f + 1]], ig[cl, go[f]:go[f + 1]],
                                                                idt[cl, do[f]:do[f + 1]], mn)
        tps = np.sort(matched[k][matched[k] > -np.inf])[::-1]
        th = kitti_get_thresholds(tps, int(combo_ngt[k]))
        n_thr[k] = len(th)
        thresholds[k, :len(th)] = th
        for f in range(F):
            tp, fp, fn, sim = _statement_second_pass(
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


class KittiEval:
    """The stages of ``kitti_eval`` as device tensors (csrc/kitti_eval.hip: five launches and one ``torch.sort`` between the two
    calls; no host read until ``curves``).  Geometry, boxes, alpha and SCORES are uploaded as fp32: scores are compared as fp32 values
    (two scores that differ only beyond fp32 are a tie, and the lowest detection index wins it, as the reference's strict ``>`` does
    for equal scores); an overlap is an fp32 value that is widened to fp64 against ``min_overlap``.  The per-box flags come from
    ``kitti_clean_data`` on the host, on the annos' own dtypes."""

    def __init__(self, gt_annos, dt_annos, class_names, device="cuda"):
        from . import lib as L
        device = torch.device(device)
        if device.type != "cuda":
            raise NotImplementedError("kitti_eval: CPU device (the statistics are computed in libgdmae_hip.so, no CPU fallback; "
                                      "kitti_eval_numpy is the CPU path)")
        self.classes = kitti_class_ints(class_names)
        self.compute_aos = kitti_compute_aos(dt_annos)
        cd = self.clean = kitti_clean_data(gt_annos, dt_annos, self.classes)
        self.F, self.C = len(gt_annos), len(self.classes)
        go, do = cd['gt_off'], cd['dt_off']
        for what, off in (("GT rows", go), ("detections", do)):
            if self.F and int(np.diff(off).max()) > KITTI_MAX_ROWS:
                raise ValueError(f"kitti_eval: a frame with {int(np.diff(off).max())} {what} (at most {KITTI_MAX_ROWS})")
        self.pair_off = _offsets(np.diff(go) * np.diff(do))
        self.NG, self.ND, self.NP = int(go[-1]), int(do[-1]), int(self.pair_off[-1])
        gt, dt = kitti_geometry(gt_annos, False), kitti_geometry(dt_annos, True)
        cl, me, mn, ng = kitti_combos(self.classes, cd['num_valid'])
        self.K = len(cl)
        self._host = [np.ascontiguousarray(o, np.int32) for o in (go, do, cd['dc_off'])]          # kept alive: read by the entry point
        up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t)).to(device)      # noqa: E731
        f32 = np.float32
        self._in = [up(o, np.int32) for o in self._host] + [up(self.pair_off, np.int64)] + [
            up(gt['bbox'], f32), up(gt['geo'], f32), up(gt['alpha'], f32), up(dt['bbox'], f32), up(dt['geo'], f32), up(dt['alpha'], f32),
            up(dt['score'], f32), up(gt['bbox'][cd['dc_rows']], f32), up(cd['ignored_gt'], np.int8), up(cd['ignored_dt'], np.int8),
            up(cl, np.int32), up(me, np.int32), up(mn, np.float64), up(ng, np.int32)]
        e = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device=device)      # noqa: E731
        self._overlaps, self._dc_max, self._matched = e(3, self.NP), e(self.ND), e(self.K, self.NG)
        self._thresholds, self._n_thr = e(self.K, KITTI_SAMPLE_PTS), e(self.K, dtype=torch.int32)
        self._pr_counts, self._pr_sim = e(self.K, KITTI_SAMPLE_PTS, 3, dtype=torch.int64), e(self.K, KITTI_SAMPLE_PTS, dtype=torch.float64)
        self._curves = None
        with torch.cuda.device(device):
            ws_bytes = L.load().gdmae_kitti_eval_workspace_bytes(self.F, self.K)
            ws = e(max(ws_bytes, 1), dtype=torch.uint8)
            self._call(L, 1, None, None, 0)
            self._sorted = torch.sort(self._matched, dim=1, descending=True).values.contiguous()
            self._call(L, 2, self._sorted, ws, ws_bytes)

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
