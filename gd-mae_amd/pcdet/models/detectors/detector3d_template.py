"""Model-builder subset of the reference ``Detector3DTemplate``
(pcdet/models/detectors/detector3d_template.py:14-100, 361-442): the ``module_topology`` walk with the
same keyword calls into the name->class registries, ``global_step``, and checkpoint loading by
key+shape, the RoI head of the two-stage config included.  Builders for modules outside the built paths return ``None`` unless their yaml
section is present, in which case they raise (nothing is silently skipped)."""
import os

import torch
import torch.nn as nn

from .. import backbones_2d, backbones_3d, dense_heads, roi_heads
from ..backbones_3d import vfe


class Detector3DTemplate(nn.Module):
    def __init__(self, model_cfg, num_class, dataset, logger):
        super().__init__()
        self.model_cfg, self.num_class, self.dataset, self.logger = model_cfg, num_class, dataset, logger
        self.class_names = dataset.class_names
        self.register_buffer('global_step', torch.LongTensor(1).zero_())
        self.module_topology = ['img_backbone', 'vfe', 'backbone_3d', 'map_to_bev_module', 'pfe', 'backbone_2d',
                                'dense_head', 'point_head', 'roi_head']
        self._cfg_key = {'img_backbone': 'IMG_BACKBONE', 'vfe': 'VFE', 'backbone_3d': 'BACKBONE_3D',
                         'map_to_bev_module': 'MAP_TO_BEV', 'pfe': 'PFE', 'backbone_2d': 'BACKBONE_2D',
                         'dense_head': 'DENSE_HEAD', 'point_head': 'POINT_HEAD', 'roi_head': 'ROI_HEAD'}

    @property
    def mode(self):
        return 'TRAIN' if self.training else 'TEST'

    def update_global_step(self):
        self.global_step += 1

    def build_networks(self):
        info = {'module_list': [], 'num_rawpoint_features': self.dataset.point_feature_encoder.num_point_features,
                'num_point_features': self.dataset.point_feature_encoder.num_point_features,
                'grid_size': self.dataset.grid_size, 'point_cloud_range': self.dataset.point_cloud_range,
                'voxel_size': self.dataset.voxel_size}
        for name in self.module_topology:
            builder = getattr(self, 'build_%s' % name, None)
            if builder is None:
                if self.model_cfg.get(self._cfg_key[name], None) is not None:
                    raise NotImplementedError(f"{self._cfg_key[name]} is outside the GD-MAE pre-training hot path")
                module = None
            else:
                module, info = builder(model_info_dict=info)
            self.add_module(name, module)
        return info['module_list']

    def build_vfe(self, model_info_dict):
        if self.model_cfg.get('VFE', None) is None:
            return None, model_info_dict
        m = vfe.__all__[self.model_cfg.VFE.NAME](
            model_cfg=self.model_cfg.VFE, num_point_features=model_info_dict['num_rawpoint_features'],
            point_cloud_range=model_info_dict['point_cloud_range'], voxel_size=model_info_dict['voxel_size'],
            grid_size=model_info_dict['grid_size'])
        model_info_dict['num_point_features'] = m.get_output_feature_dim()
        model_info_dict['module_list'].append(m)
        return m, model_info_dict

    def build_backbone_3d(self, model_info_dict):
        if self.model_cfg.get('BACKBONE_3D', None) is None:
            return None, model_info_dict
        m = backbones_3d.__all__[self.model_cfg.BACKBONE_3D.NAME](
            model_cfg=self.model_cfg.BACKBONE_3D, input_channels=model_info_dict['num_point_features'],
            grid_size=model_info_dict['grid_size'], voxel_size=model_info_dict['voxel_size'],
            point_cloud_range=model_info_dict['point_cloud_range'])
        model_info_dict['module_list'].append(m)
        model_info_dict['num_point_features'] = m.num_point_features
        model_info_dict['backbone_channels'] = getattr(m, 'backbone_channels', None)
        return m, model_info_dict

    def build_backbone_2d(self, model_info_dict):
        if self.model_cfg.get('BACKBONE_2D', None) is None:
            return None, model_info_dict
        m = backbones_2d.__all__[self.model_cfg.BACKBONE_2D.NAME](
            model_cfg=self.model_cfg.BACKBONE_2D, input_channels=model_info_dict.get('num_bev_features', None))
        model_info_dict['module_list'].append(m)
        model_info_dict['num_bev_features'] = m.num_bev_features
        return m, model_info_dict

    def build_dense_head(self, model_info_dict):
        if self.model_cfg.get('DENSE_HEAD', None) is None:
            return None, model_info_dict
        m = dense_heads.__all__[self.model_cfg.DENSE_HEAD.NAME](
            model_cfg=self.model_cfg.DENSE_HEAD, input_channels=model_info_dict['num_bev_features'],
            num_class=self.num_class if not self.model_cfg.DENSE_HEAD.CLASS_AGNOSTIC else 1, class_names=self.class_names,
            grid_size=model_info_dict['grid_size'], point_cloud_range=model_info_dict['point_cloud_range'],
            predict_boxes_when_training=self.model_cfg.get('ROI_HEAD', False), voxel_size=model_info_dict.get('voxel_size', False),
            backbone_channels=model_info_dict.get('backbone_channels', None))
        model_info_dict['module_list'].append(m)
        return m, model_info_dict

    def build_roi_head(self, model_info_dict):
        if self.model_cfg.get('ROI_HEAD', None) is None:
            return None, model_info_dict
        m = roi_heads.__all__[self.model_cfg.ROI_HEAD.NAME](
            model_cfg=self.model_cfg.ROI_HEAD, input_channels=model_info_dict['num_point_features'],
            backbone_channels=model_info_dict.get('backbone_channels', None), point_cloud_range=model_info_dict['point_cloud_range'],
            voxel_size=model_info_dict['voxel_size'], num_class=self.num_class if not self.model_cfg.ROI_HEAD.CLASS_AGNOSTIC else 1)
        model_info_dict['module_list'].append(m)
        return m, model_info_dict

    @staticmethod
    def generate_recall_record(box_preds, recall_dict, batch_index, data_dict=None, thresh_list=None):
        """Recall bookkeeping of the evaluation loop (reference detector3d_template.py:318-358): ground-truth boxes matched by
        a predicted box with 3-D IoU above each threshold (``recall_rcnn_*``; ``recall_roi_*`` when RoIs are present)."""
        from ...ops.iou3d_nms import iou3d_nms_utils
        if 'gt_boxes' not in data_dict:
            return recall_dict
        rois = data_dict['rois'][batch_index] if 'rois' in data_dict else None
        gt = data_dict['gt_boxes'][batch_index]
        if len(recall_dict) == 0:
            recall_dict = {'gt_num': 0}
            for t in thresh_list:
                recall_dict['recall_roi_%s' % str(t)] = 0
                recall_dict['recall_rcnn_%s' % str(t)] = 0
        nz = (gt.abs().sum(dim=1) != 0).nonzero()
        gt = gt[:int(nz.max()) + 1] if nz.numel() else gt[:0]       # trailing all-zero rows are padding
        if gt.shape[0] > 0:
            iou_rcnn = iou3d_nms_utils.boxes_iou3d_gpu(box_preds[:, 0:7], gt[:, 0:7]) if box_preds.shape[0] > 0 else None
            iou_roi = iou3d_nms_utils.boxes_iou3d_gpu(rois[:, 0:7], gt[:, 0:7]) if rois is not None else None
            for t in thresh_list:
                if iou_rcnn is not None:
                    recall_dict['recall_rcnn_%s' % str(t)] += int((iou_rcnn.max(dim=0)[0] > t).sum().item())
                if iou_roi is not None:
                    recall_dict['recall_roi_%s' % str(t)] += int((iou_roi.max(dim=0)[0] > t).sum().item())
            recall_dict['gt_num'] += gt.shape[0]
        return recall_dict

    def post_processing(self, batch_dict):
        """(pred_dicts, recall_dict) from ``batch_cls_preds`` (B, n, n_class) / ``batch_box_preds`` (B, n, 7) tensors: the shipped
        branch of the reference's post_processing (detector3d_template.py:196-316) - sigmoid unless ``cls_preds_normalized``, best
        class -> label + 1, ``class_agnostic_nms`` (model_nms_utils.py:6-25: SCORE_THRESH mask, the NMS_PRE_MAXSIZE best, rotated
        NMS, NMS_POST_MAXSIZE) and the recall record.  On the device the scores never reach torch ops: ``gdmae_anchor_select`` (one
        launch for the whole batch) leaves the anchors above the threshold compacted in anchor order, so the top-k, the gather
        and the NMS see a few hundred rows per sample instead of n.  ``fused_select = False``: the same with torch ops."""
        cfg = self.model_cfg.POST_PROCESSING
        nms = cfg.NMS_CONFIG
        if nms.MULTI_CLASSES_NMS:
            raise NotImplementedError("MULTI_CLASSES_NMS: True (per-class NMS in post_processing) is not built")
        if isinstance(batch_dict['batch_cls_preds'], list) or isinstance(batch_dict['batch_box_preds'], list):
            raise NotImplementedError("list-valued batch_cls_preds / batch_box_preds (multi-head) are not built")
        nms_off = not nms.get('NMS', True)
        if batch_dict.get('has_class_labels', False) and not nms_off:
            raise NotImplementedError("has_class_labels (labels from a RoI head) with NMS on is not built in post_processing")
        if batch_dict.get('batch_index', None) is not None:
            raise NotImplementedError("batch_index (concatenated predictions) is not built in post_processing")
        if cfg.get('OUTPUT_RAW_SCORE', False):
            raise NotImplementedError("post_processing: OUTPUT_RAW_SCORE True is not built")
        if nms_off:
            return self.post_processing_without_nms(batch_dict)
        if nms.NMS_TYPE != 'nms_gpu':
            raise NotImplementedError("post_processing: only NMS_TYPE nms_gpu with OUTPUT_RAW_SCORE False is built")
        from gdmae_hip import lib as L
        cls_all, box_all = batch_dict['batch_cls_preds'], batch_dict['batch_box_preds']
        B = batch_dict['batch_size']
        assert box_all.dim() == 3 and cls_all.shape[2] in (1, self.num_class)
        normalized = bool(batch_dict['cls_preds_normalized'])
        thresh = cfg.SCORE_THRESH
        fused = getattr(self, 'fused_select', True) and cls_all.is_cuda and thresh is not None
        if fused:
            n, C = cls_all.shape[1], cls_all.shape[2]
            cls_c = cls_all.float().contiguous()
            idx = torch.empty(B, n, dtype=torch.int32, device=cls_c.device)
            score = torch.empty(B, n, dtype=torch.float32, device=cls_c.device)
            label = torch.empty(B, n, dtype=torch.int32, device=cls_c.device)
            count = torch.empty(B, dtype=torch.int32, device=cls_c.device)
            L.call("gdmae_anchor_select", L.ptr(cls_c), B, n, C, int(normalized), float(thresh), L.ptr(idx), L.ptr(score), L.ptr(label),
                   L.ptr(count), L.stream())
            counts = count.tolist()                     # the one host read of the call: the output shapes depend on it
        recall_dict, pred_dicts = {}, []
        for b in range(B):
            box_preds = box_all[b]
            if fused:
                m = counts[b]
                orig, scores, labels = idx[b, :m].long(), score[b, :m], label[b, :m].long()
            else:
                cp = cls_all[b] if normalized else torch.sigmoid(cls_all[b])
                sc_all, lab_all = torch.max(cp, dim=-1)
                lab_all = lab_all + 1
                mask = sc_all >= thresh if thresh is not None else torch.ones_like(sc_all, dtype=torch.bool)
                orig = mask.nonzero().view(-1)
                scores, labels = sc_all[orig], lab_all[orig]
            pred, recall_dict = self.finish_sample(box_preds[orig], scores, labels, recall_dict, b, batch_dict,
                                                   all_boxes=box_preds if 'rois' in batch_dict else None)
            pred_dicts.append(pred)
        return pred_dicts, recall_dict

    def post_processing_without_nms(self, batch_dict):
        """The ``NMS: False`` branch (reference detector3d_template.py:269-299; the two-stage configs): the score is the maximum
        over the classes, the label comes from ``roi_labels`` (``batch_pred_labels``) when ``has_class_labels`` and is the best
        class + 1 otherwise, no box is selected; rows with label 0 (padded RoIs) are dropped; the recall record is computed on
        all boxes when RoIs are present."""
        cfg = self.model_cfg.POST_PROCESSING
        cls_all, box_all = batch_dict['batch_cls_preds'], batch_dict['batch_box_preds']
        assert box_all.dim() == 3 and cls_all.shape[2] in (1, self.num_class)
        recall_dict, pred_dicts = {}, []
        for b in range(batch_dict['batch_size']):
            box_preds = box_all[b]
            cp = cls_all[b] if batch_dict['cls_preds_normalized'] else torch.sigmoid(cls_all[b])
            scores, labels = torch.max(cp, dim=-1)
            if batch_dict.get('has_class_labels', False):
                labels = batch_dict['roi_labels' if 'roi_labels' in batch_dict else 'batch_pred_labels'][b]
            else:
                labels = labels + 1
            ok = labels != 0
            final_boxes, final_scores, final_labels = box_preds[ok], scores[ok], labels[ok]
            if cfg.get('RECALL_MODE', 'normal') == 'normal':
                recall_dict = self.generate_recall_record(box_preds=final_boxes if 'rois' not in batch_dict else box_preds,
                                                          recall_dict=recall_dict, batch_index=b, data_dict=batch_dict,
                                                          thresh_list=cfg.RECALL_THRESH_LIST)
            pred_dicts.append({'pred_boxes': final_boxes, 'pred_scores': final_scores, 'pred_labels': final_labels})
        return pred_dicts, recall_dict

    def finish_sample(self, boxes, scores, labels, recall_dict, batch_index, batch_dict, all_boxes=None):
        """The per-sample tail of ``post_processing`` on PRE-SELECTED anchors: ``boxes`` (m, 7+), ``scores`` (m), ``labels`` (m, int64,
        1-based) of the anchors at or above SCORE_THRESH, in anchor order.  The NMS_PRE_MAXSIZE best, rotated NMS, NMS_POST_MAXSIZE,
        the ``label != 0`` filter and the recall record (on ``all_boxes`` when RoIs are present).  -> (pred_dict, recall_dict)."""
        from ...ops.iou3d_nms import iou3d_nms_utils
        cfg = self.model_cfg.POST_PROCESSING
        nms = cfg.NMS_CONFIG
        if scores.shape[0] > 0:
            top_scores, top = torch.topk(scores, k=min(int(nms.NMS_PRE_MAXSIZE), scores.shape[0]))
            keep, _ = iou3d_nms_utils.nms_gpu(boxes[top][:, 0:7], top_scores, nms.NMS_THRESH)
            sel = top[keep[:int(nms.NMS_POST_MAXSIZE)]]
        else:
            sel = torch.zeros(0, dtype=torch.int64, device=scores.device)
        final_scores, final_labels, final_boxes = scores[sel], labels[sel], boxes[sel]
        ok = final_labels != 0
        final_boxes, final_scores, final_labels = final_boxes[ok], final_scores[ok], final_labels[ok]
        if cfg.get('RECALL_MODE', 'normal') == 'normal':
            recall_dict = self.generate_recall_record(box_preds=final_boxes if all_boxes is None else all_boxes,
                                                      recall_dict=recall_dict, batch_index=batch_index, data_dict=batch_dict,
                                                      thresh_list=cfg.RECALL_THRESH_LIST)
        return {'pred_boxes': final_boxes, 'pred_scores': final_scores, 'pred_labels': final_labels}, recall_dict

    # ---- the same tail for the whole batch on the device (csrc/anchor_detect.hip)
    def _batched_plan(self):
        """(NMS_PRE_MAXSIZE, NMS_POST_MAXSIZE, NMS_THRESH) of ``finish_batch``; everything the batched tail does not build is refused
        here by name."""
        cfg = self.model_cfg.POST_PROCESSING
        nms = cfg.NMS_CONFIG
        if nms.MULTI_CLASSES_NMS:
            raise NotImplementedError("finish_batch: MULTI_CLASSES_NMS: True (per-class NMS) is not built")
        if not nms.get('NMS', True):
            raise NotImplementedError("finish_batch: NMS: False (the batched tail is the NMS branch of post_processing)")
        if cfg.get('OUTPUT_RAW_SCORE', False):
            raise NotImplementedError("finish_batch: OUTPUT_RAW_SCORE True is not built")
        if nms.NMS_TYPE != 'nms_gpu':
            raise NotImplementedError(f"finish_batch: NMS_TYPE {nms.NMS_TYPE} (built: nms_gpu)")
        pre, post = int(nms.NMS_PRE_MAXSIZE), int(nms.NMS_POST_MAXSIZE)
        if pre > 4096:
            raise NotImplementedError(f"finish_batch: NMS_PRE_MAXSIZE {pre} > 4096 (the candidates of a sample are sorted in LDS)")
        if pre < 1 or post < 1:
            raise NotImplementedError(f"finish_batch: NMS_PRE_MAXSIZE {pre} / NMS_POST_MAXSIZE {post} below 1")
        return pre, post, float(nms.NMS_THRESH)

    def batched_rows(self):
        """Rows per sample of the padded output of ``finish_batch``: min(NMS_PRE_MAXSIZE, NMS_POST_MAXSIZE)."""
        pre, post, _ = self._batched_plan()
        return min(pre, post)

    def finish_batch(self, count, scores, labels, boxes):
        """``finish_sample`` for all samples in ``gdmae_anchor_detect`` (three launches, no host read), on the anchors at or above
        SCORE_THRESH as ``gdmae_anchor_head_infer`` leaves them: ``count`` (B) int32, ``scores`` (B, A) fp32, ``labels`` (B, A) int32
        1-based, ``boxes`` (B, A, 7) fp32; the first count[b] rows of a sample are read.  Ties in the score go to the earlier row, which
        ``finish_sample`` leaves unspecified.  -> {'pred_boxes' (B, n, 7), 'pred_scores' (B, n), 'pred_labels' (B, n) int64, 'num' (B)
        int32} on the device, n = ``batched_rows()``; rows at or beyond num[b] are zero (label 0).  No recall record."""
        from gdmae_hip import lib as L
        pre, post, thresh = self._batched_plan()
        if not all(t.is_cuda for t in (count, scores, labels, boxes)):
            raise NotImplementedError("finish_batch: CPU tensors (the tail runs in libgdmae_hip.so, no CPU fallback)")
        B, A = scores.shape
        if (count.dtype, scores.dtype, labels.dtype, boxes.dtype) != (torch.int32, torch.float32, torch.int32, torch.float32) or \
                tuple(count.shape) != (B,) or tuple(labels.shape) != (B, A) or tuple(boxes.shape) != (B, A, 7):
            raise NotImplementedError("finish_batch: count (B) int32, scores (B, A) fp32, labels (B, A) int32, boxes (B, A, 7) fp32")
        dev = scores.device
        n_out = min(pre, post)
        out = {'pred_boxes': torch.empty(B, n_out, 7, dtype=torch.float32, device=dev),
               'pred_scores': torch.empty(B, n_out, dtype=torch.float32, device=dev),
               'pred_labels': torch.empty(B, n_out, dtype=torch.int64, device=dev),
               'num': torch.empty(B, dtype=torch.int32, device=dev)}
        ws = torch.empty(L.load().gdmae_anchor_detect_workspace_bytes(B, pre), dtype=torch.uint8, device=dev)
        L.call("gdmae_anchor_detect", L.ptr(count), L.ptr(scores), L.ptr(labels), L.ptr(boxes), B, A, pre, post, thresh, n_out,
               L.ptr(out['pred_boxes']), L.ptr(out['pred_scores']), L.ptr(out['pred_labels']), L.ptr(out['num']), L.ptr(ws), L.stream())
        return out

    @staticmethod
    def padded_to_pred_dicts(out):
        """The padded tensors of ``finish_batch`` -> the per-sample list ``post_processing`` returns.  ONE host read (``num``)."""
        num = out['num'].tolist()
        return [{'pred_boxes': out['pred_boxes'][b, :n], 'pred_scores': out['pred_scores'][b, :n], 'pred_labels': out['pred_labels'][b, :n]}
                for b, n in enumerate(num)]

    def forward(self, **kwargs):
        raise NotImplementedError

    # ---- checkpoints (reference-compatible dict: model_state / optimizer_state / epoch / it / version)
    def _load_state_dict(self, model_state_disk, *, strict=True):
        """Load by key + shape (reference detector3d_template.py:360-388).  Sparse-conv weights saved by another spconv
        generation are re-laid first: a tensor whose last two axes are swapped w.r.t. ours (spconv 1.x keeps (..., Cin, Cout))
        is transposed; failing that, the kernel-first layout (k.., Cin, Cout) is rotated to ours (Cout, k.., Cin) - the
        reference does this for 5-D (3-D conv) weights only and asserts otherwise, the 2-D convolutions of this path get the
        same treatment.  With ``strict`` the FILTERED dict is what ``load_state_dict`` sees, so keys of ours that the file
        does not cover raise, while foreign / mis-shaped keys of the file are ignored - exactly the reference's behaviour."""
        from ...utils.spconv_utils import find_all_spconv_keys
        state_dict = self.state_dict()
        sparse_keys = find_all_spconv_keys(self)
        update = {}
        for key, val in model_state_disk.items():
            want = state_dict.get(key, None)
            if want is None:
                continue
            if key in sparse_keys and want.shape != val.shape and val.dim() == want.dim():
                swapped = val.transpose(-1, -2)
                rotated = val.permute(val.dim() - 1, *range(val.dim() - 1))
                if swapped.shape == want.shape:
                    val = swapped.contiguous()
                elif rotated.shape == want.shape:
                    val = rotated.contiguous()
            if want.shape == val.shape:
                update[key] = val
        if strict:
            self.load_state_dict(update)
        else:
            state_dict.update(update)
            self.load_state_dict(state_dict)
        return state_dict, update

    def load_params_from_file(self, filename, logger, to_cpu=False):
        if not os.path.isfile(filename):
            raise FileNotFoundError(filename)
        ckpt = torch.load(filename, map_location=torch.device('cpu') if to_cpu else None)
        disk = ckpt['model_state']
        logger.info('==> Loading parameters from checkpoint %s (version %s)' % (filename, ckpt.get('version', None)))
        state_dict, update = self._load_state_dict(disk, strict=False)
        for k in state_dict:
            if k not in update:
                logger.info('Not updated weight %s: %s' % (k, str(state_dict[k].shape)))
        logger.info('==> Done (loaded %d/%d)' % (len(update), len(state_dict)))

    def load_params_with_optimizer(self, filename, to_cpu=False, optimizer=None, logger=None):
        if not os.path.isfile(filename):
            raise FileNotFoundError(filename)
        ckpt = torch.load(filename, map_location=torch.device('cpu') if to_cpu else None)
        self._load_state_dict(ckpt['model_state'], strict=True)
        if optimizer is not None and ckpt.get('optimizer_state', None) is not None:
            optimizer.load_state_dict(ckpt['optimizer_state'])
        return ckpt.get('it', 0.0), ckpt.get('epoch', -1)
