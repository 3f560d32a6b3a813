"""CPU: the batched CenterHead tail is declared, bound and sized, and refuses by name what it does not build.  No compute
call: the tail itself runs in libgdmae_hip.so on the device (tests/test_center_head_detect_gpu.py)."""
import copy
import os
import re

import numpy as np
import pytest
import torch

from gdmae_hip import configs
from gdmae_hip import lib as L

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ['Vehicle', 'Pedestrian', 'Cyclist']
PCR, VS = [0, -7.68, -3, 15.36, 7.68, 1], [0.32, 0.32, 4]


def _head(cfg, names=NAMES):
    from pcdet.models.dense_heads import CenterHead
    grid = np.round((np.array(PCR[3:6]) - np.array(PCR[0:3])) / np.array(VS)).astype(np.int64)
    torch.manual_seed(5)
    return CenterHead(model_cfg=cfg, input_channels=32, num_class=len(names), class_names=list(names), grid_size=grid,
                      point_cloud_range=np.array(PCR, dtype=np.float32), voxel_size=list(VS), predict_boxes_when_training=False).eval()


def _ts_cfg():
    return copy.deepcopy(configs.waymo_two_stage_cfg()[0].DENSE_HEAD)


def _pd(B=1, C=3, H=48, W=48):
    z = lambda c: torch.zeros(B, c, H, W)   # noqa: E731
    return {"hm": z(C), "center": z(2), "center_z": z(1), "dim": z(3), "rot": z(2)}


def test_new_symbols_are_declared_and_bound():
    txt = open(os.path.join(REPO, "include", "gdmae_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = L.load()
    for name in ("gdmae_center_head_detect", "gdmae_center_head_detect_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert len(L.SIGNATURES["gdmae_center_head_detect"][1]) == 32
    # sorted boxes + scores + labels + n + (K, K / 64) mask words, each block aligned
    b = lib.gdmae_center_head_detect_workspace_bytes(3, 500, 7)
    assert b >= 3 * 500 * (7 * 4 + 4 + 4 + 8 * 8) and b < 2 * 3 * 500 * (7 * 4 + 4 + 4 + 8 * 8)
    assert lib.gdmae_center_head_detect_workspace_bytes(3, 1025, 7) == 0          # more candidates than the tail sorts


def test_rows_of_the_padded_output_follow_the_config():
    assert _head(configs.center_head_cfg()).batched_rows() == 500                 # nms_gpu: min(500, 500)
    assert _head(_ts_cfg()).batched_rows() == 500                                 # multi_class_nms: min(500, 200 + 150 + 150)
    cfg = _ts_cfg()
    cfg.POST_PROCESSING.MAX_OBJ_PER_SAMPLE = 40
    cfg.POST_PROCESSING.NMS_CONFIG.NMS_POST_MAXSIZE = [3, 2, 2]
    assert _head(cfg).batched_rows() == 7
    cfg.POST_PROCESSING.NMS_CONFIG.NMS_POST_MAXSIZE = [30, 20, 20]
    assert _head(cfg).batched_rows() == 40
    assert _head(configs.center_head_cfg()).batched_rows(num_cells=12) == 12      # a map with fewer cells than MAX_OBJ_PER_SAMPLE


def test_refusals_by_name_on_a_cpu_head():
    head = _head(configs.center_head_cfg())
    with pytest.raises(NotImplementedError, match="CPU tensors"):
        head.generate_predicted_boxes_batched(1, [_pd()])
    cfg = configs.center_head_cfg()
    cfg.POST_PROCESSING.MAX_OBJ_PER_SAMPLE = 1025
    with pytest.raises(NotImplementedError, match="MAX_OBJ_PER_SAMPLE 1025"):
        _head(cfg).generate_predicted_boxes_batched(1, [_pd()])
    cfg = configs.center_head_cfg()
    cfg.POST_PROCESSING.NMS_CONFIG.NMS_TYPE = 'circle_nms'
    with pytest.raises(NotImplementedError, match="NMS_TYPE circle_nms"):
        _head(cfg).generate_predicted_boxes_batched(1, [_pd()])
    cfg = configs.center_head_cfg()
    cfg.CLASS_NAMES_EACH_HEAD = [['Vehicle'], ['Pedestrian', 'Cyclist']]
    two = _head(cfg)
    assert len(two.heads_list) == 2
    with pytest.raises(NotImplementedError, match="2 heads"):
        two.generate_predicted_boxes_batched(1, [_pd(C=1), _pd(C=2)])
    # the op-by-op tail, the comparator, is what it was: it still takes the two heads' dicts (and needs the device for them)
    assert two.generate_predicted_boxes.__func__ is type(two).generate_predicted_boxes


def test_padded_to_pred_dicts_slices_by_num():
    from pcdet.models.dense_heads import CenterHead
    out = {"pred_boxes": torch.arange(2 * 4 * 7, dtype=torch.float32).view(2, 4, 7), "pred_scores": torch.rand(2, 4),
           "pred_labels": torch.ones(2, 4, dtype=torch.int64), "num": torch.tensor([3, 0], dtype=torch.int32)}
    got = CenterHead.padded_to_pred_dicts(out)
    assert [d["pred_boxes"].shape[0] for d in got] == [3, 0] and torch.equal(got[0]["pred_scores"], out["pred_scores"][0, :3])
    assert got[1]["pred_labels"].dtype == torch.int64 and got[1]["pred_boxes"].shape == (0, 7)
