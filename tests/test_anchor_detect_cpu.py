"""CPU: the batched anchor-head tail is declared, bound and sized, and refuses by name what it does not build.  No compute
call: the tail itself runs in libgdmae_hip.so on the device (tests/test_anchor_detect_gpu.py)."""
import logging
import os
import re

import pytest
import torch

from gdmae_hip import configs
from gdmae_hip import lib as L

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("gdmae_anchor_detect", "gdmae_anchor_detect_workspace_bytes")


def _model(cfg_edit=None):
    """the detector of the shipped KITTI fine-tune config on the CPU"""
    from pcdet.models import build_network
    cfg, ds = configs.kitti_finetune_cfg()
    if cfg_edit is not None:
        cfg_edit(cfg.POST_PROCESSING)
    torch.manual_seed(3)
    return build_network(cfg, len(ds.class_names), ds, logging.getLogger("t")).eval()


def _inputs(B=1, A=8):
    return (torch.zeros(B, dtype=torch.int32), torch.zeros(B, A), torch.ones(B, A, dtype=torch.int32), torch.zeros(B, A, 7))


def _align(x, a=256):
    return (x + a - 1) // a * a


def test_new_symbols_are_declared_and_bound():
    txt = open(os.path.join(REPO, "include", "gdmae_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = L.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert len(L.SIGNATURES["gdmae_anchor_detect"][1]) == 16
    assert len(L.SIGNATURES["gdmae_anchor_detect_workspace_bytes"][1]) == 2


@pytest.mark.parametrize("B,pre_max", [(1, 65), (3, 500), (3, 1000), (2, 4096), (8, 4096)])
def test_workspace_size(B, pre_max):
    """sorted boxes + scores + labels + n + (pre_max, ceil(pre_max / 64)) mask words"""
    words = (pre_max + 63) // 64
    blocks = [B * pre_max * 7 * 4, B * pre_max * 4, B * pre_max * 4, B * 4, B * pre_max * words * 8]
    got = L.load().gdmae_anchor_detect_workspace_bytes(B, pre_max)
    assert sum(blocks) <= got < 2 * sum(blocks)
    assert got <= sum(_align(x) for x in blocks)


def test_workspace_size_is_zero_for_what_the_entry_refuses():
    lib = L.load()
    assert lib.gdmae_anchor_detect_workspace_bytes(3, 4097) == 0
    assert lib.gdmae_anchor_detect_workspace_bytes(3, 0) == 0
    assert lib.gdmae_anchor_detect_workspace_bytes(0, 100) == 0
    assert lib.gdmae_anchor_detect_workspace_bytes(3, 4096) > 0


def test_rows_of_the_padded_output_follow_the_config():
    assert _model().batched_rows() == 500                                 # the shipped 4096 / 500

    def small(post):
        post.NMS_CONFIG.NMS_PRE_MAXSIZE, post.NMS_CONFIG.NMS_POST_MAXSIZE = 10, 30
    assert _model(small).batched_rows() == 10


def test_refusals_by_name_on_a_cpu_model():
    with pytest.raises(NotImplementedError, match="CPU tensors"):
        _model().finish_batch(*_inputs())

    def edit(**kw):
        def f(post):
            for k, v in kw.items():
                if k in post.NMS_CONFIG or k == "NMS":
                    post.NMS_CONFIG[k] = v
                else:
                    post[k] = v
        return f
    for kw, match in ((dict(NMS_PRE_MAXSIZE=4097), "NMS_PRE_MAXSIZE 4097"), (dict(MULTI_CLASSES_NMS=True), "MULTI_CLASSES_NMS"),
                      (dict(NMS_TYPE="nms_normal_gpu"), "NMS_TYPE nms_normal_gpu"), (dict(OUTPUT_RAW_SCORE=True), "OUTPUT_RAW_SCORE"),
                      (dict(NMS=False), "NMS: False")):
        m = _model(edit(**kw))
        with pytest.raises(NotImplementedError, match=match):
            m.finish_batch(*_inputs())
        with pytest.raises(NotImplementedError, match=match):
            m.batched_rows()


def test_padded_to_pred_dicts_slices_by_num():
    from pcdet.models.detectors.detector3d_template import Detector3DTemplate
    out = {"pred_boxes": torch.arange(2 * 4 * 7, dtype=torch.float32).view(2, 4, 7), "pred_scores": torch.rand(2, 4),
           "pred_labels": torch.ones(2, 4, dtype=torch.int64), "num": torch.tensor([3, 0], dtype=torch.int32)}
    got = Detector3DTemplate.padded_to_pred_dicts(out)
    assert [d["pred_boxes"].shape[0] for d in got] == [3, 0] and torch.equal(got[0]["pred_scores"], out["pred_scores"][0, :3])
    assert got[1]["pred_labels"].dtype == torch.int64 and got[1]["pred_boxes"].shape == (0, 7)
