"""Golden for the ONCE evaluator: the reference's ``get_evaluation_results`` and its own ``compute_iou3d``, ``filter_data``,
``accumulate_scores``, ``get_thresholds`` and ``compute_statistics`` (pcdet/datasets/once/once_eval/evaluation.py with iou_utils.py and
eval_utils.py, all imported UNMODIFIED from where they lie) on the seeded scene of tests/once_eval_reference.py ``golden_scene``.
Build container only (reads the reference tree); holds none of its text; never run by a test.

Stand-ins (numba is not installed): ``numba`` with ``jit`` as the identity decorator (bare and with arguments) and ``float32``;
``numba.cuda`` with ``jit`` as the identity and ``local.array`` / ``shared.array`` returning fp32 zeros; the kernel launch of
``rotate_iou_gpu_eval`` replaced by a pair loop over the reference's own ``devRotateIoUEval`` on fp32 rows.  So the reference's polygon
arithmetic runs in numpy fp32 scalars instead of CUDA fp32: "the reference under the stub".  ``num_parts`` is the number of frames,
so that the pair loop runs per frame; the per-frame overlaps do not depend on it.

The fixture holds the annos and, for (use_superclass, ap_with_heading) = (True, True) ``sh``, (False, True) ``nh``, (True, False)
``s_``: the reference's per-frame ``ious`` (concatenated, GT-major), its flags (C, bands, rows), per combo ``num_valid_gt``, the
threshold list ((K, 64) fp64, 0 behind the count) and tp / fp / fn ((K, 64, 3)), the keys and values of ``ret_dict`` and the text."""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd"), HERE, os.path.join(REPO, "tests")]
REF = "/root/reference"
MODE = 'Overall&Distance'
CONFIGS = {'sh': (True, True), 'nh': (False, True), 's_': (True, False)}
SLOTS = 64


def golden_scene():
    """Runs BEFORE the reference's namespace modules are installed: the builder imports this repository's ``pcdet``."""
    import once_eval_reference as kr
    gt_annos, pred_annos = kr.golden_scene()
    statements = {}
    for tag, (sup, heading) in CONFIGS.items():
        _, _, st = statements[tag] = kr.statement(gt_annos, pred_annos, kr.FIVE, use_superclass=sup, ap_with_heading=heading)
        for flags in (st['flag_gt'], st['flag_pred']):
            for c in range(flags.shape[0]):
                assert set(np.unique(flags[c, 0]).tolist()) == {-1, 0}, (tag, c)                       # "overall" ignores nothing
                for b in range(1, 4):
                    assert set(np.unique(flags[c, b]).tolist()) == {-1, 0, 1}, (tag, c, b)
    names = set(n for a in gt_annos for n in a['name'])
    assert set(kr.FIVE) < names and len(names) == 6, names                                              # the five and an unknown one
    st = statements['sh'][2]
    matched = (st['matched'] > -np.inf).sum(axis=1)
    assert matched[0] > 51 and st['n_thresholds'][0] < matched[0], matched                              # the rule skips Vehicle scores
    lone = np.nonzero(st['num_valid'] == 1)[0]
    assert lone.size == 1 and matched[lone[0]] == 1 and st['n_thresholds'][lone[0]] == 51               # 51 copies of one score
    return gt_annos, pred_annos, kr.pack_annos(gt_annos, pred_annos), statements, kr.FIVE


def install_stubs():
    for k in [k for k in sys.modules if k == "pcdet" or k.startswith("pcdet.")]:
        del sys.modules[k]
    for name in ["pcdet", "pcdet.datasets", "pcdet.datasets.once", "pcdet.datasets.once.once_eval"]:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, *name.split("."))]
        sys.modules[name] = m

    def jit(*args, **kw):
        if len(args) == 1 and callable(args[0]) and not kw:
            return args[0]
        return lambda fn: fn
    zeros = lambda shape, dtype=None: np.zeros(shape, np.float32)      # noqa: E731
    numba, cuda = types.ModuleType("numba"), types.ModuleType("numba.cuda")
    numba.jit, numba.float32, numba.cuda = jit, np.float32, cuda
    cuda.jit = jit
    cuda.local, cuda.shared = types.SimpleNamespace(array=zeros), types.SimpleNamespace(array=zeros)
    for m in (numba, cuda):
        sys.modules[m.__name__] = m


def main():
    gt_annos, pred_annos, z, statements, classes = golden_scene()
    install_stubs()
    ev = importlib.import_module("pcdet.datasets.once.once_eval.evaluation")
    ri = importlib.import_module("pcdet.datasets.once.once_eval.iou_utils")
    assert ev.__file__.startswith(REF) and ri.__file__.startswith(REF)

    def rotate_iou_pairs(boxes, query_boxes, criterion=-1, device_id=0):
        boxes, query_boxes = boxes.astype(np.float32), query_boxes.astype(np.float32)
        out = np.zeros((boxes.shape[0], query_boxes.shape[0]), np.float32)
        for n in range(boxes.shape[0]):
            for k in range(query_boxes.shape[0]):
                out[n, k] = ri.devRotateIoUEval(query_boxes[k], boxes[n], criterion)
        return out
    ev.rotate_iou_gpu_eval = rotate_iou_pairs
    F = len(gt_annos)
    worst = 0.0
    for tag, (sup, heading) in CONFIGS.items():
        with np.errstate(all='ignore'):
            ret_str, ret = ev.get_evaluation_results(gt_annos, pred_annos, list(classes), use_superclass=sup, ap_with_heading=heading,
                                                     difficulty_mode=MODE, num_parts=F)
            ious = ev.compute_iou3d(gt_annos, pred_annos, [1] * F, with_heading=heading)
            evaluated = statements[tag][2]['classes']
            thr = ev.superclass_iou_threshold_dict if sup else ev.iou_threshold_dict
            K = len(evaluated) * 4
            flag_gt, flag_pred = [], []
            num_valid, n_thr = np.zeros(K, np.int64), np.zeros(K, np.int64)
            thresholds, table = np.zeros((K, SLOTS), np.float64), np.zeros((K, SLOTS, 3), np.int64)
            for c, cls in enumerate(evaluated):
                for b in range(4):
                    k = c * 4 + b
                    flags = [ev.filter_data(g, p, MODE, difficulty_level=b, class_name=cls, use_superclass=sup) for g, p in zip(gt_annos, pred_annos)]
                    flag_gt.append(np.concatenate([f[0] for f in flags])), flag_pred.append(np.concatenate([f[1] for f in flags]))
                    num_valid[k] = sum(int((f[0] == 0).sum()) for f in flags)
                    scores = np.concatenate([ev.accumulate_scores(ious[f], pred_annos[f]['score'], flags[f][0], flags[f][1], iou_threshold=thr[cls])
                                             for f in range(F)], axis=0)
                    th = ev.get_thresholds(scores, num_valid[k], num_pr_points=50)
                    n_thr[k] = len(th)
                    thresholds[k, :len(th)] = th
                    for f in range(F):
                        for t, score_th in enumerate(th):
                            table[k, t] += ev.compute_statistics(ious[f], pred_annos[f]['score'], flags[f][0], flags[f][1], score_threshold=score_th,
                                                                 iou_threshold=thr[cls])
        st = statements[tag][2]
        for f in range(F):
            if ious[f].size:
                worst = max(worst, float(np.abs(np.nan_to_num(ious[f].astype(np.float64)) - st['overlaps'][f]).max()))
        C = len(evaluated)
        z[tag + "_ious"] = np.concatenate([np.asarray(i, np.float64).reshape(-1) for i in ious])
        z[tag + "_flag_gt"] = np.stack(flag_gt).reshape(C, 4, -1).astype(np.int8)
        z[tag + "_flag_pred"] = np.stack(flag_pred).reshape(C, 4, -1).astype(np.int8)
        z[tag + "_num_valid"], z[tag + "_n_thresholds"], z[tag + "_thresholds"], z[tag + "_table"] = num_valid, n_thr, thresholds, table
        z[tag + "_ret_keys"] = np.array(list(ret.keys()))
        z[tag + "_ret_values"] = np.array([float(v) for v in ret.values()], np.float64)
        z[tag + "_text"] = np.array(ret_str)
        print(tag, ret_str)
    print(f"largest deviation of the reference's fp32-polygon ious from the statement's: {worst:.3e}")
    assert worst < 2.5e-4, worst                                  # a quarter of the scene's 1e-3 margin: "equal" does not rest on luck
    path = os.path.join(HERE, "once_eval.npz")
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB;", F, "frames,", int(z['gt_count'].sum()), "GT rows,",
          int(z['pred_count'].sum()), "predictions")


if __name__ == "__main__":
    main()
