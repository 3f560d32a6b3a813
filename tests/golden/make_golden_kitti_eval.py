"""Golden for the KITTI evaluator: the reference's ``get_official_eval_result`` and ``eval_class``
(pcdet/datasets/kitti/kitti_object_eval_python/eval.py with rotate_iou.py, both imported UNMODIFIED from where they lie) on the seeded
scene of tests/kitti_eval_reference.py ``golden_scene``.  Build container only (reads the reference tree); holds none of its text.

Stand-ins (numba is not installed): ``numba`` with ``jit`` as the identity decorator (bare and with arguments), ``float32`` and
``numba.core.errors``; ``numba.cuda`` with ``jit`` as the identity and ``local.array`` / ``shared.array`` returning fp32 zeros; the
kernel launch of ``rotate_iou_gpu_eval`` replaced by a pair loop over the reference's own ``devRotateIoUEval`` on fp32 rows.  So the
reference's polygon arithmetic runs in numpy fp32 scalars instead of CUDA fp32: "the reference under the stub".

The fixture holds the annos, precision / recall / orientation of ``eval_class`` for the three metrics ((3, C, 3, 2, 41) each), the
keys and values of ``ret_dict`` and the result text, for the classes Car, Pedestrian, Cyclist."""
import os
import sys
import types
import importlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd"), HERE, os.path.join(REPO, "tests")]
REF = "/root/reference"
CLASSES = ['Car', 'Pedestrian', 'Cyclist']


def golden_scene():
    """Runs BEFORE the reference's namespace modules are installed: the builder imports this repository's ``pcdet``."""
    import kitti_eval_reference as kr
    gt_annos, dt_annos = kr.golden_scene()
    _, _, st = kr.statement(gt_annos, dt_annos, CLASSES)
    names = set(n for a in gt_annos for n in a['name'])
    assert {'Car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting', 'DontCare', 'Truck', 'Tram'} <= names, names
    cd = st['clean']
    for flags in (cd['ignored_gt'], cd['ignored_dt']):
        for c in range(3):
            for l in range(3):
                assert set(np.unique(flags[c, l]).tolist()) == {-1, 0, 1}, (c, l)
    matched = (st['matched'] > -np.inf).sum(axis=1)
    assert matched.max() > 41 and (st['n_thresholds'] < matched).any(), matched          # get_thresholds skips scores
    assert st['compute_aos']
    return gt_annos, dt_annos, kr.pack_annos(gt_annos, dt_annos)


def install_stubs():
    for k in [k for k in sys.modules if k == "pcdet" or k.startswith("pcdet.")]:
        del sys.modules[k]
    for name in ["pcdet", "pcdet.datasets", "pcdet.datasets.kitti", "pcdet.datasets.kitti.kitti_object_eval_python"]:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, *name.split("."))]
        sys.modules[name] = m

    def jit(*args, **kw):
        if len(args) == 1 and callable(args[0]) and not kw:
            return args[0]
        return lambda fn: fn
    zeros = lambda shape, dtype=None: np.zeros(shape, np.float32)      # noqa: E731
    numba, cuda, core, errors = (types.ModuleType(n) for n in ("numba", "numba.cuda", "numba.core", "numba.core.errors"))
    numba.jit, numba.float32, numba.cuda, numba.core = jit, np.float32, cuda, core
    cuda.jit = jit
    cuda.local, cuda.shared = types.SimpleNamespace(array=zeros), types.SimpleNamespace(array=zeros)
    core.errors = errors
    errors.NumbaPerformanceWarning = type("NumbaPerformanceWarning", (Warning,), {})
    errors.NumbaDeprecationWarning = type("NumbaDeprecationWarning", (Warning,), {})
    for m in (numba, cuda, core, errors):
        sys.modules[m.__name__] = m


def main():
    gt_annos, dt_annos, z = golden_scene()
    install_stubs()
    ev = importlib.import_module("pcdet.datasets.kitti.kitti_object_eval_python.eval")
    ri = importlib.import_module("pcdet.datasets.kitti.kitti_object_eval_python.rotate_iou")
    assert ev.__file__.startswith(REF) and ri.__file__.startswith(REF)

    def rotate_iou_pairs(boxes, query_boxes, criterion=-1, device_id=0):
        boxes, query_boxes = boxes.astype(np.float32), query_boxes.astype(np.float32)
        out = np.zeros((boxes.shape[0], query_boxes.shape[0]), np.float32)
        for n in range(boxes.shape[0]):
            for k in range(query_boxes.shape[0]):
                out[n, k] = ri.devRotateIoUEval(query_boxes[k], boxes[n], criterion)
        return out
    ev.rotate_iou_gpu_eval = rotate_iou_pairs
    with np.errstate(all='ignore'):
        result, ret = ev.get_official_eval_result(gt_annos, dt_annos, CLASSES)
        mo = np.stack([np.array([[0.7, 0.5, 0.5]] * 3), np.array([[0.7, 0.5, 0.5], [0.5, 0.25, 0.25], [0.5, 0.25, 0.25]])], axis=0)
        per_metric = [ev.eval_class(gt_annos, dt_annos, [0, 1, 2], [0, 1, 2], m, mo, compute_aos=(m == 0)) for m in range(3)]
    for k in ("precision", "recall", "orientation"):
        z["ref_" + k] = np.stack([r[k] for r in per_metric])
    z["ret_keys"] = np.array(list(ret.keys()))
    z["ret_values"] = np.array([float(v) for v in ret.values()], np.float64)
    z["result"] = np.array(result)
    assert "aos  AP:" in result and len(ret) == 36
    path = os.path.join(HERE, "kitti_eval.npz")
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB;", len(gt_annos), "frames,", int(z['gt_count'].sum()), "GT rows,",
          int(z['dt_count'].sum()), "detections")
    print(result)


if __name__ == "__main__":
    main()
