"""Golden for the KITTI annos of the detections: the reference's per-sample dicts of ``KittiDataset.generate_prediction_dicts``
on the seeded scene of tests/kitti_annos_reference.py ``golden_scene``, computed by the reference's own
``box_utils.boxes3d_lidar_to_kitti_camera`` / ``boxes3d_kitti_camera_to_imageboxes`` (pcdet/utils/box_utils.py) and ``Calibration``
(pcdet/utils/calibration_kitti.py), both imported UNMODIFIED from where they lie, on the lidar boxes and a dict calibration.  Build
container only (reads the reference tree); holds none of its text.

    python tests/golden/make_golden_kitti_annos.py <root of the reference tree>

Stand-ins: ``pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils`` and ``pcdet.utils.common_utils`` (a compiled extension and its users;
neither function above calls them) as empty modules, and ``scipy`` / ``scipy.spatial.Delaunay`` when scipy is not installed.

The fixture holds the inputs (boxes, scores, labels, calibration index, counts per frame) and the reference's outputs per key, rows
concatenated over the frames that have rows."""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd"), HERE, os.path.join(REPO, "tests")]


def scene():
    """Runs BEFORE the reference's namespace modules are installed: the builder imports this repository's ``pcdet``."""
    import kitti_annos_reference as ka
    frames, names = ka.golden_scene()
    got = set()
    for f in frames:
        assert ka.rows_hold(f['boxes'], ka.CALIBS[f['calib']], ka.SHAPES[f['calib']]).all()
        got |= ka.reached(f)
    assert got == ka.EDGES, ka.EDGES - got
    return ka, frames, names


def install_stubs(ref):
    for k in [k for k in sys.modules if k == "pcdet" or k.startswith("pcdet.")]:
        del sys.modules[k]
    for name in ["pcdet", "pcdet.utils"]:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(ref, *name.split("."))]
        sys.modules[name] = m
    for name in ["pcdet.ops", "pcdet.ops.roiaware_pool3d", "pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils", "pcdet.utils.common_utils"]:
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    sys.modules["pcdet.ops.roiaware_pool3d"].roiaware_pool3d_utils = sys.modules["pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils"]
    sys.modules["pcdet.utils"].common_utils = sys.modules["pcdet.utils.common_utils"]
    try:
        import scipy.spatial      # noqa: F401
    except ImportError:
        scipy, spatial = types.ModuleType("scipy"), types.ModuleType("scipy.spatial")
        scipy.spatial, spatial.Delaunay = spatial, object
        sys.modules["scipy"], sys.modules["scipy.spatial"] = scipy, spatial


def main():
    ref = os.path.abspath(sys.argv[1])
    ka, frames, names = scene()
    install_stubs(ref)
    box_utils = importlib.import_module("pcdet.utils.box_utils")
    calibration = importlib.import_module("pcdet.utils.calibration_kitti")
    assert box_utils.__file__.startswith(ref) and calibration.__file__.startswith(ref)
    annos = []
    for f, class_names in zip(frames, names):
        n = len(f['scores'])
        if n == 0:
            annos.append({'score': np.zeros(0)})
            continue
        calib = calibration.Calibration(ka.CALIBS[f['calib']], None)
        boxes = f['boxes'].copy()
        camera = box_utils.boxes3d_lidar_to_kitti_camera(boxes, calib)
        image = box_utils.boxes3d_kitti_camera_to_imageboxes(camera, calib, image_shape=np.array(ka.SHAPES[f['calib']]))
        assert np.array_equal(boxes, f['boxes'])
        # The dict is assembled here, key by key as generate_single_sample_dict fills it: kitti_dataset.py itself cannot be imported
        # without the dataset's dependencies.  alpha is `rotation_y - arctan2(-y, x)`, which is bit for bit the reference's
        # `-arctan2(-y, x) + rotation_y` in IEEE fp32 (a + b = b + a, and the negation is exact).
        annos.append({'name': np.array(class_names)[f['labels'] - 1], 'truncated': np.zeros(n), 'occluded': np.zeros(n),
                      'alpha': camera[:, 6] - np.arctan2(-boxes[:, 1], boxes[:, 0]), 'bbox': image, 'dimensions': camera[:, 3:6],
                      'location': camera[:, 0:3], 'rotation_y': camera[:, 6], 'score': f['scores'], 'boxes_lidar': boxes})
    z = ka.pack_golden(frames, annos)
    path = os.path.join(HERE, "kitti_annos.npz")
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), "bytes;", len(frames), "frames,", int(z['count'].sum()), "rows;",
          {k: str(z['ref_' + k].dtype) for k in ka.ANNO_KEYS})


if __name__ == "__main__":
    main()
