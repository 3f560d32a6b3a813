"""CPU: the numpy statement of the KITTI annos (``gdmae_hip.evaluation.kitti_annos_numpy``) against the reference's recorded
per-sample dicts (tests/golden/kitti_annos.npz, made by tests/golden/make_golden_kitti_annos.py), and the host-side pieces around it.

The reference computes in fp32 (through BLAS for the two matrix products) and rounds the corners to fp32 before it projects them;
the statement computes in fp64 and rounds once.  ``name``, ``dimensions``, ``score``, ``boxes_lidar`` and every clipped ``bbox``
entry are EQUAL; which entries are clipped is equal.  The rest, measured here on the CPU against the golden (63 rows, depths 0.2 ..
75 m), the largest figure over the scene:
  location, relative to max(|value|, 1)   1.822e-7     three fp32 roundings of a sum of products
  rotation_y                              2.385e-7     one fp32 ulp at 4 .. 8 rad
  alpha                                   9.537e-7     two fp32 ulps at 4 .. 8 rad: atan2, the sum
  bbox, pixels                            1.336e-4     fp32 corners at 1e3 px and 1e1 m: ulp(1e3) = 6.1e-5
The tests assert 4 x these figures.

The label-file text: a line is '%.4f' of values that differ from the reference's by up to the figures above, so a digit in the fourth
decimal can differ.  The lines must equal the lines formatted HERE (``label_line``) from the same annos; against lines formatted from
the golden values the name and the '-1 -1' fields are equal, the fields of the equal keys (dimensions, score, clipped bbox entries) are
equal as text, and every other field is within its bound above plus the 1e-4 of the print."""
import os
import re

import numpy as np
import pytest
import torch

import kitti_annos_reference as ka
from gdmae_hip import evaluation
from gdmae_hip import lib as L

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MEASURED = {'location': 1.822e-7, 'rotation_y': 2.385e-7, 'alpha': 9.537e-7, 'bbox': 1.336e-4}


def golden():
    z = np.load(os.path.join(REPO, "tests", "golden", "kitti_annos.npz"))
    frames, ref = ka.unpack_golden(z)
    return frames, ref, ka.golden_scene()[1]


def clip_limits(frame):
    h, w = ka.SHAPES[frame['calib']]
    return np.array([w - 1, h - 1, w - 1, h - 1], np.float32)


def deviation(key, got, want):
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    return d / np.maximum(np.abs(want.astype(np.float64)), 1.0) if key == 'location' else d


def label_line(anno, i):
    """the reference's label-file line, written out once more: name, -1 -1, alpha, bbox, h w l, location, rotation_y, score"""
    v = [anno['alpha'][i], *anno['bbox'][i], anno['dimensions'][i][1], anno['dimensions'][i][2], anno['dimensions'][i][0], *anno['location'][i],
         anno['rotation_y'][i], anno['score'][i]]
    return ' '.join([str(anno['name'][i]), '-1', '-1'] + ['%.4f' % x for x in v])


def test_the_golden_scene_is_the_builders_scene_and_reaches_its_edges():
    frames, ref, names = golden()
    built, _ = ka.golden_scene()
    got = set()
    for f, g in zip(frames, built):
        assert f['calib'] == g['calib'] and all(np.array_equal(f[k], g[k]) for k in ('boxes', 'scores', 'labels'))
        assert ka.rows_hold(f['boxes'], ka.CALIBS[f['calib']], ka.SHAPES[f['calib']]).all()
        got |= ka.reached(f)
    assert got == ka.EDGES, ka.EDGES - got
    assert {f['calib'] for f in frames} == {0, 1, 2} and any(len(f['scores']) == 0 for f in frames)
    assert set(n for r in ref if r is not None for n in r['name']) == set(ka.THREE) and ka.SWAPPED in names
    # the labels of the swapped frame mean another class than under KITTI's order
    swapped = names.index(ka.SWAPPED)
    assert set(frames[swapped]['labels'].tolist()) == {1, 2} and set(ref[swapped]['name']) == {'Pedestrian', 'Car'}
    assert (ref[swapped]['name'][frames[swapped]['labels'] == 1] == 'Pedestrian').all()


def test_statement_against_the_golden():
    frames, ref, names = golden()
    worst, clipped_entries = {}, 0
    for f, r, cn in zip(frames, ref, names):
        a = ka.statement(f, cn)
        if r is None:
            assert len(a['score']) == 0
            continue
        hi = clip_limits(f)
        for k in ('name', 'dimensions', 'score', 'boxes_lidar', 'truncated', 'occluded'):
            assert np.array_equal(a[k], r[k]), k
        for k in ('alpha', 'bbox', 'dimensions', 'location', 'rotation_y', 'score', 'boxes_lidar'):
            assert a[k].dtype == np.float32 and a[k].shape == r[k].shape, k
        clipped = (r['bbox'] == 0) | (r['bbox'] == hi)
        assert np.array_equal((a['bbox'] == 0) | (a['bbox'] == hi), clipped) and np.array_equal(a['bbox'][clipped], r['bbox'][clipped])
        clipped_entries += int(clipped.sum())
        for k in MEASURED:
            worst[k] = max(worst.get(k, 0.0), float(deviation(k, a[k], r[k]).max()))
    print("statement against the golden:", {k: f"{v:.3e}" for k, v in worst.items()}, f"{clipped_entries} clipped entries")
    assert clipped_entries > 8
    for k, m in MEASURED.items():
        assert worst[k] <= 4 * m, (k, worst[k])


def test_clean_data_on_the_statements_annos_reaches_every_flag():
    frames, _, names = golden()
    annos = [ka.statement(f, cn) for f, cn in zip(frames, names)]
    classes = evaluation.kitti_class_ints(ka.THREE)
    cd = evaluation.kitti_clean_dt(annos, classes)
    assert cd['ignored_dt'].shape == (3, 3, sum(len(f['scores']) for f in frames))
    for c in range(3):
        for l in range(3):
            assert set(np.unique(cd['ignored_dt'][c, l]).tolist()) == {-1, 0, 1}, (c, l)
    # the whole of kitti_clean_data is its two halves
    gt = [{k: v[:0] for k, v in a.items()} for a in annos]
    both = evaluation.kitti_clean_data(gt, annos, classes)
    assert np.array_equal(both['ignored_dt'], cd['ignored_dt']) and np.array_equal(both['dt_off'], cd['dt_off'])
    assert sorted(both) == ['dc_off', 'dc_rows', 'dt_off', 'gt_off', 'ignored_dt', 'ignored_gt', 'num_valid']


def test_duck_typed_calibrations_give_equal_results():
    frames, _, names = golden()
    for f, cn in zip(frames[:3], names):
        d = ka.CALIBS[f['calib']]
        a, b = ka.statement(f, cn, calib=d), ka.statement(f, cn, calib=ka.CalibObject(d))
        c = ka.statement(f, cn, calib={k: v.astype(np.float64).tolist() for k, v in d.items()})
        for k in ka.ANNO_KEYS:
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    assert np.array_equal(evaluation.kitti_pack_calib(ka.CalibObject(ka.CALIBS[1]), ka.SHAPES[1])[:33],
                          np.concatenate([ka.CALIBS[1][k].reshape(-1) for k in ('P2', 'R0', 'Tr_velo2cam')]))
    assert evaluation.kitti_pack_calib(ka.CALIBS[1], ka.SHAPES[1])[33:].tolist() == [370.0, 1224.0, 0.0]


def test_zero_rows_give_the_empty_template():
    a = evaluation.kitti_annos_numpy(np.zeros((0, 7), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64), ka.CALIBS[0], ka.SHAPES[0], ka.THREE)
    assert sorted(a) == sorted(ka.ANNO_KEYS)
    for k in ka.ANNO_KEYS:
        assert a[k].dtype == np.float64 and a[k].shape == ((0, 4) if k == 'bbox' else (0, 3) if k in ('dimensions', 'location') else (
            0, 7) if k == 'boxes_lidar' else (0,)), k
    t = evaluation.kitti_annos_template(3)
    assert t['bbox'].shape == (3, 4) and t['boxes_lidar'].shape == (3, 7) and not any(v.any() for v in t.values())


def test_prediction_dicts_on_cpu_tensors_and_their_label_files(tmp_path):
    frames, ref, names = golden()
    frames, ref = frames[:5], ref[:5]                                   # the frames of one class_names list
    bd = ka.batch_dict(frames, first_id=7)
    pred = [{'pred_boxes': torch.from_numpy(f['boxes']), 'pred_scores': torch.from_numpy(f['scores']), 'pred_labels': torch.from_numpy(f['labels'])}
            for f in frames]
    annos = evaluation.kitti_prediction_dicts(bd, pred, ka.THREE, output_path=tmp_path)
    assert [a['frame_id'] for a in annos] == bd['frame_id'] == ['%06d' % i for i in range(7, 12)]
    same_text = all_fields = 0
    for f, r, a, fid in zip(frames, ref, annos, bd['frame_id']):
        want = ka.statement(f, ka.THREE)
        assert all(np.array_equal(a[k], want[k]) for k in ka.ANNO_KEYS)
        lines = open(os.path.join(tmp_path, fid + '.txt')).read().split('\n')
        assert lines[-1] == '' and len(lines) == len(f['scores']) + 1
        assert lines[:-1] == [label_line(a, i) for i in range(len(f['scores']))] == evaluation.kitti_label_lines(a)
        if r is None:
            continue
        hi = clip_limits(f)
        # the fields of a line: name -1 -1 alpha x1 y1 x2 y2 h w l x y z rotation_y score
        bound = [MEASURED['alpha']] + [MEASURED['bbox']] * 4 + [0.0] * 3 + [MEASURED['location']] * 3 + [MEASURED['rotation_y'], 0.0]
        for i, line in enumerate(lines[:-1]):
            got, gold = line.split(' '), label_line(r, i).split(' ')
            assert got[:3] == gold[:3] == [str(r['name'][i]), '-1', '-1'] and len(got) == len(gold) == 16
            clipped = [False] + [bool(r['bbox'][i][j] in (0.0, hi[j])) for j in range(4)] + [False] * 8
            for j in range(13):
                all_fields += 1
                same_text += got[3 + j] == gold[3 + j]
                if bound[j] == 0.0 or clipped[j]:
                    assert got[3 + j] == gold[3 + j], (fid, i, j)
                else:
                    scale = max(abs(float(gold[3 + j])), 1.0) if 8 <= j <= 10 else 1.0
                    assert abs(float(got[3 + j]) - float(gold[3 + j])) <= 4 * bound[j] * scale + 1.0001e-4, (fid, i, j, got[3 + j], gold[3 + j])
    print(f"label files: {same_text} of {all_fields} numeric fields are the same text as the golden's")
    assert same_text > 0.9 * all_fields


def test_the_new_symbol_is_declared_and_bound():
    txt = open(os.path.join(REPO, "include", "gdmae_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = L.load()
    assert re.search(r"\bgdmae_kitti_annos\s*\(", txt)
    assert "gdmae_kitti_annos" in L.SIGNATURES and hasattr(lib, "gdmae_kitti_annos")
    assert len(L.SIGNATURES["gdmae_kitti_annos"][1]) == 22
    src = open(os.path.join(REPO, "gd-mae_amd", "gdmae_hip", "build.py")).read()
    assert '"kitti_annos.hip"' in src and os.path.exists(os.path.join(REPO, "gd-mae_amd", "csrc", "kitti_annos.hip"))


def test_the_entry_refuses_before_anything_is_launched():
    """rows > 1024, a negative frame count, null pointers: non-zero with the entry's name in the message; nothing touches a device"""
    lib = L.load()
    one = L.host_i32([0])
    fake = 256                                                             # a non-null pointer that a refused call never reads

    def refused(F, rows, stride=7, ptrs=fake, class_map=one, n_names=1, classes=one, n_classes=1, nd=1):
        rc = lib.gdmae_kitti_annos(ptrs, stride, ptrs, ptrs, ptrs, ptrs, ptrs, F, rows, nd, class_map, n_names, classes, n_classes,
                                   ptrs, ptrs, ptrs, ptrs, ptrs, ptrs, ptrs, None)
        return rc != 0 and b"kitti_annos" in lib.gdmae_last_error()
    assert refused(1, 1025) and refused(1, 0) and refused(-1, 500)
    assert refused(1, 500, ptrs=None) and refused(1, 500, class_map=None) and refused(1, 500, classes=None)
    assert refused(1, 500, stride=6) and refused(1, 500, n_names=17) and refused(1, 500, n_classes=7) and refused(1, 500, nd=-1)
    assert lib.gdmae_kitti_annos(fake, 7, fake, fake, fake, fake, fake, 0, 500, 0, one, 1, one, 1, fake, fake, fake, fake, fake, fake, fake, None) == 0


def test_the_record_refuses_by_name():
    with pytest.raises(NotImplementedError, match="KittiDetections"):
        evaluation.KittiDetections(ka.THREE, "cpu")
    assert evaluation.kitti_class_map(['Pedestrian', 'car', 'Tram']) == [1, 0, -1]
