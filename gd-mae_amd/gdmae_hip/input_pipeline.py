"""On-GPU input pipeline (SURVEY §8 "next" row f2): the reference's per-frame numpy chain of the SSL configuration

    random_world_flip -> random_world_rotation -> random_world_scaling      (data_augmentor.py:54-143)
    mask_points_and_boxes_outside_range -> shuffle_points                   (data_processor.py:77-100)
    collate_batch (batch index prepended, frames concatenated)              (dataset.py:181-186)

as ONE HIP pass over the raw frames (gdmae_augment_collate) + one row permutation.  The random decisions are drawn
on the host with the same ``np.random`` calls, in the same order, as the reference (so a seeded run sees the same
flips / angles / scales); the shuffle is a device-side random permutation within each frame (``torch.rand`` keys),
or an explicit permutation for parity tests.  No fallback: without libgdmae_hip.so this raises.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import lib as L

# tools/cfgs/waymo_models/gd_mae_ssl.yaml:18-31
SSL_AUG_CONFIG = (
    {"NAME": "random_world_flip", "PROBABILITY": 0.5, "ALONG_AXIS_LIST": ["x", "y"]},
    {"NAME": "random_world_rotation", "PROBABILITY": 1.0, "WORLD_ROT_ANGLE": [-0.78539816, 0.78539816]},
    {"NAME": "random_world_scaling", "PROBABILITY": 1.0, "WORLD_SCALE_RANGE": [0.95, 1.05]},
)


def draw_world_params(aug_config: Sequence[dict] = SSL_AUG_CONFIG) -> dict:
    """Random world transformation of ONE frame; consumes ``np.random`` exactly like DataAugmentor.forward does
    (data_augmentor.py:62, :97-101, :123-127) so that seeded runs agree with the reference."""
    out = {"flip_x": False, "flip_y": False, "angle": 0.0, "scale": 1.0}
    for cfg in aug_config:
        p = cfg["PROBABILITY"]
        if cfg["NAME"] == "random_world_flip":
            for axis in cfg["ALONG_AXIS_LIST"]:
                if np.random.choice([False, True], replace=False, p=[1 - p, p]):
                    if axis not in ("x", "y"):
                        raise NotImplementedError(axis)
                    out["flip_" + axis] = True
        elif cfg["NAME"] == "random_world_rotation":
            enable = np.random.choice([False, True], replace=False, p=[1 - p, p])
            lo, hi = cfg["WORLD_ROT_ANGLE"] if enable else (0.0, 0.0)
            out["angle"] = float(np.random.uniform(lo, hi))
        elif cfg["NAME"] == "random_world_scaling":
            enable = np.random.choice([False, True], replace=False, p=[1 - p, p])
            lo, hi = cfg["WORLD_SCALE_RANGE"] if enable else (1.0, 1.0)
            out["scale"] = float(np.random.uniform(lo, hi))
        else:
            raise NotImplementedError(f"augmentation {cfg['NAME']} is outside the SSL pre-training configuration")
    return out


def params_table(params: Sequence[dict]) -> np.ndarray:
    """(B, 8) fp32 rows [flip_x, flip_y, cos, sin, scale, 0, 0, 0]: cos / sin evaluated in fp64 and rounded to fp32
    (rotate_points_along_z: torch.cos on the float64 angle, ``.float()``), scale rounded to fp32 (in-place multiply of
    a float32 array by a python float)."""
    t = np.zeros((len(params), 8), np.float32)
    for i, p in enumerate(params):
        a = np.float64(p["angle"])
        t[i, :5] = (float(p["flip_x"]), float(p["flip_y"]), np.float32(np.cos(a)), np.float32(np.sin(a)), np.float32(p["scale"]))
    return t


class GpuInputPipeline:
    def __init__(self, point_cloud_range, aug_config: Optional[Sequence[dict]] = SSL_AUG_CONFIG, shuffle: bool = True,
                 device: Optional[torch.device] = None):
        r = [float(v) for v in point_cloud_range]
        self.xy_range = (r[0], r[1], r[3], r[4])
        self.aug_config = aug_config
        self.shuffle = shuffle
        self.device = device or torch.device("cuda", torch.cuda.current_device())

    def _staging(self, n_elems: int) -> torch.Tensor:
        """Pinned host staging buffer, allocated once and grown geometrically (page-locking is slow)."""
        buf = getattr(self, "_pinned", None)
        if buf is None or buf.numel() < n_elems:
            buf = self._pinned = torch.empty(int(n_elems * 1.25) + 1024, dtype=torch.float32).pin_memory()
        ev = getattr(self, "_copied", None)
        if ev is not None:
            ev.synchronize()                        # previous batch's H2D copy has left the buffer
        return buf[:n_elems]

    def __call__(self, frames: List[np.ndarray], params: Optional[Sequence[dict]] = None,
                 perms: Optional[Sequence[np.ndarray]] = None) -> torch.Tensor:
        """frames: B raw clouds (n_i, F) float32 (x, y, z, features...).  Returns the collated batch (N, 1 + F) on the
        device.  ``params`` / ``perms``: explicit world transformations and per-frame permutations of the KEPT points
        (parity tests); by default they are drawn (np.random for the world parameters, torch.rand keys for the order)."""
        B = len(frames)
        F = int(frames[0].shape[1])
        if params is None:
            ident = {"flip_x": False, "flip_y": False, "angle": 0.0, "scale": 1.0}
            params = [draw_world_params(self.aug_config) if self.aug_config else dict(ident) for _ in range(B)]
        off = np.zeros(B + 1, np.int32)
        off[1:] = np.cumsum([f.shape[0] for f in frames])
        n_raw = int(off[-1])
        host = self._staging(max(n_raw, 1) * F).view(-1, F)[:max(n_raw, 1)]
        hv = host.numpy()
        for i, f in enumerate(frames):
            assert f.dtype == np.float32 and f.shape[1] == F
            hv[off[i]:off[i + 1]] = f
        dev = self.device
        raw = host.to(dev, non_blocking=True)
        self._copied = torch.cuda.Event()
        self._copied.record()                       # the staging buffer is reused by the next call
        off_d = torch.from_numpy(off).to(dev, non_blocking=True)
        tab_d = torch.from_numpy(params_table(params)).to(dev, non_blocking=True)
        out = torch.empty(max(n_raw, 1), 1 + F, dtype=torch.float32, device=dev)
        kept = torch.empty(B + 1, dtype=torch.int32, device=dev)
        ws = torch.empty(L.load().gdmae_augment_collate_workspace_bytes(n_raw), dtype=torch.uint8, device=dev)
        L.call("gdmae_augment_collate", L.ptr(raw), n_raw, F, L.ptr(off_d), B, L.ptr(tab_d), L.host_f32(self.xy_range), L.ptr(out),
               L.ptr(kept), L.ptr(ws), L.stream())
        kept_h = kept.tolist()                      # the one host sync of the pipeline (it runs a batch ahead)
        n = kept_h[B]
        for b in range(B - 1, -1, -1):              # empty frames: first row = that of the next frame
            if kept_h[b] < 0:
                kept_h[b] = kept_h[b + 1]
        pts = out[:n]
        if perms is not None:
            idx = torch.cat([torch.from_numpy(np.asarray(p, np.int64)) + kept_h[b] for b, p in enumerate(perms)]).to(dev)
        elif self.shuffle and n > 0:
            # random order within each frame: sort by (frame index + U[0,1))
            idx = torch.argsort(pts[:, 0] + torch.rand(n, device=dev))      # fp32 keys: 2^-20 resolution at B <= 8
        else:
            return pts
        return pts.index_select(0, idx)             # rows are 4 * (1 + F) = 20-24 bytes: below the 16-byte row kernels


# ---------------------------------------------------------------------------------------------------------------------
# Fine-tune mode: gt_sampling + the world augmentation of points AND boxes + range masks + collate
#
#     gt_sampling -> random_world_flip -> random_world_rotation -> random_world_scaling -> heading limit_period
#       -> class selection + class column -> mask_points_and_boxes_outside_range -> shuffle_points -> collate_batch
#
# (database_sampler.py, data_augmentor.py, dataset.py:125-162 / :181-192, data_processor.py:77-90).  The host draws what
# the reference draws, with the same np.random calls in the same order (per frame: the candidates of every sample
# group, then the world parameters); the two launches of csrc/gt_sampling.hip do the rest.
# ---------------------------------------------------------------------------------------------------------------------
# tools/cfgs/waymo_models/gd_mae.yaml:18-55
FINETUNE_AUG_CONFIG = ({"NAME": "gt_sampling", "BACKEND": {"NAME": "HardDiskBackend"}, "USE_ROAD_PLANE": False,
        "DB_INFO_PATH": ["waymo_processed_data_waymo_dbinfos_train_sampled_1.pkl"], "USE_SHARED_MEMORY": False,
        "DB_DATA_PATH": ["waymo_processed_data_gt_database_train_sampled_1_global.npy"],
        "PREPARE": {"filter_by_min_points": ["Vehicle:5", "Pedestrian:10", "Cyclist:10"], "filter_by_difficulty": [-1]},
        "SAMPLE_GROUPS": ["Vehicle:15", "Pedestrian:10", "Cyclist:10"], "NUM_POINT_FEATURES": 5, "REMOVE_POINTS": True,
        "REMOVE_EXTRA_WIDTH": [0.0, 0.0, 0.0], "LIMIT_WHOLE_SCENE": True},
       {"NAME": "random_world_flip", "PROBABILITY": 0.5, "ALONG_AXIS_LIST": ["x", "y"]},
       {"NAME": "random_world_rotation", "PROBABILITY": 1.0, "WORLD_ROT_ANGLE": [-0.78539816, 0.78539816]},
       {"NAME": "random_world_scaling", "PROBABILITY": 1.0, "WORLD_SCALE_RANGE": [0.95, 1.05]})

MAX_CANDIDATES = 64         # per frame (csrc/gt_sampling.hip: GS_MAX_CAND; the library also refuses more than 448 GT boxes)


class GtDatabase:
    """The GT database of ``gt_sampling`` in its ``*_global.npy`` form: ``points`` (N, F) float32 holds every object's
    LOCAL points (box centre subtracted, not rotated) back to back, ``offsets`` (M, 2) the row range of every entry,
    ``boxes`` (M, 7) its ``box3d_lidar``, ``names`` (M) its class.  ``class_index[name]`` lists the entries of a class
    in file order: the list the reference's sampler indexes (``db_infos[name]``)."""

    def __init__(self, points, offsets, boxes, names, num_points_in_gt=None, difficulty=None):
        if offsets is None:
            raise NotImplementedError("database without global offsets: only the *_global.npy form (global_data_offset) is supported")
        self.points = np.ascontiguousarray(points, dtype=np.float32)
        self.offsets = np.asarray(offsets, dtype=np.int64).reshape(-1, 2)
        boxes = np.asarray(boxes)
        if boxes.ndim == 2 and boxes.shape[1] > 7:
            raise NotImplementedError("GT boxes with more than 7 columns (velocities) are not supported")
        self.boxes = boxes.reshape(-1, 7).astype(np.float32)
        self.names = np.asarray(names).astype(str).reshape(-1)
        M = self.offsets.shape[0]
        assert self.points.ndim == 2 and self.boxes.shape[0] == M and self.names.shape[0] == M
        assert M == 0 or (self.offsets.min() >= 0 and self.offsets.max() <= self.points.shape[0] and (self.offsets[:, 0] <= self.offsets[:, 1]).all())
        self.num_points_in_gt = None if num_points_in_gt is None else np.asarray(num_points_in_gt, dtype=np.int64).reshape(-1)
        self.difficulty = None if difficulty is None else np.asarray(difficulty, dtype=np.int64).reshape(-1)
        self.class_index = {}
        for n in dict.fromkeys(self.names.tolist()):
            self.class_index[n] = np.flatnonzero(self.names == n)
        self.points_dev = None

    @classmethod
    def from_reference_files(cls, info_pkl_paths, global_npy_path):
        """The reference's ``*_dbinfos_*.pkl`` ({class: [info, ...]}; several files extend every class's list, as
        database_sampler.py:31-34 does) and its ``*_gt_database_*_global.npy``."""
        import pickle
        per_class = {}
        for path in ([info_pkl_paths] if isinstance(info_pkl_paths, (str, bytes)) or hasattr(info_pkl_paths, "__fspath__") else info_pkl_paths):
            with open(path, "rb") as f:
                for name, infos in pickle.load(f).items():
                    per_class.setdefault(name, []).extend(infos)
        infos = [i for lst in per_class.values() for i in lst]
        if any("global_data_offset" not in i for i in infos):
            raise NotImplementedError("database without global offsets: an info has no global_data_offset")
        return cls(np.load(global_npy_path), [i["global_data_offset"] for i in infos] or np.zeros((0, 2)),
                   np.stack([np.asarray(i["box3d_lidar"]) for i in infos]) if infos else np.zeros((0, 7)),
                   [i["name"] for i in infos], [i.get("num_points_in_gt", -1) for i in infos], [i.get("difficulty", 0) for i in infos])

    def _select(self, keep):
        pick = lambda a: None if a is None else a[keep]      # noqa: E731
        db = GtDatabase(self.points, self.offsets[keep], self.boxes[keep], self.names[keep], pick(self.num_points_in_gt), pick(self.difficulty))
        db.points_dev = self.points_dev
        return db

    def prepare(self, prepare_cfg):
        """``PREPARE`` of the sampler config, in its key order (database_sampler.py:36-37, :93-120)."""
        db = self
        for func, val in dict(prepare_cfg or {}).items():
            if func == "filter_by_min_points":
                if db.num_points_in_gt is None:
                    raise ValueError("filter_by_min_points needs the database's num_points_in_gt")
                keep = np.ones(db.names.shape[0], bool)
                for name_num in val:
                    name, num = name_num.split(":")
                    if int(num) > 0:
                        keep &= ~((db.names == name) & (db.num_points_in_gt < int(num)))
            elif func == "filter_by_difficulty":
                if db.difficulty is None:
                    raise ValueError("filter_by_difficulty needs the database's difficulty")
                keep = ~np.isin(db.difficulty, np.asarray(list(val), dtype=np.int64))
            else:
                raise NotImplementedError(f"PREPARE step {func}")
            db = db._select(keep)
        return db

    def to(self, device):
        """Resident mode: the object points live on the device, a batch copies none of them."""
        self.points_dev = torch.from_numpy(self.points).to(device)
        return self


def check_sampler_cfg(cfg):
    """Refuses, by name, what the fine-tune pass does not restate."""
    if cfg.get("USE_ROAD_PLANE", False):
        raise NotImplementedError("gt_sampling USE_ROAD_PLANE: True")
    if cfg.get("DATABASE_WITH_FAKELIDAR", False):
        raise NotImplementedError("gt_sampling DATABASE_WITH_FAKELIDAR")
    if cfg.get("FADE_EPOCH", 0) != 0:
        raise NotImplementedError("gt_sampling FADE_EPOCH != 0")


def sampler_state(sampler_cfg, database, class_names):
    """Pointer and permutation of every sample group (database_sampler.py:41-54): the pointer starts past the end, so
    the first draw of a class permutes."""
    check_sampler_cfg(sampler_cfg)
    groups = []
    for x in sampler_cfg["SAMPLE_GROUPS"]:
        name, num = x.split(":")
        if name not in class_names:
            continue
        n = int(database.class_index.get(name, np.zeros(0)).shape[0]) if isinstance(database, GtDatabase) else int(database[name])
        groups.append({"name": name, "sample_num": int(num), "pointer": n, "indices": np.arange(n), "size": n})
    return {"groups": groups, "limit_whole_scene": bool(sampler_cfg.get("LIMIT_WHOLE_SCENE", False))}


def draw_candidates(state, gt_names):
    """Candidate draw of ONE frame, group by group in SAMPLE_GROUPS order, consuming ``np.random`` like
    DataBaseSampler.__call__ / sample_with_fixed_number (database_sampler.py:122-139, :230-235): -> [(class name,
    indices into that class's list)].  LIMIT_WHOLE_SCENE subtracts the frame's own count of the name, over ALL names."""
    names = np.asarray(gt_names).astype(str)
    out = []
    for g in state["groups"]:
        num = g["sample_num"] - int(np.sum(g["name"] == names)) if state["limit_whole_scene"] else g["sample_num"]
        if num <= 0:
            continue
        if g["pointer"] >= g["size"]:
            g["indices"] = np.random.permutation(g["size"])
            g["pointer"] = 0
        out.append((g["name"], np.asarray(g["indices"][g["pointer"]:g["pointer"] + num], dtype=np.int64)))
        g["pointer"] += num
    return out


def finetune_params_table(params: Sequence[dict]) -> np.ndarray:
    """``params_table`` plus, in column 5, the angle rounded to fp32: what ``gt_boxes[:, 6] += noise_rotation`` adds to a
    float32 heading (data_augmentor.py:108)."""
    t = params_table(params)
    t[:, 5] = [np.float32(p["angle"]) for p in params]
    return t


class GpuFinetuneInputPipeline(GpuInputPipeline):
    def __init__(self, point_cloud_range, class_names, aug_config: Optional[Sequence[dict]] = FINETUNE_AUG_CONFIG, database: Optional[GtDatabase] = None,
                 shuffle: bool = True, resident: bool = True, min_num_corners: int = 1, device: Optional[torch.device] = None):
        aug_config = list(aug_config or [])
        world = [c for c in aug_config if c["NAME"] != "gt_sampling"]
        for c in world:
            if c["NAME"] not in ("random_world_flip", "random_world_rotation", "random_world_scaling"):
                raise NotImplementedError(f"augmentation {c['NAME']} is outside the fine-tune input pipeline")
        super().__init__(point_cloud_range, world, shuffle, device)
        self.range6 = [float(v) for v in point_cloud_range]
        self.class_names = list(class_names)
        self.min_num_corners = int(min_num_corners)
        sampler = [c for c in aug_config if c["NAME"] == "gt_sampling"]
        if len(sampler) > 1 or (sampler and aug_config[0]["NAME"] != "gt_sampling"):
            raise NotImplementedError("gt_sampling must be the first and only sampler of the augmentation list")
        self.sampler_cfg = sampler[0] if sampler and database is not None else None
        self.database = self.state = None
        self.resident = bool(resident)
        self.extra_width, self.remove_points = [0.0, 0.0, 0.0], True
        self.time_kernels, self.kernel_events = False, None       # tools/bench_finetune_input.py: events around the two launches
        if sampler:
            check_sampler_cfg(sampler[0])
        if self.sampler_cfg is not None:
            self.database = database.prepare(self.sampler_cfg.get("PREPARE", {}))
            self.state = sampler_state(self.sampler_cfg, self.database, self.class_names)
            self.group_of = {g["name"]: k for k, g in enumerate(self.state["groups"])}
            self.remove_points = bool(self.sampler_cfg.get("REMOVE_POINTS", True))
            self.extra_width = [float(v) for v in self.sampler_cfg.get("REMOVE_EXTRA_WIDTH", [0.0, 0.0, 0.0])]
            if self.resident and self.database.points_dev is None:
                self.database.to(self.device)

    def __call__(self, frames: List[np.ndarray], gt_boxes: List[np.ndarray], gt_names: List[Sequence[str]],
                 params: Optional[Sequence[dict]] = None, candidates: Optional[Sequence[Sequence]] = None,
                 perms: Optional[Sequence[np.ndarray]] = None) -> dict:
        """frames: B raw clouds (n_i, F) float32; gt_boxes: B arrays (m_i, 7); gt_names: B name lists (ALL of the frame's
        names, also those outside ``class_names``).  -> {'points' (N, 1 + F), 'gt_boxes' (B, max_gt, 8), 'batch_size',
        'num_gt' (host list: kept boxes per frame; 0 is where the reference re-draws another sample), 'sampled_valid'
        (per frame, one flag per candidate)}.  ``params`` / ``candidates`` (per frame [(class name, indices into the
        class's list), ...] in group order) / ``perms``: explicit decisions for parity tests."""
        return self._run(frames, gt_boxes, gt_names, params, candidates, perms)

    # what GpuFinetuneAugInputPipeline replaces: one frame's draws behind the sampler's, ints behind the packed counts, the launches
    def _draw_frame_params(self) -> dict:
        return draw_world_params(self.aug_config) if self.aug_config else {"flip_x": False, "flip_y": False, "angle": 0.0, "scale": 1.0}

    def _extra_meta_ints(self, B: int) -> int:
        return 0

    def _launch(self, k, ev) -> None:
        """k: the call's tables and buffers; ev: None or three events (before, between and behind the two launches)."""
        try:
            L.call("gdmae_gt_sample_select", k.boxes, k.desc_h.ctypes.data, k.desc, k.group, k.B, k.n_groups, k.tab,
                   L.host_f32(self.range6), L.host_f32(self.extra_width), self.min_num_corners, k.cap, k.valid, L.ptr(k.rm_boxes),
                   k.n_valid, k.gt_out, k.num_gt, L.stream())
        except L.GdmaeHipError as e:
            if "more than" in str(e):
                raise NotImplementedError(str(e)) from e
            raise
        if ev:
            ev[1].record()
        L.call("gdmae_gt_sample_collate", L.ptr(k.raw), L.ptr(k.db), k.F, k.seg, k.S, k.n_rows, k.B, k.tab, k.boxes, k.valid,
               L.ptr(k.rm_boxes), k.n_valid if self.remove_points else None, L.host_f32(self.xy_range), L.ptr(k.out), k.kept, L.ptr(k.ws),
               L.stream())

    def _prepare(self, k) -> None:
        pass

    def _extend_result(self, result: dict, k, extra: list) -> None:
        pass

    def _run(self, frames, gt_boxes, gt_names, params, candidates, perms, **aug) -> dict:
        B = len(frames)
        F = int(frames[0].shape[1])
        db = self.database
        drawn_c, drawn_p = [], []
        for b in range(B):                                  # the reference's order: per frame, the sampler, then the world draws
            if candidates is not None:
                drawn_c.append(list(candidates[b]))
            else:
                drawn_c.append(draw_candidates(self.state, gt_names[b]) if self.state is not None else [])
            if params is None:
                drawn_p.append(self._draw_frame_params())
        params = drawn_p if params is None else params
        if any(len(c) for c in drawn_c) and db is None:
            raise ValueError("candidates without a database")
        if db is not None and db.points.shape[1] != F:
            raise ValueError(f"database points have {db.points.shape[1]} columns, the frames {F}")

        # ---- host tables -------------------------------------------------------------------------------------------
        box_rows, desc, cand_group, cand_entry, cap = [], [], [], [], 0
        for b in range(B):
            gb = np.asarray(gt_boxes[b])
            if gb.ndim == 2 and gb.shape[1] > 7:
                raise NotImplementedError("GT boxes with more than 7 columns (velocities) are not supported")
            gb = gb.reshape(-1, 7).astype(np.float32)
            names = np.asarray(gt_names[b]).astype(str).reshape(-1)
            assert names.shape[0] == gb.shape[0], "one name per GT box"
            cls = np.array([self.class_names.index(n) + 1 if n in self.class_names else 0 for n in names], np.float32)
            ents, grp = [], []
            for name, local in drawn_c[b]:
                e = db.class_index[name][np.asarray(local, dtype=np.int64)]
                ents.append(e)
                grp += [self.group_of[name]] * len(e)
            ents = np.concatenate(ents) if ents else np.zeros(0, np.int64)
            ccls = np.array([self.class_names.index(n) + 1 for n in db.names[ents]], np.float32) if len(ents) else np.zeros(0, np.float32)
            cb = db.boxes[ents] if len(ents) else np.zeros((0, 7), np.float32)
            desc.append((sum(r.shape[0] for r in box_rows), gb.shape[0], len(ents), len(cand_group)))
            box_rows.append(np.concatenate([np.concatenate([gb, cb]), np.concatenate([cls, ccls])[:, None]], 1))
            cand_group += grp
            cand_entry.append(ents)
            cap = max(cap, int((cls > 0).sum()) + len(ents))
        C = len(cand_group)
        n_groups = len(self.state["groups"]) if self.state is not None else 0
        boxes_h = np.concatenate(box_rows).astype(np.float32) if box_rows else np.zeros((0, 8), np.float32)
        desc_h = np.asarray(desc, np.int32).reshape(B, 4)

        # virtual rows: per frame the object points of every candidate, then the scene points
        n_scene = sum(f.shape[0] for f in frames)
        n_obj = sum(int(db.offsets[e, 1] - db.offsets[e, 0]) for ents in cand_entry for e in ents)
        staged_rows = n_scene + (0 if self.resident else n_obj)
        host = self._staging(max(staged_rows, 1) * F).view(-1, F)[:max(staged_rows, 1)]
        hv = host.numpy()
        seg, row, src, stage, frame_rows = [], 0, 0, n_scene, [0]
        for b, f in enumerate(frames):
            assert f.dtype == np.float32 and f.shape[1] == F
            first, row0 = 1, row                            # column 7: the frame's first virtual row (the drop's row index counts from it)
            for k, e in enumerate(cand_entry[b]):
                s0, s1 = (int(v) for v in db.offsets[e])
                if s1 > s0:
                    if self.resident:
                        seg.append((row, s0, 1, b, desc[b][0] + desc[b][1] + k, desc[b][3] + k, first, row0))
                    else:
                        hv[stage:stage + s1 - s0] = db.points[s0:s1]
                        seg.append((row, stage, 0, b, desc[b][0] + desc[b][1] + k, desc[b][3] + k, first, row0))
                        stage += s1 - s0
                    row += s1 - s0
                    first = 0
            if f.shape[0]:
                hv[src:src + f.shape[0]] = f
                seg.append((row, src, 0, b, -1, -1, first, row0))
                row += f.shape[0]
                src += f.shape[0]
            frame_rows.append(row)
        n_rows, S = row, len(seg)
        assert n_rows < 2 ** 31
        ints_h = np.concatenate([desc_h.reshape(-1), np.asarray(cand_group, np.int32), np.asarray(seg, np.int32).reshape(-1)]).astype(np.int32)
        flts_h = np.concatenate([finetune_params_table(params).reshape(-1), boxes_h.reshape(-1)]).astype(np.float32)

        # ---- device ------------------------------------------------------------------------------------------------
        dev = self.device
        raw = host.to(dev, non_blocking=True)
        self._copied = torch.cuda.Event()
        self._copied.record()
        ints_d = torch.from_numpy(ints_h).to(dev)
        flts_d = torch.from_numpy(flts_h).to(dev)
        desc_d, group_d, seg_d = ints_d[:B * 4], ints_d[B * 4:B * 4 + C], ints_d[B * 4 + C:]
        tab_d, boxes_d = flts_d[:B * 8], flts_d[B * 8:]
        n_extra = self._extra_meta_ints(B)
        meta = torch.empty(3 * B + 1 + C + n_extra, dtype=torch.int32, device=dev)     # [kept_off (B + 1) | num_gt (B) | n_valid (B) | valid (C) | extra]
        kept, num_gt_d, n_valid_d, valid_d = meta[:B + 1], meta[B + 1:2 * B + 1], meta[2 * B + 1:3 * B + 1], meta[3 * B + 1:3 * B + 1 + C]
        rm_boxes = torch.empty(B, MAX_CANDIDATES, 8, dtype=torch.float32, device=dev)
        gt_out = torch.empty(B, cap, 8, dtype=torch.float32, device=dev)
        out = torch.empty(max(n_rows, 1), 1 + F, dtype=torch.float32, device=dev)
        ws = torch.empty(L.load().gdmae_gt_sample_workspace_bytes(n_rows), dtype=torch.uint8, device=dev)
        dptr = lambda t: t.data_ptr() if t.numel() else None      # noqa: E731  (views of the packed tables; empty ones are never read)
        k = SimpleNamespace(B=B, F=F, S=S, C=C, n_rows=n_rows, n_groups=n_groups, cap=cap, desc_h=desc_h, frame_rows=frame_rows, dev=dev,
                            raw=raw, db=db.points_dev if (db is not None and self.resident) else raw, boxes=dptr(boxes_d),
                            desc=dptr(desc_d), group=dptr(group_d), seg=dptr(seg_d), tab=dptr(tab_d), valid=dptr(valid_d),
                            n_valid=dptr(n_valid_d), num_gt=dptr(num_gt_d), kept=dptr(kept), gt_out=dptr(gt_out), rm_boxes=rm_boxes, out=out,
                            ws=ws, extra=meta[3 * B + 1 + C:], params=params, aug=aug)
        self._prepare(k)
        ev = self.kernel_events = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if self.time_kernels else None
        if ev:
            ev[0].record()
        self._launch(k, ev)
        if ev:
            ev[2].record()
        meta_h = meta.tolist()                              # the one host read of the call: point counts and box counts together
        kept_h, num_gt = meta_h[:B + 1], meta_h[B + 1:2 * B + 1]
        valid_h = np.asarray(meta_h[3 * B + 1:3 * B + 1 + C], dtype=bool)
        n = kept_h[B]
        for b in range(B - 1, -1, -1):
            if kept_h[b] < 0:
                kept_h[b] = kept_h[b + 1]
        pts = out[:n]
        if perms is not None:
            idx = torch.cat([torch.from_numpy(np.asarray(p, np.int64)) + kept_h[b] for b, p in enumerate(perms)]).to(dev)
            pts = pts.index_select(0, idx)
        elif self.shuffle and n > 0:
            pts = pts.index_select(0, torch.argsort(pts[:, 0] + torch.rand(n, device=dev)))
        result = {"points": pts, "gt_boxes": gt_out[:, :max(num_gt) if num_gt else 0].contiguous(), "batch_size": B, "num_gt": num_gt,
                  "sampled_valid": [valid_h[d[3]:d[3] + d[2]] for d in desc]}
        self._extend_result(result, k, meta_h[3 * B + 1 + C:])
        return result


# ---------------------------------------------------------------------------------------------------------------------
# random_world_translation and random_world_drop ("translation and drop"): the lists of waymo_models/gd_mae_iou.yaml
# and gd_mae_ts.yaml
#
#     gt_sampling -> flip -> rotation -> scaling -> translation -> drop -> heading limit_period -> range masks -> shuffle -> collate
# ---------------------------------------------------------------------------------------------------------------------
_WORLD3 = ("random_world_flip", "random_world_rotation", "random_world_scaling")
_TAIL = ("random_world_translation", "random_world_drop")
_GOLDEN = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1


def drop_keys_of(seed: int, n: int) -> np.ndarray:
    """The device's 32-bit drop keys of virtual rows 0 .. n - 1 of a frame, restated in numpy uint64: the upper half of splitmix64's
    finaliser on ``seed + (j + 1) * 0x9E3779B97F4A7C15`` (csrc/gt_sampling.hip: gs_drop_key)."""
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & _M64) + (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(_GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return ((z ^ (z >> np.uint64(31))) >> np.uint64(32)).astype(np.uint32)


def _enable(p) -> bool:
    return bool(np.random.choice([False, True], replace=False, p=[1 - p, p]))


def draw_translation(cfg) -> np.ndarray:
    """data_augmentor.py:151-159: the enable draw, then three normals (std 0 when disabled) -> (3) float64."""
    std = cfg["NOISE_TRANSLATE_STD"] if _enable(cfg["PROBABILITY"]) else [0.0, 0.0, 0.0]
    if not isinstance(std, list):
        std = [std, std, std]
    return np.array([np.random.normal(0, std[0], 1), np.random.normal(0, std[1], 1), np.random.normal(0, std[2], 1)]).T.reshape(3).astype(np.float64)


def draw_drop(cfg):
    """data_augmentor.py:46-47: the enable draw -> q = Python's 1 - DROP_RATIO or 1.0; then the frame's 64-bit seed (the reference draws
    its k-subset with np.random.choice here: the same distribution, another stream)."""
    q = 1 - cfg["DROP_RATIO"] if _enable(cfg["PROBABILITY"]) else 1.0
    hi, lo = (int(v) for v in np.random.randint(0, 1 << 32, 2, dtype=np.uint64))
    return float(q), (hi << 32) | lo


class GpuFinetuneAugInputPipeline(GpuFinetuneInputPipeline):
    """GpuFinetuneInputPipeline plus ``random_world_translation`` and / or ``random_world_drop`` behind the scaling, in that order.
    ``params`` dicts may carry ``translate`` (3 float64), ``drop_q`` (1 - DROP_RATIO, or 1.0 for a frame that does not drop) and
    ``drop_seed``; absent keys mean no translation and no drop.  ``drop_keys``: one uint32 array per frame over its virtual rows (every
    candidate's object points, then the scene points) instead of the hashed keys.  The result gains ``drop_n`` / ``drop_k`` (host
    lists: eligible rows and rows the drop keeps, per frame; None when no frame of the batch drops)."""

    def __init__(self, point_cloud_range, class_names, aug_config, database: Optional[GtDatabase] = None, **kw):
        aug_config = list(aug_config or [])
        names = [c["NAME"] for c in aug_config]
        rest = [c for c in aug_config if c["NAME"] not in _TAIL]
        tail = [c for c in aug_config if c["NAME"] in _TAIL]
        for n in names:                                     # a foreign name is refused as such, wherever it stands
            if n not in ("gt_sampling",) + _WORLD3 + _TAIL:
                raise NotImplementedError(f"augmentation {n} is outside the fine-tune input pipeline")
        for n in _TAIL:
            if names.count(n) > 1:
                raise NotImplementedError(f"augmentation {n} appears twice in the list")
        bad = next((n for i, n in enumerate(names) if n in _TAIL and any(m not in _TAIL for m in names[i + 1:])), None)     # not at the end
        if bad is None and [c["NAME"] for c in tail] == list(reversed(_TAIL)):
            bad = _TAIL[1]                                                                                                   # drop before translation
        if bad is not None:
            raise NotImplementedError(f"augmentation {bad} is out of order: the fine-tune input pipeline applies flip, rotation, scaling, "
                                      "random_world_translation, random_world_drop in this order")
        super().__init__(point_cloud_range, class_names, rest, database, **kw)
        self.translate_cfg = next((c for c in tail if c["NAME"] == _TAIL[0]), None)
        self.drop_cfg = next((c for c in tail if c["NAME"] == _TAIL[1]), None)
        if self.translate_cfg is not None:
            std = self.translate_cfg["NOISE_TRANSLATE_STD"]
            if isinstance(std, (list, tuple)) and len(std) != 3:
                raise ValueError(f"random_world_translation NOISE_TRANSLATE_STD needs 3 entries or a scalar, got {len(std)}")
        if self.drop_cfg is not None and not 0.0 <= float(self.drop_cfg["DROP_RATIO"]) <= 1.0:
            raise ValueError(f"random_world_drop DROP_RATIO {self.drop_cfg['DROP_RATIO']} is outside [0, 1]")
        self.plan_events = None

    def __call__(self, frames, gt_boxes, gt_names, params=None, candidates=None, perms=None, drop_keys=None) -> dict:
        return self._run(frames, gt_boxes, gt_names, params, candidates, perms, drop_keys=drop_keys)

    def _draw_frame_params(self) -> dict:
        p = super()._draw_frame_params()
        if self.translate_cfg is not None:
            p["translate"] = draw_translation(self.translate_cfg)
        if self.drop_cfg is not None:
            p["drop_q"], p["drop_seed"] = draw_drop(self.drop_cfg)
        return p

    def _extra_meta_ints(self, B: int) -> int:
        return 8 * B                                        # the drop plan: [n, k, T, admitted ties, J, ties, 0, 0] per frame

    def _prepare(self, k) -> None:
        B = k.B
        t = np.zeros((B, 3), np.float64)
        q = np.ones(B, np.float64)
        seeds = np.zeros(B, np.uint64)
        for b, p in enumerate(k.params):
            if "translate" in p:
                if self.translate_cfg is None:
                    raise ValueError("params carry a translation, but random_world_translation is not in the augmentation list")
                t[b] = np.asarray(p["translate"], np.float64).reshape(3)
            if float(p.get("drop_q", 1.0)) != 1.0 and self.drop_cfg is None:
                raise ValueError("params carry a drop, but random_world_drop is not in the augmentation list")
            q[b] = float(p.get("drop_q", 1.0))
            seeds[b] = np.uint64(int(p.get("drop_seed", 0)) & _M64)
        if ((q < 0) | (q > 1)).any():
            raise ValueError("drop_q outside [0, 1]")
        k.plan_on = bool((q != 1.0).any())
        packed = torch.from_numpy(np.concatenate([t.reshape(-1).view(np.int64), q.view(np.int64), seeds.view(np.int64)])).to(k.dev)
        k.packed = packed
        k.translate = packed.data_ptr() if self.translate_cfg is not None else None      # in the list: the add runs, also with t = 0
        k.q, k.seeds = packed[3 * B:].data_ptr(), packed[4 * B:].data_ptr()
        k.keys = k.keys_t = k.drop_ws = None
        if k.plan_on:
            dk = k.aug.get("drop_keys")
            if dk is not None and k.n_rows > 0:
                for b in range(B):
                    assert len(dk[b]) == k.frame_rows[b + 1] - k.frame_rows[b], "one key per virtual row of the frame"
                k.keys_t = torch.from_numpy(np.concatenate([np.asarray(a, np.uint32) for a in dk]).view(np.int32)).to(k.dev)
                k.keys = k.keys_t.data_ptr()
            k.drop_ws = torch.empty(L.load().gdmae_gt_sample_drop_workspace_bytes(k.n_rows, B), dtype=torch.uint8, device=k.dev)

    def _launch(self, k, ev) -> None:
        try:
            L.call("gdmae_gt_sample_select_aug", k.boxes, k.desc_h.ctypes.data, k.desc, k.group, k.B, k.n_groups, k.tab, k.translate,
                   L.host_f32(self.range6), L.host_f32(self.extra_width), self.min_num_corners, k.cap, k.valid, L.ptr(k.rm_boxes),
                   k.n_valid, k.gt_out, k.num_gt, L.stream())
        except L.GdmaeHipError as e:
            if "more than" in str(e):
                raise NotImplementedError(str(e)) from e
            raise
        if ev:
            ev[1].record()
        n_valid = k.n_valid if self.remove_points else None
        plan = None
        if k.plan_on:
            plan = k.extra.data_ptr()
            pe = self.plan_events = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if ev else None
            if pe:
                pe[0].record()
            L.call("gdmae_gt_sample_drop_plan", L.ptr(k.raw), L.ptr(k.db), k.F, k.seg, k.S, k.n_rows, k.B, k.boxes, k.valid, L.ptr(k.rm_boxes),
                   n_valid, k.seeds, k.q, k.keys, plan, L.ptr(k.drop_ws), L.stream())
            if pe:
                pe[1].record()
        L.call("gdmae_gt_sample_collate_aug", L.ptr(k.raw), L.ptr(k.db), k.F, k.seg, k.S, k.n_rows, k.B, k.tab, k.translate, k.boxes, k.valid,
               L.ptr(k.rm_boxes), n_valid, k.seeds, k.keys, plan, L.ptr(k.drop_ws) if plan else None, L.host_f32(self.xy_range), L.ptr(k.out),
               k.kept, L.ptr(k.ws), L.stream())

    def _extend_result(self, result: dict, k, extra: list) -> None:
        result["drop_n"] = [extra[8 * b] for b in range(k.B)] if k.plan_on else None
        result["drop_k"] = [extra[8 * b + 1] for b in range(k.B)] if k.plan_on else None


def finetune_input_pipeline(point_cloud_range, class_names, aug_config: Optional[Sequence[dict]] = FINETUNE_AUG_CONFIG,
                            database: Optional[GtDatabase] = None, **kw) -> GpuFinetuneInputPipeline:
    """The fine-tune input pipeline of an augmentation list: GpuFinetuneInputPipeline for the list of waymo_models/gd_mae.yaml,
    GpuFinetuneAugInputPipeline when the list holds ``random_world_translation`` and / or ``random_world_drop`` (gd_mae_iou.yaml,
    gd_mae_ts.yaml: ``configs.waymo_iou_finetune_data_cfg`` / ``waymo_two_stage_data_cfg``).  Every other name is refused by name."""
    names = {c["NAME"] for c in (aug_config or [])}
    cls = GpuFinetuneAugInputPipeline if names & set(_TAIL) else GpuFinetuneInputPipeline
    return cls(point_cloud_range, class_names, aug_config, database, **kw)
