"""ctypes mirror of include/similari_pose.h and include/similari_pose_batch.h (keypoint association: the poses of a frame, or of the
frames of many cameras, matched to the tracks of a point bank, on the device) and PoseBank, a PointBank that can be asked which pose
continues which track.

    bank = PoseBank(engine, points=17)
    ids = bank.track(pts, new_ids)                 # associate, step the matched and the new tracks, let the others coast
    ids, w = bank.associate(pts)                   # or only the question: [m] track ids (0 = a new track), [m] weights (NaN = none)
    with register_tensor(engine, pose):            # the poses where the network left them
        ids, w = bank.associate(rows=DeviceRows.from_tensor(pose[:, 4:4 + 17 * 3]), comps=3, min_score=0.3)
    per_cam = bank.associate_batch([(ids0, pts0), (ids1, pts1)])   # every camera in one call: [(track ids, weights), ...]
    per_cam = bank.track_batch([(ids0, pts0), (ids1, pts1)], new_ids)   # the frame loop for all cameras: one associate_batch, one step, one predict
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .points import POINTS, PointBank, sa_point_rows
from .pose_oks import default_threshold, set_metric
from .search import _p

u32, u64 = C.c_uint32, C.c_uint64
P = C.POINTER
SA_POSE_MAX = 2048
SA_POSE_BATCH_SCENES = 65535
SA_POSE_BATCH_CELLS = 1 << 27


class sa_pose_options(C.Structure):
    _fields_ = [("struct_size", u32), ("min_common", u32), ("threshold", C.c_float), ("reserved", u32)]


class sa_pose_stats(C.Structure):
    _fields_ = [("struct_size", u32), ("poses", u32), ("tracks", u32), ("launches", u32), ("roots", u32), ("matched", u32),
                ("bytes_h2d", u64), ("bytes_d2h", u64), ("src_bytes", u64), ("device_ms", C.c_double), ("kernel_ms", C.c_double * 3)]


class sa_pose_batch_stats(C.Structure):
    _fields_ = [("struct_size", u32), ("scenes", u32), ("poses", u32), ("tracks", u32), ("tiles", u32), ("launches", u32), ("roots", u32),
                ("matched", u32), ("bytes_h2d", u64), ("bytes_d2h", u64), ("src_bytes", u64), ("device_ms", C.c_double),
                ("kernel_ms", C.c_double * 3)]


# ---- prototypes of every symbol include/similari_pose.h and include/similari_pose_batch.h declare --
PROTOTYPES = {
    "sa_pose_options_default": (None, [P(sa_pose_options)]),
    "sa_points_associate": (C.c_int, [POINTS, u32, P(u64), u32, P(sa_point_rows), P(sa_pose_options), P(u64), P(C.c_float), P(C.c_float)]),
    "sa_points_associate_last": (C.c_int, [POINTS, P(sa_pose_stats)]),
    "sa_points_associate_batch": (C.c_int, [POINTS, u32, P(u32), P(u64), P(u32), P(sa_point_rows), P(sa_pose_options), P(u64), P(C.c_float), P(u32),
                                            P(C.c_float)]),
    "sa_points_associate_batch_last": (C.c_int, [POINTS, P(sa_pose_batch_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


class PoseBank(PointBank):
    """A point bank whose tracks the poses of a frame can be matched to."""

    def __init__(self, engine, points: int = 17, position_weight: float = 1 / 20, velocity_weight: float = 1 / 160, metric=None):
        """metric: None (the mean inverted Mahalanobis cost) or a pose_oks.OksMetric: every vote of the bank is by it, and a vote
        whose caller gives no threshold takes 0.3 instead of 1.0."""
        super().__init__(engine, points, position_weight, velocity_weight)
        if not getattr(self.lib, "_sa_pose_bound", False):
            bind(self.lib)
            self.lib._sa_pose_bound = True
        self.metric = None
        if metric is not None:
            set_metric(self, metric)

    def associate(self, pts=None, present=None, rows=None, comps=2, min_score=0.0, ids=None, threshold=None, min_common=1, matrix=False):
        """The poses ([m, P, 2 or 3] array, or rows= with one row per pose: len(rows.index), else rows.n_rows) against the tracks `ids`
        (None: every track, in order() order) -> (track_ids [m] u64, 0 = no track: a new one; weights [m] f32, NaN where none) and,
        with matrix=True, the [m, tracks] weights of every pair (NaN = no pair).  Changes no state."""
        if rows is None:
            m = len(pts)
        else:
            index = getattr(rows, "index", None)
            m = len(index) if index is not None else int(rows.n_rows)
        alive, r = self._source(m, pts, present, rows, comps, min_score)
        o = sa_pose_options()
        self.lib.sa_pose_options_default(C.byref(o))
        o.threshold, o.min_common = default_threshold(getattr(self, "metric", None), threshold), min_common
        n = len(self)
        if ids is not None:
            ids = self._ids(ids)
            n = len(ids)
        out_ids, out_w = np.zeros(m, np.uint64), np.full(m, np.nan, np.float32)
        tap = np.full((m, n), np.nan, np.float32) if matrix else None
        self._chk(self.lib.sa_points_associate(self.h, n, None if ids is None else _p(ids, u64), m, C.byref(r), C.byref(o),
                                              _p(out_ids, u64), _p(out_w, C.c_float), _p(tap, C.c_float)))
        return (out_ids, out_w, tap) if matrix else (out_ids, out_w)

    def last_associate(self) -> dict:
        """The fields of sa_pose_stats of the last associate."""
        st = sa_pose_stats()
        self._chk(self.lib.sa_points_associate_last(self.h, C.byref(st)))
        out = {f: getattr(st, f) for f, _ in sa_pose_stats._fields_}
        out["kernel_ms"] = list(st.kernel_ms)
        return out

    def associate_batch(self, scenes=None, rows=None, track_ids=None, track_counts=None, pose_counts=None, present=None, comps=2, min_score=0.0,
                        threshold=None, min_common=1, matrix=False):
        """The poses of many scenes (cameras) against the tracks of this bank in one call, three launches whatever their number.
        scenes: a list of (ids, pts[, present]) — the scene's track ids, its poses [m, P, 2 or 3] (the same 2 or 3 in every scene) and,
        for all scenes or for none, their present mask.  Or rows= (a DeviceRows whose rows, or index, list the poses of the whole call
        scene after scene) with track_ids (a list of per-scene id arrays, or one flat array with track_counts=) and pose_counts=;
        present: the [sum m, P] mask of the whole call.
        -> one (track_ids [m_s] u64, weights [m_s] f32) per scene, as associate() gives them for that scene alone; with matrix=True
        (track_ids, weights, tap [m_s, n_s]).  A pose is never given a track of another scene.  Changes no state."""
        if scenes is not None:
            assert rows is None and track_ids is None and present is None, "scenes carry their own ids, poses and masks"
            scenes = [tuple(sc) for sc in scenes]
            id_list = [self._ids(sc[0]) for sc in scenes]
            pts_list = [np.asarray(sc[1], np.float32) for sc in scenes]
            comps_in = {p.shape[2] for p in pts_list if p.ndim == 3} or {2}
            assert len(comps_in) == 1, "every scene's poses have 2, or every scene's have 3, components"
            c = comps_in.pop()
            pts_list = [p.reshape(-1, self.P, c) for p in pts_list]
            pose_counts = [len(p) for p in pts_list]
            masked = [len(sc) > 2 and sc[2] is not None for sc in scenes]
            assert all(masked) or not any(masked), "a present mask for every scene or for none"
            pts = np.concatenate(pts_list) if pts_list else np.zeros((0, self.P, c), np.float32)
            if any(masked):
                present = np.concatenate([np.asarray(sc[2]).reshape(-1, self.P) != 0 for sc in scenes])
        else:
            assert rows is not None and track_ids is not None and pose_counts is not None, "rows= comes with track_ids= and pose_counts="
            id_list = [self._ids(t) for t in track_ids] if track_counts is None else None
            pts = None
        if id_list is not None:
            track_counts = [len(t) for t in id_list]
            flat = np.concatenate(id_list) if id_list else np.zeros(0, np.uint64)
        else:
            flat = self._ids(track_ids)
        tc = np.ascontiguousarray(track_counts, np.uint32).reshape(-1)
        pc = np.ascontiguousarray(pose_counts, np.uint32).reshape(-1)
        assert len(tc) == len(pc) and int(tc.sum()) == len(flat), "one track count and one pose count per scene; the ids scene after scene"
        S, m = len(pc), int(pc.sum())
        alive, r = self._source(m, pts, present, rows, comps, min_score)
        o = sa_pose_options()
        self.lib.sa_pose_options_default(C.byref(o))
        o.threshold, o.min_common = default_threshold(getattr(self, "metric", None), threshold), min_common
        out_ids, out_w = np.zeros(max(m, 1), np.uint64), np.full(max(m, 1), np.nan, np.float32)
        cells = pc.astype(np.int64) * tc.astype(np.int64)
        tap = np.full(max(int(cells.sum()), 1), np.nan, np.float32) if matrix else None
        flat = flat if len(flat) else np.zeros(1, np.uint64)   # never a null pointer
        roots = np.zeros(max(S, 1), np.uint32)
        self._batch_roots = None
        self._chk(self.lib.sa_points_associate_batch(self.h, S, _p(tc, u32), _p(flat, u64), _p(pc, u32), C.byref(r), C.byref(o), _p(out_ids, u64),
                                                    _p(out_w, C.c_float), _p(roots, u32), _p(tap, C.c_float)))
        self._batch_roots = roots[:S]
        p0 = np.concatenate([[0], np.cumsum(pc, dtype=np.int64)])
        c0 = np.concatenate([[0], np.cumsum(cells)])
        out = []
        for s in range(S):
            got = (out_ids[p0[s]: p0[s + 1]], out_w[p0[s]: p0[s + 1]])
            out.append(got + (tap[c0[s]: c0[s + 1]].reshape(int(pc[s]), int(tc[s])),) if matrix else got)
        return out

    def last_associate_batch(self) -> dict:
        """The fields of sa_pose_batch_stats of the last associate_batch and "scene_roots", the search roots of each scene (None after
        a refused call)."""
        st = sa_pose_batch_stats()
        self._chk(self.lib.sa_points_associate_batch_last(self.h, C.byref(st)))
        out = {f: getattr(st, f) for f, _ in sa_pose_batch_stats._fields_}
        out["kernel_ms"] = list(st.kernel_ms)
        out["scene_roots"] = getattr(self, "_batch_roots", None)
        return out

    def track(self, pts, new_ids, present=None, min_score=0.0, threshold=None, min_common=1, coast=True):
        """One frame of a tracker loop over host poses pts [m, P, 2 or 3]: associate; step the matched tracks and, for every
        unmatched pose, the next unused id of new_ids, in pose order; coast: predict the tracks nobody matched.  -> the id given to
        every pose [m] u64."""
        ids, _ = self.associate(pts, present=present, min_score=min_score, threshold=threshold, min_common=min_common)
        fresh = np.flatnonzero(ids == 0)
        new_ids = self._ids(new_ids)
        assert len(new_ids) >= len(fresh), "one new id per unmatched pose"
        idle = np.setdiff1d(self.order(), ids[ids != 0]) if coast else np.zeros(0, np.uint64)
        ids[fresh] = new_ids[: len(fresh)]
        if len(ids):
            self.step(ids, pts, present=present, min_score=min_score)
        if len(idle):
            self.predict(idle)
        return ids

    def track_batch(self, scenes, new_ids, min_score=0.0, threshold=None, min_common=1, coast=True):
        """One frame of the tracker loop for all cameras.  scenes: a list of (ids, pts[, present]) as associate_batch takes them, ids
        being the tracks the bank holds for that camera.  One associate_batch; ONE step over every matched and every new track of
        every scene — an unmatched pose gets the next unused id of new_ids, in scene order, then pose order; coast: ONE predict over
        the listed tracks nobody matched.  -> per scene, the id given to every pose [m_s] u64."""
        scenes = [tuple(sc) for sc in scenes]
        got = self.associate_batch(scenes, min_score=min_score, threshold=threshold, min_common=min_common)
        ids = np.concatenate([g[0] for g in got]) if got else np.zeros(0, np.uint64)
        fresh = np.flatnonzero(ids == 0)
        new_ids = self._ids(new_ids)
        assert len(new_ids) >= len(fresh), "one new id per unmatched pose"
        listed = np.concatenate([self._ids(sc[0]) for sc in scenes]) if scenes else np.zeros(0, np.uint64)
        idle = np.setdiff1d(listed, ids[ids != 0]) if coast else np.zeros(0, np.uint64)
        ids[fresh] = new_ids[: len(fresh)]
        if len(ids):
            pts = np.concatenate([np.asarray(sc[1], np.float32).reshape(len(g[0]), self.P, -1) for sc, g in zip(scenes, got)])
            masked = len(scenes[0]) > 2 and scenes[0][2] is not None
            present = np.concatenate([np.asarray(sc[2]).reshape(-1, self.P) != 0 for sc in scenes]) if masked else None
            self.step(ids, pts, present=present, min_score=min_score)
        if len(idle):
            self.predict(idle)
        ends = np.cumsum([len(g[0]) for g in got])
        return np.split(ids, ends[:-1]) if got else []
