"""ctypes mirror of include/similari_pose_track.h (the keypoint frame loop in one call: associate, step and coast on the device) and
PoseTrackBank, a PoseBank whose track() and track_batch() are that one call.

    bank = PoseTrackBank(engine, points=17)
    ids = bank.track(pts, next_id)                                  # one C call: the vote, the step behind it, the coasting
    per_cam = bank.track_batch([(ids0, pts0), (ids1, pts1)], next_id)   # every camera in one call
    next_id += bank.last_track()["created"]
    with register_tensor(engine, pose):                             # the poses where the network left them
        ids = bank.track(None, next_id, rows=DeviceRows.from_tensor(pose[:, 4:4 + 17 * 3]), comps=3, min_score=0.3)

PoseBank.track / track_batch — one associate, one step, one predict, with the host between them — return and leave the same bits; they
stay as the yardstick.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .points import POINTS, sa_point_rows
from .pose import PoseBank
from .pose_oks import default_threshold
from .search import _p

u32, u64 = C.c_uint32, C.c_uint64
P = C.POINTER


class sa_pose_track_options(C.Structure):
    _fields_ = [("struct_size", u32), ("min_common", u32), ("threshold", C.c_float), ("coast", u32)]


class sa_pose_track_stats(C.Structure):
    _fields_ = [("struct_size", u32), ("scenes", u32), ("poses", u32), ("tracks", u32), ("vote_launches", u32), ("step_launches", u32),
                ("roots", u32), ("matched", u32), ("created", u32), ("coasted", u32), ("bytes_h2d", u64), ("bytes_d2h", u64), ("src_bytes", u64),
                ("device_ms", C.c_double), ("kernel_ms", C.c_double * 5)]


# ---- prototypes of every symbol include/similari_pose_track.h declares ---------------------------
PROTOTYPES = {
    "sa_pose_track_options_default": (None, [P(sa_pose_track_options)]),
    "sa_points_track": (C.c_int, [POINTS, u32, P(u64), u32, P(sa_point_rows), u32, P(u64), P(sa_pose_track_options), P(u64), P(C.c_float),
                                  P(C.c_float), P(u32)]),
    "sa_points_track_batch": (C.c_int, [POINTS, u32, P(u32), P(u64), P(u32), P(sa_point_rows), u32, P(u64), P(sa_pose_track_options), P(u64),
                                        P(C.c_float), P(C.c_float), P(u32), P(u32)]),
    "sa_points_track_last": (C.c_int, [POINTS, P(sa_pose_track_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


class PoseTrackBank(PoseBank):
    """A PoseBank whose frame loop is one call."""

    def __init__(self, engine, points: int = 17, position_weight: float = 1 / 20, velocity_weight: float = 1 / 160, metric=None):
        super().__init__(engine, points, position_weight, velocity_weight, metric)
        if not getattr(self.lib, "_sa_pose_track_bound", False):
            bind(self.lib)
            self.lib._sa_pose_track_bound = True

    def _options(self, threshold, min_common, coast):
        o = sa_pose_track_options()
        self.lib.sa_pose_track_options_default(C.byref(o))
        o.threshold, o.min_common, o.coast = default_threshold(getattr(self, "metric", None), threshold), min_common, int(bool(coast))
        return o

    def _new_ids(self, new_ids, m):
        """An array of ids to offer, or the first of m consecutive ones."""
        if np.ndim(new_ids) == 0:
            return np.arange(int(new_ids), int(new_ids) + m, dtype=np.uint64)
        return self._ids(new_ids)

    def track(self, pts, new_ids, present=None, min_score=0.0, threshold=None, min_common=1, coast=True, rows=None, comps=2, track_ids=None, xy=False):
        """PoseBank.track in one call: the poses (pts [m, P, 2 or 3], or rows= with one row per pose) against the tracks track_ids
        (None: every track); a matched pose steps its track, every other takes the next unused id of new_ids (an array, or a first
        id: m consecutive ones are offered), in pose order; coast: the listed tracks nobody matched are predicted.
        -> the id given to every pose [m] u64; with xy=True (ids, xy [m, P, 2]), the step's means."""
        if rows is None:
            m = len(pts)
        else:
            index = getattr(rows, "index", None)
            m = len(index) if index is not None else int(rows.n_rows)
        alive, r = self._source(m, pts, present, rows, comps, min_score)
        o = self._options(threshold, min_common, coast)
        new_ids = self._new_ids(new_ids, m)
        n = 0
        if track_ids is not None:
            track_ids = self._ids(track_ids)
            n = len(track_ids)
            track_ids = track_ids if n else np.zeros(1, np.uint64)   # never a null pointer: null means every track
        out_ids, self._weights = np.zeros(max(m, 1), np.uint64), np.full(max(m, 1), np.nan, np.float32)
        out_xy = self._xy(max(m, 1)) if xy else None
        created = u32()
        self._track_roots = None
        self._chk(self.lib.sa_points_track(self.h, n, _p(track_ids, u64), m, C.byref(r), len(new_ids), _p(new_ids, u64), C.byref(o),
                                          _p(out_ids, u64), _p(self._weights, C.c_float), _p(out_xy, C.c_float), C.byref(created)))
        self._weights = self._weights[:m]
        return (out_ids[:m], out_xy[:m]) if xy else out_ids[:m]

    def track_batch(self, scenes, new_ids, min_score=0.0, threshold=None, min_common=1, coast=True, rows=None, track_ids=None, track_counts=None,
                    pose_counts=None, present=None, comps=2, xy=False):
        """PoseBank.track_batch in one call.  scenes: a list of (ids, pts[, present]) as associate_batch takes them; or scenes=None and
        rows= with track_ids, pose_counts (and track_counts for a flat id array, and present), also as associate_batch takes them.
        -> per scene, the id given to every pose [m_s] u64; with xy=True (ids, xy [m_s, P, 2]) per scene."""
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
        o = self._options(threshold, min_common, coast)
        new_ids = self._new_ids(new_ids, m)
        out_ids, self._weights = np.zeros(max(m, 1), np.uint64), np.full(max(m, 1), np.nan, np.float32)
        out_xy = self._xy(max(m, 1)) if xy else None
        flat = flat if len(flat) else np.zeros(1, np.uint64)   # never a null pointer
        roots = np.zeros(max(S, 1), np.uint32)
        created = u32()
        self._track_roots = None
        self._chk(self.lib.sa_points_track_batch(self.h, S, _p(tc, u32), _p(flat, u64), _p(pc, u32), C.byref(r), len(new_ids), _p(new_ids, u64),
                                                C.byref(o), _p(out_ids, u64), _p(self._weights, C.c_float), _p(out_xy, C.c_float), _p(roots, u32),
                                                C.byref(created)))
        self._track_roots = roots[:S]
        self._weights = self._weights[:m]
        ends = np.cumsum(pc, dtype=np.int64)[:-1]
        ids = np.split(out_ids[:m], ends) if S else []
        return list(zip(ids, np.split(out_xy[:m], ends))) if xy and S else ids

    def last_weights(self) -> np.ndarray:
        """The association's weight of every pose of the last track / track_batch, in call order; NaN for a created track."""
        return self._weights

    def last_track(self) -> dict:
        """The fields of sa_pose_track_stats of the last track / track_batch and, after a track_batch, "scene_roots"."""
        st = sa_pose_track_stats()
        self._chk(self.lib.sa_points_track_last(self.h, C.byref(st)))
        out = {f: getattr(st, f) for f, _ in sa_pose_track_stats._fields_}
        out["kernel_ms"] = list(st.kernel_ms)
        out["scene_roots"] = getattr(self, "_track_roots", None)
        return out
