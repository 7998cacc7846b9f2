"""ctypes mirror of include/similari_pose.h (keypoint association: the poses of a frame matched to the tracks of a point bank, on the
device) and PoseBank, a PointBank that can be asked which pose continues which track.

    bank = PoseBank(engine, points=17)
    ids = bank.track(pts, new_ids)                 # associate, step the matched and the new tracks, let the others coast
    ids, w = bank.associate(pts)                   # or only the question: [m] track ids (0 = a new track), [m] weights (NaN = none)
    with register_tensor(engine, pose):            # the poses where the network left them
        ids, w = bank.associate(rows=DeviceRows.from_tensor(pose[:, 4:4 + 17 * 3]), comps=3, min_score=0.3)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .points import POINTS, PointBank, sa_point_rows
from .search import _p

u32, u64 = C.c_uint32, C.c_uint64
P = C.POINTER
SA_POSE_MAX = 2048


class sa_pose_options(C.Structure):
    _fields_ = [("struct_size", u32), ("min_common", u32), ("threshold", C.c_float), ("reserved", u32)]


class sa_pose_stats(C.Structure):
    _fields_ = [("struct_size", u32), ("poses", u32), ("tracks", u32), ("launches", u32), ("roots", u32), ("matched", u32),
                ("bytes_h2d", u64), ("bytes_d2h", u64), ("src_bytes", u64), ("device_ms", C.c_double), ("kernel_ms", C.c_double * 3)]


# ---- prototypes of every symbol include/similari_pose.h declares ---------------------------------
PROTOTYPES = {
    "sa_pose_options_default": (None, [P(sa_pose_options)]),
    "sa_points_associate": (C.c_int, [POINTS, u32, P(u64), u32, P(sa_point_rows), P(sa_pose_options), P(u64), P(C.c_float), P(C.c_float)]),
    "sa_points_associate_last": (C.c_int, [POINTS, P(sa_pose_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


class PoseBank(PointBank):
    """A point bank whose tracks the poses of a frame can be matched to."""

    def __init__(self, engine, points: int = 17, position_weight: float = 1 / 20, velocity_weight: float = 1 / 160):
        super().__init__(engine, points, position_weight, velocity_weight)
        if not getattr(self.lib, "_sa_pose_bound", False):
            bind(self.lib)
            self.lib._sa_pose_bound = True

    def associate(self, pts=None, present=None, rows=None, comps=2, min_score=0.0, ids=None, threshold=1.0, min_common=1, matrix=False):
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
        o.threshold, o.min_common = threshold, min_common
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

    def track(self, pts, new_ids, present=None, min_score=0.0, threshold=1.0, min_common=1, coast=True):
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
