"""ctypes mirror of include/similari_points.h (point banks: the 2D point-vector Kalman filter for the keypoints of many tracks, on the
device) and PointBank, the Python face of it.

A PointBank keeps the Kalman states of T tracks x P keypoints on an Engine's GPU, keyed by track id, and steps them in one launch per
call.  The points of a call are an [n, P, comps] float array (comps 2: x, y; 3: x, y, score) with an optional [n, P] `present` mask, or
`rows=`, a devrows.DeviceRows over the pose network's output where it lies (f32, f16 or bf16, strided, gathered by a row index):

    bank = PointBank(engine, points=17)
    xy = bank.step(ids, pts)                       # initiate what is first sighted, predict, update: [n, 17, 2], NaN = no state yet
    with register_tensor(engine, pose):            # pose: a [B, W] fp16 tensor on the engine's GPU
        xy = bank.step(ids, rows=DeviceRows.from_tensor(pose[:, 4:4 + 17 * 3], index=det_of_track), comps=3, min_score=0.3)
    bank.predict(idle_ids)                         # tracks without a detection coast
    bank.remove(wasted_ids)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import devrows as _devrows
from . import framerows as _framerows
from .abi import ENGINE
from .devrows import sa_dev_rows
from .search import _p

u32, u64 = C.c_uint32, C.c_uint64
P = C.POINTER
POINTS = C.c_void_p
SA_POINT_D2, SA_POINT_COST, SA_POINT_COST_INVERTED = 0, 1, 2
MODE = {"d2": SA_POINT_D2, "cost": SA_POINT_COST, "cost_inverted": SA_POINT_COST_INVERTED}
SA_ROW_NONE = 0xFFFFFFFF


class sa_points_options(C.Structure):
    _fields_ = [("struct_size", u32), ("points", u32), ("position_weight", C.c_float), ("velocity_weight", C.c_float)]


class sa_point_rows(C.Structure):
    _fields_ = [("struct_size", u32), ("comps", u32), ("min_score", C.c_float), ("reserved", u32), ("host", P(C.c_float)),
                ("present", P(C.c_uint8)), ("dev", P(sa_dev_rows))]


class sa_points_stats(C.Structure):
    _fields_ = [("struct_size", u32), ("tracks", u32), ("launches", u32), ("capacity", u32), ("points", u64), ("present", u64),
                ("bytes_h2d", u64), ("bytes_d2h", u64), ("src_bytes", u64), ("device_ms", C.c_double)]


# ---- prototypes of every symbol include/similari_points.h declares -------------------------------
PROTOTYPES = {
    "sa_points_options_default": (None, [P(sa_points_options)]),
    "sa_points_create": (C.c_int, [ENGINE, P(sa_points_options), P(POINTS)]),
    "sa_points_destroy": (None, [POINTS]),
    "sa_points_initiate": (C.c_int, [POINTS, u32, P(u64), P(sa_point_rows)]),
    "sa_points_predict": (C.c_int, [POINTS, u32, P(u64), P(C.c_float)]),
    "sa_points_update": (C.c_int, [POINTS, u32, P(u64), P(sa_point_rows), P(C.c_float)]),
    "sa_points_distance": (C.c_int, [POINTS, u32, P(u64), P(sa_point_rows), u32, P(C.c_float)]),
    "sa_points_step": (C.c_int, [POINTS, u32, P(u64), P(sa_point_rows), P(C.c_float)]),
    "sa_points_remove": (C.c_int, [POINTS, u32, P(u64)]),
    "sa_points_count": (C.c_int, [POINTS, P(u32)]),
    "sa_points_order": (C.c_int, [POINTS, P(u64), u32, P(u32)]),
    "sa_points_get_state": (C.c_int, [POINTS, u64, P(C.c_uint8), P(C.c_float), P(C.c_float)]),
    "sa_points_set_state": (C.c_int, [POINTS, u64, P(C.c_uint8), P(C.c_float), P(C.c_float)]),
    "sa_points_last": (C.c_int, [POINTS, P(sa_points_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach the prototypes of similari_devrows.h, similari_framerows.h and similari_points.h to a library abi.load_library returned."""
    _devrows.bind(lib)
    _framerows.bind(lib)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library(path=None) -> C.CDLL:
    from . import abi

    return bind(abi.load_library(path))


def point_rows(n, points, pts, present, rows, comps, min_score):
    """-> (keep-alive, sa_point_rows) of n items x `points` keypoints: a host array [n, points, 2 or 3], or rows= a DeviceRows (or its
    sa_dev_rows) of points * comps elements per row.  What every keypoint call — the bank's, the vote's, pose NMS — hands the library."""
    assert (pts is None) != (rows is None), "the points come as an array or as rows=, not both"
    mask = None if present is None else np.ascontiguousarray(np.asarray(present) != 0, np.uint8).reshape(-1)
    assert mask is None or len(mask) == n * points, "one present flag per point"
    min_score = 0.0 if min_score is None else min_score
    if rows is None:
        pts = np.ascontiguousarray(pts, np.float32)
        assert pts.ndim == 3 and pts.shape[:2] == (n, points) and pts.shape[2] in (2, 3), "points are [n, P, 2 or 3]"
        r = sa_point_rows(C.sizeof(sa_point_rows), pts.shape[2], min_score, 0, _p(pts, C.c_float), _p(mask, C.c_uint8), None)
        return (pts, mask), r
    st = rows if isinstance(rows, sa_dev_rows) else rows.struct()
    r = sa_point_rows(C.sizeof(sa_point_rows), int(comps), min_score, 0, None, _p(mask, C.c_uint8), C.pointer(st))
    return (rows, st, mask), r


class PointBank:
    """The Kalman states of T tracks x `points` keypoints, resident on the engine's GPU."""

    def __init__(self, engine, points: int = 17, position_weight: float = 1 / 20, velocity_weight: float = 1 / 160):
        self.engine = engine
        self.lib = engine.lib
        if not getattr(self.lib, "_sa_points_bound", False):
            bind(self.lib)
            self.lib._sa_points_bound = True
        self.P = int(points)
        o = sa_points_options()
        self.lib.sa_points_options_default(C.byref(o))
        o.points = self.P
        o.position_weight = position_weight
        o.velocity_weight = velocity_weight
        self.h = POINTS()
        self._chk(self.lib.sa_points_create(engine.h, C.byref(o), C.byref(self.h)))

    def _chk(self, rc):
        if rc != 0:
            from .engine import EngineError

            msg = self.lib.sa_last_error(self.engine.h)
            raise EngineError(rc, msg.decode() if msg else "")

    def close(self):
        if self.h:
            self.lib.sa_points_destroy(self.h)
        self.h = POINTS()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        n = u32()
        self._chk(self.lib.sa_points_count(self.h, C.byref(n)))
        return n.value

    # ---- the arguments of a call ----
    @staticmethod
    def _ids(ids):
        return np.ascontiguousarray(ids, np.uint64).reshape(-1)

    def _source(self, n, pts, present, rows, comps, min_score):
        """-> (keep-alive, sa_point_rows) of a host array [n, P, comps] or a DeviceRows."""
        return point_rows(n, self.P, pts, present, rows, comps, min_score)

    def _xy(self, n):
        return np.empty((n, self.P, 2), np.float32)

    # ---- the calls ----
    def initiate(self, ids, pts=None, present=None, rows=None, comps=2, min_score=0.0):
        """Unknown ids are created; every present point gets initiate(z), an absent one keeps what it has."""
        ids = self._ids(ids)
        alive, r = self._source(len(ids), pts, present, rows, comps, min_score)
        self._chk(self.lib.sa_points_initiate(self.h, len(ids), _p(ids, u64), C.byref(r)))

    def predict(self, ids=None):
        """Every point with a state is predicted -> [n, P, 2] the new x, y (NaN: no state).  ids None: every track, in order() order."""
        if ids is None:
            out = self._xy(len(self))
            self._chk(self.lib.sa_points_predict(self.h, 0, None, _p(out, C.c_float)))
            return out
        ids = self._ids(ids)
        out = self._xy(len(ids))
        self._chk(self.lib.sa_points_predict(self.h, len(ids), _p(ids, u64), _p(out, C.c_float)))
        return out

    def update(self, ids, pts=None, present=None, rows=None, comps=2, min_score=0.0):
        ids = self._ids(ids)
        alive, r = self._source(len(ids), pts, present, rows, comps, min_score)
        out = self._xy(len(ids))
        self._chk(self.lib.sa_points_update(self.h, len(ids), _p(ids, u64), C.byref(r), _p(out, C.c_float)))
        return out

    def distance(self, ids, pts=None, present=None, rows=None, comps=2, min_score=0.0, mode="d2"):
        """-> [n, P] d^2 ("d2"), calculate_cost(d^2, False) ("cost") or calculate_cost(d^2, True) ("cost_inverted"); NaN where the
        point is absent or has no state.  mode may also be the raw integer."""
        ids = self._ids(ids)
        alive, r = self._source(len(ids), pts, present, rows, comps, min_score)
        out = np.empty((len(ids), self.P), np.float32)
        self._chk(self.lib.sa_points_distance(self.h, len(ids), _p(ids, u64), C.byref(r), MODE[mode] if isinstance(mode, str) else int(mode),
                                             _p(out, C.c_float)))
        return out

    def step(self, ids, pts=None, present=None, rows=None, comps=2, min_score=0.0):
        """make_prediction for every point: initiate what is first sighted, predict what has a state, update what is present."""
        ids = self._ids(ids)
        alive, r = self._source(len(ids), pts, present, rows, comps, min_score)
        out = self._xy(len(ids))
        self._chk(self.lib.sa_points_step(self.h, len(ids), _p(ids, u64), C.byref(r), _p(out, C.c_float)))
        return out

    def remove(self, ids):
        ids = self._ids(ids)
        self._chk(self.lib.sa_points_remove(self.h, len(ids), _p(ids, u64)))

    def order(self) -> np.ndarray:
        n = len(self)
        out = np.zeros(max(n, 1), np.uint64)
        got = u32()
        self._chk(self.lib.sa_points_order(self.h, _p(out, u64), n, C.byref(got)))
        return out[:n]

    def state(self, track_id):
        """-> (has [P] bool, mean [P, 4], cov [P, 4, 4]); mean and cov are NaN where the point has no state."""
        has = np.zeros(self.P, np.uint8)
        mean = np.empty((self.P, 4), np.float32)
        cov = np.empty((self.P, 4, 4), np.float32)
        self._chk(self.lib.sa_points_get_state(self.h, int(track_id), _p(has, C.c_uint8), _p(mean, C.c_float), _p(cov, C.c_float)))
        return has.astype(bool), mean, cov

    def set_state(self, track_id, has, mean, cov):
        has = np.ascontiguousarray(np.asarray(has) != 0, np.uint8).reshape(-1)
        mean = np.ascontiguousarray(mean, np.float32).reshape(-1)
        cov = np.ascontiguousarray(cov, np.float32).reshape(-1)
        assert len(has) == self.P and len(mean) == self.P * 4 and len(cov) == self.P * 16, "has [P], mean [P, 4], cov [P, 4, 4]"
        self._chk(self.lib.sa_points_set_state(self.h, int(track_id), _p(has, C.c_uint8), _p(mean, C.c_float), _p(cov, C.c_float)))

    def last(self) -> dict:
        """The fields of sa_points_stats of the last call that launched."""
        st = sa_points_stats()
        self._chk(self.lib.sa_points_last(self.h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in sa_points_stats._fields_}
