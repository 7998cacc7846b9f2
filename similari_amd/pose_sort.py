"""ctypes mirror of include/similari_pose_sort.h (the keypoint tracker: scenes, epochs, idle expiry and the spatio-temporal gate on the
device) and KeypointSort, the Python face of it.

    trk = KeypointSort(engine, points=17, max_idle_epochs=5, constraints=[(1, 1.0), (3, 2.0)])
    per_cam = trk.predict({0: pts0, 1: pts1})            # one C call per frame: {scene: [records]}, one record per pose
    with register_tensor(engine, pose):                  # the poses where the network left them
        per_cam = trk.predict([0, 1], rows=DeviceRows.from_tensor(pose[:, 4:4 + 17 * 3]), pose_counts=[m0, m1], comps=3, min_score=0.3)
    for rec in trk.wasted():                             # the tracks that expired, with their final states
        ...

PoseTrackBank.track_batch with the life cycle kept by the caller returns and leaves the same bits when there are no constraints; it
stays as the yardstick.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from .abi import ENGINE
from .points import POINTS, sa_point_rows
from .pose_oks import default_threshold, set_metric
from .pose_track import PoseTrackBank
from .search import _p

u32, u64 = C.c_uint32, C.c_uint64
P = C.POINTER
SORT = C.c_void_p
SA_POSE_SORT_CONSTRAINTS = 8
SA_POSE_SORT_ALL_SCENES = 0xFFFFFFFFFFFFFFFF


class sa_pose_sort_options(C.Structure):
    _fields_ = [("struct_size", u32), ("points", u32), ("position_weight", C.c_float), ("velocity_weight", C.c_float), ("max_idle_epochs", u32),
                ("min_common", u32), ("threshold", C.c_float), ("coast", u32), ("n_constraints", u32), ("reserved", u32),
                ("epoch_delta", u32 * SA_POSE_SORT_CONSTRAINTS), ("max_dist", C.c_float * SA_POSE_SORT_CONSTRAINTS)]


class sa_pose_sort_track(C.Structure):
    _fields_ = [("id", u64), ("scene", u64), ("epoch", u32), ("length", u32), ("weight", C.c_float), ("created", u32)]


class sa_pose_sort_stats(C.Structure):
    _fields_ = [("struct_size", u32), ("scenes", u32), ("poses", u32), ("tracks", u32), ("vote_launches", u32), ("step_launches", u32),
                ("roots", u32), ("matched", u32), ("created", u32), ("coasted", u32), ("bytes_h2d", u64), ("bytes_d2h", u64), ("src_bytes", u64),
                ("device_ms", C.c_double), ("kernel_ms", C.c_double * 5), ("expired", u32), ("gate_launches", u32), ("refused_pairs", u64),
                ("gate_ms", C.c_double), ("gather_ms", C.c_double)]


TRACK_DTYPE = np.dtype([("id", np.uint64), ("scene", np.uint64), ("epoch", np.uint32), ("length", np.uint32), ("weight", np.float32),
                        ("created", np.uint32)])
assert TRACK_DTYPE.itemsize == C.sizeof(sa_pose_sort_track) == 32

# ---- prototypes of every symbol include/similari_pose_sort.h declares ----------------------------
PROTOTYPES = {
    "sa_pose_sort_options_default": (None, [P(sa_pose_sort_options)]),
    "sa_pose_sort_create": (C.c_int, [ENGINE, P(sa_pose_sort_options), P(SORT)]),
    "sa_pose_sort_destroy": (None, [SORT]),
    "sa_pose_sort_bank": (POINTS, [SORT]),
    "sa_pose_sort_predict": (C.c_int, [SORT, u32, P(u64), P(u32), P(sa_point_rows), C.c_void_p, P(C.c_float)]),
    "sa_pose_sort_peek": (C.c_int, [SORT, u32, P(u64), P(u32), P(sa_point_rows), P(u64), P(C.c_float), P(u32), P(C.c_float)]),
    "sa_pose_sort_peek_cells": (u64, [SORT, u32, P(u64), P(u32)]),
    "sa_pose_sort_wasted_count": (C.c_int, [SORT, P(u32)]),
    "sa_pose_sort_wasted_take": (C.c_int, [SORT, u32, P(u64), P(u64), P(u32), P(u32), P(u32), P(C.c_uint8), P(C.c_float), P(C.c_float), P(u32)]),
    "sa_pose_sort_skip_epochs": (C.c_int, [SORT, u64, u32]),
    "sa_pose_sort_epoch": (C.c_int, [SORT, u64, P(u32)]),
    "sa_pose_sort_active": (C.c_int, [SORT, u64, P(u32)]),
    "sa_pose_sort_last": (C.c_int, [SORT, P(sa_pose_sort_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


Wasted = namedtuple("Wasted", "id scene first_epoch last_epoch length has mean cov")


class _BankView(PoseTrackBank):
    """The tracker's bank: state(), order(), len(), last().  The tracker owns it; closing the view does nothing."""

    def __init__(self, engine, points, handle):   # (no bank is created: the handle is the tracker's)
        self.engine, self.lib, self.P, self.h = engine, engine.lib, int(points), POINTS(handle)
        self.metric = None

    def close(self):
        self.h = POINTS()


class KeypointSort:
    """Sort's life cycle for poses: the tracker owns the bank, the ids, the scenes' epochs and the per-scene track lists."""

    def __init__(self, engine, points: int = 17, max_idle_epochs: int = 5, constraints=(), min_common: int = 1, threshold=None,
                 coast: bool = True, position_weight: float = 1 / 20, velocity_weight: float = 1 / 160, metric=None):
        """metric: None (the mean inverted Mahalanobis cost) or a pose_oks.OksMetric; threshold: None = 1.0, or 0.3 under an OksMetric."""
        self.engine, self.lib, self.P = engine, engine.lib, int(points)
        _bind_all(self.lib)
        o = sa_pose_sort_options()
        self.lib.sa_pose_sort_options_default(C.byref(o))
        o.points, o.position_weight, o.velocity_weight = self.P, position_weight, velocity_weight
        o.max_idle_epochs, o.min_common, o.threshold, o.coast = int(max_idle_epochs), int(min_common), default_threshold(metric, threshold), int(bool(coast))
        constraints = list(constraints)
        o.n_constraints = len(constraints)
        for k, (d, x) in enumerate(constraints[:SA_POSE_SORT_CONSTRAINTS]):
            o.epoch_delta[k], o.max_dist[k] = int(d), float(x)
        self.h = SORT()
        self._chk(self.lib.sa_pose_sort_create(engine.h, C.byref(o), C.byref(self.h)))
        self._bank = _BankView(engine, self.P, self.lib.sa_pose_sort_bank(self.h))
        if metric is not None:
            set_metric(self._bank, metric)

    def _chk(self, rc):
        if rc != 0:
            from .engine import EngineError

            msg = self.lib.sa_last_error(self.engine.h)
            raise EngineError(rc, msg.decode() if msg else "")

    def close(self):
        if self.h:
            self.lib.sa_pose_sort_destroy(self.h)
        self.h = SORT()
        self._bank.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def bank(self) -> PoseTrackBank:
        """The tracker's bank, to read: state(id), order(), len(), last()."""
        return self._bank

    # ---- the arguments of a frame ----
    def _frame(self, scenes, rows, pose_counts, present, comps, min_score):
        if isinstance(scenes, dict):
            assert rows is None and pose_counts is None, "a dict carries its own poses"
            ids = np.array(list(scenes.keys()), np.uint64)
            vals = [v if isinstance(v, tuple) else (v, None) for v in scenes.values()]
            pts_list = [np.asarray(v[0], np.float32) for v in vals]
            comps_in = {p.shape[2] for p in pts_list if p.ndim == 3 and len(p)} or {2}
            assert len(comps_in) == 1, "every scene's poses have 2, or every scene's have 3, components"
            c = comps_in.pop()
            pts_list = [p.reshape(-1, self.P, c) for p in pts_list]
            pc = np.array([len(p) for p in pts_list], np.uint32)
            masked = [v[1] is not None for v in vals]
            assert all(masked) or not any(masked), "a present mask for every scene or for none"
            pts = np.concatenate(pts_list) if pts_list else np.zeros((0, self.P, c), np.float32)
            if pts_list and any(masked):
                present = np.concatenate([np.asarray(v[1]).reshape(-1, self.P) != 0 for v in vals])
        else:
            assert rows is not None and pose_counts is not None, "scene ids come with rows= and pose_counts="
            ids = np.ascontiguousarray(scenes, np.uint64).reshape(-1)
            pc = np.ascontiguousarray(pose_counts, np.uint32).reshape(-1)
            pts = None
        assert len(ids) == len(pc), "one pose count per scene"
        m = int(pc.sum())
        alive, r = self._bank._source(m, pts, present, rows, comps, min_score)
        return ids, pc, m, alive, r

    def predict(self, scenes, rows=None, pose_counts=None, present=None, comps=2, min_score=0.0, xy=False):
        """One frame.  scenes: {scene id: pts [m_s, P, 2 or 3]} or {scene id: (pts, present)}; or a list of scene ids with rows= (a
        DeviceRows whose rows, or index, list the poses of the whole call scene after scene), pose_counts= and, optionally, present=
        [sum m, P].  -> {scene id: records [m_s]} — a structured array with id, scene, epoch, length, weight, created —; with xy=True
        {scene id: (records, xy [m_s, P, 2])}, the step's means."""
        ids, pc, m, alive, r = self._frame(scenes, rows, pose_counts, present, comps, min_score)
        out = np.zeros(max(m, 1), TRACK_DTYPE)
        out_xy = np.empty((max(m, 1), self.P, 2), np.float32) if xy else None
        self._chk(self.lib.sa_pose_sort_predict(self.h, len(ids), _p(ids, u64), _p(pc, u32), C.byref(r), out.ctypes.data, _p(out_xy, C.c_float)))
        ends = np.cumsum(pc, dtype=np.int64)[:-1]
        recs = np.split(out[:m], ends) if len(ids) else []
        if xy:
            return {int(s): (a, b) for s, a, b in zip(ids, recs, np.split(out_xy[:m], ends))}
        return {int(s): a for s, a in zip(ids, recs)}

    def peek(self, scenes, rows=None, pose_counts=None, present=None, comps=2, min_score=0.0, matrix=False):
        """The vote of the predict that would come next; changes nothing.  -> {scene id: (track ids [m_s] u64, 0 = the pose would
        create a track; weights [m_s] f32)}; with matrix=True (track ids, weights, tap [m_s, tracks of the scene])."""
        ids, pc, m, alive, r = self._frame(scenes, rows, pose_counts, present, comps, min_score)
        S = len(ids)
        out_t, out_w = np.zeros(max(m, 1), np.uint64), np.full(max(m, 1), np.nan, np.float32)
        tc = np.zeros(max(S, 1), np.uint32)
        tap = None
        if matrix:
            cells = int(self.lib.sa_pose_sort_peek_cells(self.h, S, _p(ids, u64), _p(pc, u32)))
            tap = np.full(max(cells, 1), np.nan, np.float32)
        self._chk(self.lib.sa_pose_sort_peek(self.h, S, _p(ids, u64), _p(pc, u32), C.byref(r), _p(out_t, u64), _p(out_w, C.c_float), _p(tc, u32),
                                            _p(tap, C.c_float)))
        p0 = np.concatenate([[0], np.cumsum(pc, dtype=np.int64)])
        c0 = np.concatenate([[0], np.cumsum(pc.astype(np.int64) * tc[:S].astype(np.int64))])
        out = {}
        for s in range(S):
            got = (out_t[p0[s]: p0[s + 1]], out_w[p0[s]: p0[s + 1]])
            out[int(ids[s])] = got + (tap[c0[s]: c0[s + 1]].reshape(int(pc[s]), int(tc[s])),) if matrix else got
        return out

    def wasted(self) -> list:
        """The tracks that expired since the last call, oldest first, with their final states (has [P] bool, mean [P, 4], cov
        [P, 4, 4]; NaN where a point has no state); the list is emptied."""
        n = u32()
        self._chk(self.lib.sa_pose_sort_wasted_count(self.h, C.byref(n)))
        n = n.value
        if n == 0:
            return []
        ids, scenes = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        first, last, length = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        has, mean, cov = np.zeros((n, self.P), np.uint8), np.empty((n, self.P, 4), np.float32), np.empty((n, self.P, 4, 4), np.float32)
        got = u32()
        self._chk(self.lib.sa_pose_sort_wasted_take(self.h, n, _p(ids, u64), _p(scenes, u64), _p(first, u32), _p(last, u32), _p(length, u32),
                                                   _p(has, C.c_uint8), _p(mean, C.c_float), _p(cov, C.c_float), C.byref(got)))
        return [Wasted(int(ids[k]), int(scenes[k]), int(first[k]), int(last[k]), int(length[k]), has[k].astype(bool), mean[k], cov[k])
                for k in range(got.value)]

    def skip_epochs(self, scene, n: int = 1):
        self._chk(self.lib.sa_pose_sort_skip_epochs(self.h, int(scene), int(n)))

    def epoch(self, scene) -> int:
        e = u32()
        self._chk(self.lib.sa_pose_sort_epoch(self.h, int(scene), C.byref(e)))
        return e.value

    def active(self, scene=None) -> int:
        n = u32()
        self._chk(self.lib.sa_pose_sort_active(self.h, SA_POSE_SORT_ALL_SCENES if scene is None else int(scene), C.byref(n)))
        return n.value

    def last(self) -> dict:
        """The fields of sa_pose_sort_stats of the last predict or peek."""
        st = sa_pose_sort_stats()
        self._chk(self.lib.sa_pose_sort_last(self.h, C.byref(st)))
        out = {f: getattr(st, f) for f, _ in sa_pose_sort_stats._fields_}
        out["kernel_ms"] = list(st.kernel_ms)
        return out


def _bind_all(lib):
    """the prototypes of the bank's headers and of this one, once per library"""
    from . import points as _points
    from . import pose as _pose
    from . import pose_track as _pose_track

    for flag, mod in (("_sa_points_bound", _points), ("_sa_pose_bound", _pose), ("_sa_pose_track_bound", _pose_track), ("_sa_pose_sort_bound", None)):
        if not getattr(lib, flag, False):
            (mod.bind if mod else bind)(lib)
            setattr(lib, flag, True)
