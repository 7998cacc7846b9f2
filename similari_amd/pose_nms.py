"""ctypes mirror of include/similari_pose_nms.h: non-maximum suppression of poses by object keypoint similarity on the engine's GPU, for
one scene or a whole batch of scenes in one call — what Engine.nms / frames.nms_batch are for boxes, in front of the keypoint tracker.

    keep = pose_nms(engine, pts, scores, nms_threshold=0.7)              # pts [m, 17, 2 or 3]; -> uint32 indices, best score first
    keeps = pose_nms_batch(engine, [(pts_0, scores_0), (pts_1, scores_1, present_1), ...])
    with register_tensor(engine, pose):                                  # the pose network's [B, W] tensor, where it lies
        rows = DeviceRows.from_tensor(pose[:, 4:4 + 17 * 3])
        keep = pose_nms(engine, None, scores, rows=rows, comps=3, min_score=0.3)
        tracks = sort.predict([scene], rows=keep_rows(rows, keep), pose_counts=[len(keep)], comps=3, min_score=0.3)   # nothing was copied
    order, w = pose_nms_matrix(engine, pts, scores)                      # the pairs themselves, for parity tests
    last(engine)                                                         # what the last call cost
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi
from .devrows import DeviceRows
from .points import SA_ROW_NONE, point_rows, sa_point_rows
from .pose_oks import COCO_SIGMAS
from .search import _p

u32, u64 = C.c_uint32, C.c_uint64
P = C.POINTER
F32_P, U32_P = P(C.c_float), P(u32)
SA_POSE_NMS_MAX_SCENES, SA_POSE_NMS_MAX, SA_POSE_NMS_TAP_MAX = 65535, 16384, 2048


class sa_pose_nms_options(C.Structure):
    _fields_ = [("struct_size", u32), ("points", u32), ("min_common", u32), ("n_sigmas", u32), ("sigmas", F32_P),
                ("nms_threshold", C.c_float), ("score_threshold", C.c_float)]


class sa_pose_nms_stats(C.Structure):
    _fields_ = [("struct_size", u32), ("scenes", u32), ("poses", u32), ("launches", u32), ("host_waits", u32), ("reserved", u32),
                ("bytes_h2d", u64), ("bytes_d2h", u64), ("src_bytes", u64), ("device_ms", C.c_double)]


# ---- prototypes of every symbol include/similari_pose_nms.h declares -----------------------------
PROTOTYPES = {
    "sa_pose_nms_options_default": (None, [P(sa_pose_nms_options)]),
    "sa_pose_nms": (C.c_int, [abi.ENGINE, P(sa_pose_nms_options), u32, P(sa_point_rows), F32_P, U32_P, U32_P]),
    "sa_pose_nms_batch": (C.c_int, [abi.ENGINE, P(sa_pose_nms_options), u32, U32_P, P(sa_point_rows), F32_P, P(U32_P), U32_P]),
    "sa_pose_nms_matrix": (C.c_int, [abi.ENGINE, P(sa_pose_nms_options), u32, P(sa_point_rows), F32_P, U32_P, F32_P, U32_P]),
    "sa_pose_nms_last": (C.c_int, [abi.ENGINE, P(sa_pose_nms_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


def _bound(lib):
    if not getattr(lib, "_sa_pose_nms_bound", False):
        bind(lib)
        lib._sa_pose_nms_bound = True
    return lib


def options(lib, sigmas=COCO_SIGMAS, nms_threshold=0.9, score_threshold=None, min_common=1):
    """-> (keep-alive, sa_pose_nms_options) for poses of len(sigmas) points."""
    sig = np.ascontiguousarray(sigmas, np.float32).reshape(-1)
    o = sa_pose_nms_options()
    _bound(lib).sa_pose_nms_options_default(C.byref(o))
    o.points = o.n_sigmas = len(sig)
    o.sigmas = sig.ctypes.data_as(F32_P)
    o.min_common = int(min_common)
    o.nms_threshold = nms_threshold
    o.score_threshold = float("nan") if score_threshold is None else score_threshold
    return sig, o


def _scores(scores, n):
    sc = np.ascontiguousarray(scores, np.float32).reshape(-1)
    assert len(sc) == n, "one score per pose"
    return sc


def pose_nms(engine, pts, scores, sigmas=COCO_SIGMAS, nms_threshold=0.9, score_threshold=None, min_common=1, present=None, min_score=None,
             rows=None, comps=2):
    """OKS-NMS of one scene -> np.uint32 indices of the kept poses, in rank order (best score first).  pts: [m, P, 2 or 3], or None with
    rows= a DeviceRows of P * comps elements per row (comps: 2 or 3)."""
    lib = _bound(engine.lib)
    sc = _scores(scores, len(scores))
    m = len(sc)
    sig, o = options(lib, sigmas, nms_threshold, score_threshold, min_common)
    alive, r = point_rows(m, o.points, pts, present, rows, comps, min_score)
    keep = np.zeros(max(m, 1), np.uint32)
    n = u32()
    engine._chk(lib.sa_pose_nms(engine.h, C.byref(o), m, C.byref(r), _p(sc, C.c_float), _p(keep, u32), C.byref(n)))
    return keep[: n.value].copy()


def pose_nms_batch(engine, scenes, sigmas=COCO_SIGMAS, nms_threshold=0.9, score_threshold=None, min_common=1, min_score=None, rows=None, comps=2):
    """OKS-NMS of every scene in one call -> a list of np.uint32 index arrays (into each scene), in rank order.  scenes: a list of
    (pts, scores[, present]); with rows= (one DeviceRows over the poses of all scenes, scene after scene) pts is None in every entry."""
    lib = _bound(engine.lib)
    sig, o = options(lib, sigmas, nms_threshold, score_threshold, min_common)
    Pn = o.points
    counts = np.array([len(np.asarray(s[1]).reshape(-1)) for s in scenes], np.uint32)
    total, S = int(counts.sum()), len(scenes)
    sc = _scores(np.concatenate([np.asarray(s[1], np.float32).reshape(-1) for s in scenes]) if S else [], total)
    masked = any(len(s) > 2 and s[2] is not None for s in scenes)
    present = None
    if masked:
        present = np.concatenate([np.ones((counts[k], Pn), bool) if len(s) < 3 or s[2] is None else np.asarray(s[2]).reshape(counts[k], Pn) != 0
                                  for k, s in enumerate(scenes)])
    pts = None
    if rows is None:
        arrs = [np.asarray(s[0], np.float32) for k, s in enumerate(scenes) if counts[k]]
        pts = np.concatenate(arrs) if arrs else np.zeros((0, Pn, 2), np.float32)
    alive, r = point_rows(total, Pn, pts, present, rows, comps, min_score)
    outs = [np.zeros(max(int(c), 1), np.uint32) for c in counts]
    ptrs = (U32_P * max(S, 1))(*[a.ctypes.data_as(U32_P) for a in outs])
    out_n = np.zeros(max(S, 1), np.uint32)
    engine._chk(lib.sa_pose_nms_batch(engine.h, C.byref(o), S, _p(counts, u32), C.byref(r), _p(sc, C.c_float), ptrs, _p(out_n, u32)))
    return [a[: int(out_n[k])].copy() for k, a in enumerate(outs)]


def pose_nms_matrix(engine, pts, scores, sigmas=COCO_SIGMAS, score_threshold=None, min_common=1, present=None, min_score=None, rows=None, comps=2):
    """The parity tap of one scene -> (order [m'] uint32: the caller's indices in rank order, w [m', m'] f32: w for i < j, NaN elsewhere
    and for a pair that does not exist or is refused)."""
    lib = _bound(engine.lib)
    sc = _scores(scores, len(scores))
    m = len(sc)
    sig, o = options(lib, sigmas, 0.9, score_threshold, min_common)
    alive, r = point_rows(m, o.points, pts, present, rows, comps, min_score)
    cap = max(1, min(m, SA_POSE_NMS_TAP_MAX))
    order, w, n = np.zeros(cap, np.uint32), np.zeros((cap, cap), np.float32), u32()
    engine._chk(lib.sa_pose_nms_matrix(engine.h, C.byref(o), m, C.byref(r), _p(sc, C.c_float), _p(order, u32), _p(w, C.c_float), C.byref(n)))
    k = n.value
    return order[:k].copy(), w.reshape(-1)[: k * k].reshape(k, k).copy()


def last(engine) -> dict:
    """sa_pose_nms_last: the last pose_nms / pose_nms_batch / pose_nms_matrix of the engine (zeros before the first and after a refused one)."""
    lib = _bound(engine.lib)
    st = sa_pose_nms_stats()
    engine._chk(lib.sa_pose_nms_last(engine.h, C.byref(st)))
    return {k: getattr(st, k) for k, _ in sa_pose_nms_stats._fields_ if k not in ("struct_size", "reserved")}


def keep_rows(rows: DeviceRows, keep) -> DeviceRows:
    """The DeviceRows of the survivors: `rows` with its index composed with the kept indices, so that row i of the result is pose
    keep[i] of `rows`.  Nothing on the device is touched or copied: KeypointSort.predict takes the result as it takes `rows`."""
    keep = np.ascontiguousarray(keep, np.uint32).reshape(-1)
    index = keep if rows.index is None else rows.index[keep]
    return DeviceRows(rows.ptr, rows.n_rows, rows.row_stride, rows.elem, index.copy())


__all__ = ["pose_nms", "pose_nms_batch", "pose_nms_matrix", "last", "keep_rows", "options", "bind", "PROTOTYPES", "sa_pose_nms_options",
           "sa_pose_nms_stats", "COCO_SIGMAS", "SA_ROW_NONE", "SA_POSE_NMS_MAX", "SA_POSE_NMS_MAX_SCENES", "SA_POSE_NMS_TAP_MAX"]
