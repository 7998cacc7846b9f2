"""ctypes mirror of include/similari_framerows.h: a frame's feature rows read from device memory — f32, f16 or bf16, strided and
optionally gathered — by the per-frame association (Engine) and the tracker facade (VisualSort / BatchVisualSort with device upkeep).

A *_rows call returns, and leaves in the engine's track tables, exactly the bits the call without it returns and leaves when it is fed
the same values widened to f32 as host rows.  `rows` is a devrows.DeviceRows; its index has one entry per detection, SA_ROW_NONE for a
detection without a feature.

    with register_tensor(engine, emb):                                  # emb: the ReID head's [B, W] fp16 output on the engine's GPU
        rows = DeviceRows.from_tensor(emb[:, 4:4 + 512], index=owned)   # the scene's rows, in detection order; final before the call
        ids, votes = associate_rows(engine, scene, epoch, abi.make_detections(boxes), rows)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi
from .devrows import DeviceRows, _rows, register_tensor, sa_dev_rows  # noqa: F401  (re-exported: what a caller of this module needs)

u8, u32, u64 = C.c_uint8, C.c_uint32, C.c_uint64
P = C.POINTER
SA_ROW_NONE = 0xFFFFFFFF
ROWS_P = P(sa_dev_rows)


class sa_framerows_stats(C.Structure):
    _fields_ = [("struct_size", u32), ("launches", u32), ("rows", u64), ("wide_rows", u64), ("src_bytes", u64)]


# ---- prototypes of every symbol include/similari_framerows.h declares ------------------------------
PROTOTYPES = {
    "sa_associate_dev": (C.c_int, [abi.ENGINE, u64, u64, P(abi.sa_detections), ROWS_P, P(u64), P(u8)]),
    "sa_batch_add_dev": (C.c_int, [abi.ENGINE, u64, u64, P(abi.sa_detections), ROWS_P, P(u32)]),
    "sa_batch_add_deferred_dev": (C.c_int, [abi.ENGINE, u64, u64, P(abi.sa_detections), ROWS_P, P(u32)]),
    "sa_associate_batch_dev": (C.c_int, [abi.ENGINE, u32, P(abi.sa_scene_request), P(ROWS_P), P(abi.sa_scene_result)]),
    "sa_pipe_stage_dev": (C.c_int, [abi.ENGINE, u32, P(abi.sa_scene_request), P(ROWS_P), P(u64)]),
    "sa_pipe_submit_dev": (C.c_int, [abi.ENGINE, u32, P(abi.sa_scene_request), P(ROWS_P), P(u64)]),
    "sa_tracker_predict_dev": (C.c_int, [C.c_void_p, u64, u32, P(abi.sa_observation), ROWS_P, P(abi.sa_sort_track)]),
    "sa_tracker_predict_batch_begin_dev": (C.c_int, [C.c_void_p, u32, P(u64), P(u32), P(P(abi.sa_observation)), P(ROWS_P), P(C.c_void_p)]),
    "sa_framerows_last": (C.c_int, [abi.ENGINE, P(sa_framerows_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach the prototypes of similari_framerows.h to a library abi.load_library returned."""
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library(path=None) -> C.CDLL:
    return bind(abi.load_library(path))


def _rows_array(rows_list):
    """(keep-alive, sa_dev_rows* array) of a list of DeviceRows / sa_dev_rows / None (a null entry: the scene is staged the old way)."""
    alive = [_rows(r)[0] for r in rows_list]
    arr = (ROWS_P * max(1, len(rows_list)))()
    for i, a in enumerate(alive):
        if a is not None:
            arr[i] = C.pointer(a[1])
    return alive, arr


# ---- the association engine ----
def associate_rows(engine, scene: int, epoch: int, det: abi.sa_detections, rows):
    """Engine.associate with the detections' features described by `rows` (det.feats stays NULL): (ids, votes)."""
    bind(engine.lib)
    ids, votes = np.zeros(det.n, np.uint64), np.zeros(det.n, np.uint8)
    alive, r = _rows(rows)
    engine._chk(engine.lib.sa_associate_dev(engine.h, scene, epoch, C.byref(det), r, ids.ctypes.data_as(P(u64)), votes.ctypes.data_as(P(u8))))
    return ids, votes


def batch_add_rows(engine, scene: int, epoch: int, det: abi.sa_detections, rows, deferred: bool = False) -> int:
    """Engine.batch_add with `rows`; deferred=True: sa_batch_add_deferred_dev (fill the slot with sa_batch_fill before the run)."""
    bind(engine.lib)
    slot = u32()
    alive, r = _rows(rows)
    fn = engine.lib.sa_batch_add_deferred_dev if deferred else engine.lib.sa_batch_add_dev
    engine._chk(fn(engine.h, scene, epoch, C.byref(det), r, C.byref(slot)))
    return slot.value


def make_requests_rows(items):
    """items: [(scene_id, epoch, sa_detections, rows or None)] -> (requests, rows array, results, [(ids, votes)]): Engine.make_requests
    plus the descriptor array of associate_batch_rows / pipe_stage_rows / pipe_submit_rows.  The arrays keep their descriptors alive."""
    from .engine import Engine

    req, res, outs = Engine.make_requests([(s, e, d) for s, e, d, _ in items])
    alive, arr = _rows_array([r for _, _, _, r in items])
    arr._keep = alive
    return req, arr, res, outs


def associate_batch_rows(engine, req, rows, res, n=None):
    bind(engine.lib)
    engine._chk(engine.lib.sa_associate_batch_dev(engine.h, len(req) if n is None else n, req, rows, res))


def pipe_stage_rows(engine, req, rows, n=None) -> int:
    bind(engine.lib)
    t = u64()
    engine._chk(engine.lib.sa_pipe_stage_dev(engine.h, len(req) if n is None else n, req, rows, C.byref(t)))
    return t.value


def pipe_submit_rows(engine, req, rows, n=None) -> int:
    bind(engine.lib)
    t = u64()
    engine._chk(engine.lib.sa_pipe_submit_dev(engine.h, len(req) if n is None else n, req, rows, C.byref(t)))
    return t.value


def framerows_stats(engine) -> dict:
    """sa_framerows_last: the last request-set upload of the engine that had a *_dev slot (zeros before the first)."""
    bind(engine.lib)
    st = sa_framerows_stats()
    engine._chk(engine.lib.sa_framerows_last(engine.h, C.byref(st)))
    return {"launches": int(st.launches), "rows": int(st.rows), "wide_rows": int(st.wide_rows), "src_bytes": int(st.src_bytes)}


# ---- the tracker facade (VisualSort / BatchVisualSort created with device_upkeep=True) ----
def predict_rows(tracker, scene_id: int, items, rows):
    """VisualSort.predict_with_scene with the observations' features described by `rows` (index entry i belongs to items[i]; the
    observations carry feature=None): [SortTrack]."""
    from .trackers import SortTrack

    bind(tracker.lib)
    keep = []
    arr = tracker._obs_array(items, keep)
    out = (abi.sa_sort_track * max(1, len(items)))()
    alive, r = _rows(rows)
    tracker._chk(tracker.lib.sa_tracker_predict_dev(tracker.h, scene_id, len(items), arr, r, out))
    return [SortTrack.from_c(out[i]) for i in range(len(items))]


def predict_batch_rows(tracker, batch, rows):
    """BatchVisualSort.predict_batch_async with `rows`: {scene id: DeviceRows}, one per scene of the request -> PredictionBatchResult."""
    from .trackers import PredictionBatchResult

    bind(tracker.lib)
    scenes = list(batch.scenes.keys())
    keep = []
    arrs = [tracker._obs_array(batch.scenes[s], keep) for s in scenes]
    ids = (u64 * max(1, len(scenes)))(*scenes)
    counts = (u32 * max(1, len(scenes)))(*[len(batch.scenes[s]) for s in scenes])
    pa = (P(abi.sa_observation) * max(1, len(scenes)))(*[C.cast(a, P(abi.sa_observation)) for a in arrs])
    alive, ra = _rows_array([rows.get(s) for s in scenes])
    h = C.c_void_p()
    tracker._chk(tracker.lib.sa_tracker_predict_batch_begin_dev(tracker.h, len(scenes), ids, counts, pa, ra, C.byref(h)))
    return PredictionBatchResult(tracker, h, max([len(batch.scenes[s]) for s in scenes] + [1]), keep)
