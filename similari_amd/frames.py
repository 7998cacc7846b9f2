"""ctypes mirror of include/similari_frames.h: Engine.own_areas and Engine.nms over a whole batch of scenes in one call — one
upload, launches whose number does not depend on the number of scenes, one copy back.

    shares = own_areas_batch(engine, [boxes_of_scene_0, boxes_of_scene_1, ...])        # [f32 per box], one array per scene
    keeps = nms_batch(engine, [boxes_0, ...], [scores_0, None, ...], 0.5, 0.2)          # [indices in the reference's order]
    last_stats(engine)                                                                  # what that call cost

Scene s of a batch call returns what the single call on scene s returns; a scene may be empty.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi

u32, u64 = C.c_uint32, C.c_uint64
P = C.POINTER
BOX_P, F32_P, U32_P = P(abi.sa_box), P(C.c_float), P(u32)


class sa_frames_stats(C.Structure):
    _fields_ = [("struct_size", u32), ("scenes", u32), ("boxes", u32), ("launches", u32), ("spilled", u32), ("host_waits", u32),
                ("bytes_h2d", u64), ("bytes_d2h", u64), ("device_ms", C.c_double)]


# ---- prototypes of every symbol include/similari_frames.h declares ---------------------------------
PROTOTYPES = {
    "sa_own_areas_batch": (C.c_int, [abi.ENGINE, u32, U32_P, P(BOX_P), P(F32_P)]),
    "sa_nms_batch": (C.c_int, [abi.ENGINE, u32, U32_P, P(BOX_P), P(F32_P), C.c_float, C.c_float, P(U32_P), U32_P]),
    "sa_frames_last": (C.c_int, [abi.ENGINE, P(sa_frames_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach the prototypes of similari_frames.h to a library abi.load_library returned."""
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library(path=None) -> C.CDLL:
    return bind(abi.load_library(path))


def _scene_arrays(scenes):
    """(box arrays kept alive, counts, pointer array) of a list of per-scene box arrays; an empty scene gets a null pointer."""
    boxes = [np.ascontiguousarray(b, abi.BOX_DTYPE) for b in scenes]
    n = max(1, len(boxes))
    counts = (u32 * n)(*[len(b) for b in boxes])
    ptrs = (BOX_P * n)()
    for s, b in enumerate(boxes):
        if len(b):
            ptrs[s] = C.cast(b.ctypes.data, BOX_P)
    return boxes, counts, ptrs


def own_areas_batch(engine, scenes, out=None):
    """Engine.own_areas of every scene of `scenes` (a list of box arrays) in one call: a list of f32 arrays, one share per box.
    out: arrays to write into instead of fresh ones (they stay untouched when the call is refused)."""
    bind(engine.lib)
    boxes, counts, ptrs = _scene_arrays(scenes)
    if out is None:
        out = [np.zeros(len(b), np.float32) for b in boxes]
    outs = (F32_P * max(1, len(boxes)))()
    for s, o in enumerate(out):
        assert o.dtype == np.float32 and o.flags.c_contiguous and len(o) >= len(boxes[s])
        if len(boxes[s]):
            outs[s] = o.ctypes.data_as(F32_P)
    engine._chk(engine.lib.sa_own_areas_batch(engine.h, len(boxes), counts, ptrs, outs))
    return out


def nms_batch(engine, scenes, scores=None, nms_threshold: float = 0.5, score_threshold=None, out=None, out_n=None):
    """Engine.nms of every scene of `scenes` in one call: a list of index arrays in the reference's output order (rank descending).
    scores: None, or one entry per scene, each an array or None.  out / out_n: uint32 arrays to write into (a per-scene list and one
    array of len(scenes)) instead of fresh ones; they stay untouched when the call is refused."""
    bind(engine.lib)
    boxes, counts, ptrs = _scene_arrays(scenes)
    n = max(1, len(boxes))
    sc_alive, sc_ptrs = [], None
    if scores is not None:
        assert len(scores) == len(boxes)
        sc_ptrs = (F32_P * n)()
        for s, sc in enumerate(scores):
            if sc is not None and len(boxes[s]):
                a = np.ascontiguousarray(sc, np.float32)
                assert len(a) == len(boxes[s])
                sc_alive.append(a)
                sc_ptrs[s] = a.ctypes.data_as(F32_P)
    if out is None:
        out = [np.zeros(len(b), np.uint32) for b in boxes]
    if out_n is None:
        out_n = np.zeros(n, np.uint32)
    keeps = (U32_P * n)()
    for s, o in enumerate(out):
        assert o.dtype == np.uint32 and o.flags.c_contiguous and len(o) >= len(boxes[s])
        if len(boxes[s]):
            keeps[s] = o.ctypes.data_as(U32_P)
    engine._chk(engine.lib.sa_nms_batch(engine.h, len(boxes), counts, ptrs, sc_ptrs, nms_threshold,
                                        float("nan") if score_threshold is None else score_threshold, keeps, out_n.ctypes.data_as(U32_P)))
    return [o[: int(out_n[s])].copy() for s, o in enumerate(out)]


def last_stats(engine) -> dict:
    """sa_frames_last: the last own_areas_batch / nms_batch of the engine (zeros before the first and after a refused one)."""
    bind(engine.lib)
    st = sa_frames_stats()
    engine._chk(engine.lib.sa_frames_last(engine.h, C.byref(st)))
    return {k: getattr(st, k) for k, _ in sa_frames_stats._fields_ if k != "struct_size"}
