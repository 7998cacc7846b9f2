"""ctypes mirror of include/similari_waste.h (wasted tracker tracks enter a feature store on the device) and the functions that are
the Python face of it.  They work on an Engine and any store object of the chain (FeatureStore .. I8Store) created on it.

The reference joins a tracker and the track search by wasted(), which returns whole tracks; here the leaving tracks' feature banks go
from the engine's table into the store without crossing the bus, and the tracks leave the table:

    n_obs = waste.waste(engine, temp, {scene: ids}, keep="latest")                # append: {id: observations it brought}
    winners, dest = waste.waste_absorb(engine, gallery, {scene: ids}, topn=1, max_distance=0.3, keep="best")
    waste.last(gallery)                                                           # tracks, rows, launches_capture; feature bytes 0

    tracker.waste_into(gallery, keep="best")       # trackers.VisualSort / BatchVisualSort: every track that leaves, from now on
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import attrs as _attrs
from . import consolidate as _consolidate
from .absorb import AbsorbStore
from .abi import ENGINE
from .attrs import sa_compat, sa_track_attrs
from .merge import _keep
from .search import STORE, _p, sa_topn_params

u32, u64 = C.c_uint32, C.c_uint64
P = C.POINTER


class sa_waste_stats(C.Structure):
    _fields_ = [("struct_size", u32), ("tracks", u32), ("launches_capture", u32), ("reserved", u32), ("rows", u64),
                ("feature_bytes_h2d", u64), ("feature_bytes_d2h", u64), ("table_bytes_d2h", u64), ("capture_ms", C.c_double)]


# ---- prototypes of every symbol include/similari_waste.h declares --------------------------------
PROTOTYPES = {
    "sa_tracks_waste": (C.c_int, [ENGINE, STORE, u32, u32, P(u64), P(u32), P(P(u64)), P(u32), P(u32)]),
    "sa_tracks_waste_absorb": (C.c_int, [ENGINE, STORE, u32, P(sa_topn_params), P(sa_compat), u32, P(u64), P(u32), P(P(u64)), P(sa_track_attrs),
                                         P(u32), P(u32), P(u64), P(u64), P(C.c_double), P(u64)]),
    "sa_tracker_waste_into": (C.c_int, [C.c_void_p, STORE, u32, u32]),
    "sa_store_waste_last": (C.c_int, [STORE, P(sa_waste_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach the prototypes of similari_search.h .. similari_waste.h to a library abi.load_library returned."""
    _consolidate.bind(lib)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library(path=None) -> C.CDLL:
    from . import abi

    return bind(abi.load_library(path))


def _lib(store) -> C.CDLL:
    """The store's (or the tracker's) library with this header's prototypes attached (once per library)."""
    lib = store.lib
    if not getattr(lib, "_sa_waste_bound", False):
        bind(lib)
        lib._sa_waste_bound = True
    return lib


def _scenes(leaving):
    """{scene: ids} (or a list of (scene, ids), which may name a scene twice) -> the call's scene arrays, kept alive by the tuple."""
    items = list(leaving.items()) if isinstance(leaving, dict) else list(leaving)
    lists = [np.ascontiguousarray(ids, np.uint64).reshape(-1) for _, ids in items]
    scene_ids = np.array([int(s) for s, _ in items], np.uint64)
    counts = np.array([len(x) for x in lists], np.uint32)
    ptrs = (P(u64) * max(len(items), 1))(*[_p(x, u64) if len(x) else P(u64)() for x in lists])
    flat = np.concatenate(lists) if lists else np.zeros(0, np.uint64)
    return len(items), scene_ids, counts, ptrs, flat, lists


def _capacity(capacity, n):
    if capacity is None:
        return None
    if np.ndim(capacity) == 0:
        return np.full(max(n, 1), int(capacity), np.uint32)
    cap = np.ascontiguousarray(capacity, np.uint32).reshape(-1)
    assert len(cap) == n, "one capacity per id"
    return cap


def waste_raw(engine, store, leaving, keep="latest", capacity=None):
    """-> (ids [n] flattened in call order, n_obs [n]) as sa_tracks_waste writes them.  capacity: None (the store's K), one int, or one
    per id.  (A refusal's text lies in the engine's error slot: the call is the engine's.)"""
    lib = _lib(store)
    ns, scene_ids, counts, ptrs, flat, alive = _scenes(leaving)
    n = len(flat)
    n_obs = np.zeros(max(n, 1), np.uint32)
    engine._chk(lib.sa_tracks_waste(engine.h, store.h, _keep(keep), ns, _p(scene_ids, u64), _p(counts, u32), ptrs, _p(_capacity(capacity, n), u32),
                                   _p(n_obs, u32)))
    return flat, n_obs[:n]


def waste(engine, store, leaving, keep="latest", capacity=None) -> dict:
    """The tracks {scene: ids} leave the engine's table and their feature banks enter `store` (an unknown id is created, a known one
    joined under `keep`): {id: the observations it brought}."""
    ids, n_obs = waste_raw(engine, store, leaving, keep, capacity)
    return {int(i): int(m) for i, m in zip(ids, n_obs)}


def waste_absorb_raw(engine, store, leaving, topn, max_distance, keep="latest", capacity=None, compat=None, q_attrs=None, min_votes=1,
                     keep_below=math.inf, track=True):
    """-> (ids [n], (out_n [n], winners [n][topn], tracks [n][topn] or None, weights [n][topn], dest [n])) as sa_tracks_waste_absorb
    writes them.  q_attrs: [n] of ATTRS_DTYPE, exactly with a rule."""
    lib = _lib(store)
    ns, scene_ids, counts, ptrs, flat, alive = _scenes(leaving)
    n = len(flat)
    prm = sa_topn_params(int(topn), int(min_votes), float(max_distance), float(keep_below))
    rule = _attrs._rule(compat)
    qa = _attrs._attrs(q_attrs)
    assert qa is None or len(qa) == n, "one sa_track_attrs per id"
    shape = (max(n, 1), max(int(topn), 1))
    out_n = np.zeros(shape[0], np.uint32)
    win = np.zeros(shape, np.uint64)
    trk = np.zeros(shape, np.uint64) if track else None
    wt = np.zeros(shape, np.float64)
    dest = np.zeros(shape[0], np.uint64)
    engine._chk(lib.sa_tracks_waste_absorb(engine.h, store.h, _keep(keep), C.byref(prm), None if rule is None else C.byref(rule), ns,
                                          _p(scene_ids, u64), _p(counts, u32), ptrs, _p(qa, sa_track_attrs), _p(_capacity(capacity, n), u32),
                                          _p(out_n, u32), _p(win, u64), _p(trk, u64), _p(wt, C.c_double), _p(dest, u64)))
    return flat, (out_n[:n], win[:n], None if trk is None else trk[:n], wt[:n], dest[:n])


def waste_absorb(engine, store, leaving, topn, max_distance, keep="latest", capacity=None, compat=None, q_attrs=None, min_votes=1,
                 keep_below=math.inf):
    """The tracks {scene: ids} leave the engine's table and become the queries of one absorb on `store`: what handover.hand_over
    returns — ({id: [(winner id, weight, track id), ...]}, {id: the track of the store that took its rows — a stored one, or itself})."""
    ids, out = waste_absorb_raw(engine, store, leaving, topn, max_distance, keep, capacity, compat, q_attrs, min_votes, keep_below)
    return AbsorbStore._maps(ids, out)


def waste_into(tracker, store, keep="latest", capacity=None):
    """sa_tracker_waste_into: from now on every track that leaves the tracker's engine enters `store` (None detaches)."""
    if store is None:
        tracker._chk(_lib(tracker).sa_tracker_waste_into(tracker.h, None, 0, 0))
        return
    tracker._chk(_lib(store).sa_tracker_waste_into(tracker.h, store.h, _keep(keep), 0 if capacity is None else int(capacity)))


def last(store) -> dict:
    """The fields of sa_waste_stats of the last waste into `store`."""
    st = sa_waste_stats()
    store._chk(_lib(store).sa_store_waste_last(store.h, C.byref(st)))
    return {f: getattr(st, f) for f, _ in sa_waste_stats._fields_}
