"""ctypes mirror of include/similari_handover.h (ready tracks handed from one feature store to another on the device) and the four
functions that are the Python face of it.  They work on any store object of the chain (FeatureStore .. I8Store).

The reference's flagship pipeline is two stores (examples/track_merging.rs:371-481): tracks grow in a temporary store, and the ready
ones leave it for the gallery, where each either joins its BestFit winner or becomes a track of its own.

    baked = handover.ready(temp, now)                                      # find_usable
    winners, dest = handover.hand_over(temp, gallery, baked, topn=1, max_distance=0.3, keep="best")
    handover.last(gallery)                                                 # launches, rows; no feature byte crossed the bus

    tracks = handover.take(temp, ids)                                      # fetch_tracks: {id: (rows, quality, attrs)}, the ids are gone
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import attrs as _attrs
from . import i8 as _i8
from .absorb import AbsorbStore
from .attrs import ATTRS_DTYPE, sa_compat, sa_track_attrs
from .merge import _keep
from .search import STORE, _p, sa_topn_params

u32, u64, i64 = C.c_uint32, C.c_uint64, C.c_int64
P = C.POINTER


class sa_handover_stats(C.Structure):
    _fields_ = [("struct_size", u32), ("launches_fill", u32), ("launches_compact", u32), ("tracks_moved", u32), ("rows", u64),
                ("feature_bytes_h2d", u64), ("feature_bytes_d2h", u64), ("fill_ms", C.c_double), ("compact_ms", C.c_double)]


# ---- prototypes of every symbol include/similari_handover.h declares -----------------------------
PROTOTYPES = {
    "sa_store_ready": (C.c_int, [STORE, i64, P(u64), u32, P(u32)]),
    "sa_store_take": (C.c_int, [STORE, u32, P(u64), P(u32), P(C.c_float), P(C.c_float), P(sa_track_attrs)]),
    "sa_store_hand_over": (C.c_int, [STORE, STORE, u32, P(sa_topn_params), P(sa_compat), u32, P(u64), P(u32), P(u32), P(u64), P(u64),
                                     P(C.c_double), P(u64)]),
    "sa_store_handover_last": (C.c_int, [STORE, P(sa_handover_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach the prototypes of similari_search.h .. similari_handover.h to a library abi.load_library returned."""
    _i8.bind(lib)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library(path=None) -> C.CDLL:
    from . import abi

    return bind(abi.load_library(path))


def _lib(store) -> C.CDLL:
    """The store's library with this header's prototypes attached (once per library)."""
    lib = store.lib
    if not getattr(lib, "_sa_handover_bound", False):
        bind(lib)
        lib._sa_handover_bound = True
    return lib


def _ids(ids) -> np.ndarray:
    return np.ascontiguousarray(ids, np.uint64).reshape(-1)


def ready(store, ready_at) -> list:
    """find_usable: the ids whose stored attributes end at or before `ready_at`, in store order."""
    lib = _lib(store)
    n = u32()
    store._chk(lib.sa_store_ready(store.h, int(ready_at), None, 0, C.byref(n)))
    out = np.zeros(max(n.value, 1), np.uint64)
    store._chk(lib.sa_store_ready(store.h, int(ready_at), _p(out, u64), n.value, C.byref(n)))
    return [int(i) for i in out[: n.value]]


def take_raw(store, ids):
    """-> (n_obs [n], feats [n][K][D], quality [n][K], attrs [n] of ATTRS_DTYPE) as sa_store_take writes them; the ids have left."""
    lib = _lib(store)
    ids = _ids(ids)
    n = len(ids)
    n_obs = np.zeros(max(n, 1), np.uint32)
    feats = np.zeros((max(n, 1), store.K, store.D), np.float32)
    qual = np.zeros((max(n, 1), store.K), np.float32)
    attrs = np.zeros(max(n, 1), ATTRS_DTYPE)
    store._chk(lib.sa_store_take(store.h, n, _p(ids, u64), _p(n_obs, u32), _p(feats, C.c_float), _p(qual, C.c_float),
                                 _p(attrs, sa_track_attrs)))
    return n_obs[:n], feats[:n], qual[:n], attrs[:n]


def take(store, ids) -> dict:
    """fetch_tracks: {id: (rows [n_obs][D], quality [n_obs], (key, start, end))}; the ids have left the store (an id it does not hold
    has no observations and attributes (0, 0, 0))."""
    n_obs, feats, qual, attrs = take_raw(store, ids)
    return {int(i): (feats[k, : n_obs[k]].copy(), qual[k, : n_obs[k]].copy(), (int(attrs[k]["key"]), int(attrs[k]["start"]), int(attrs[k]["end"])))
            for k, i in enumerate(_ids(ids))}


def hand_over_raw(src, dst, ids, topn, max_distance, keep="latest", capacity=None, compat=None, min_votes=1, keep_below=math.inf, track=True):
    """-> (out_n [n], winners [n][topn], tracks [n][topn] or None, weights [n][topn], dest [n]) as sa_store_hand_over writes them.
    capacity: None (dst's K), one int, or one per id."""
    lib = _lib(dst)
    ids = _ids(ids)
    n = len(ids)
    prm = sa_topn_params(int(topn), int(min_votes), float(max_distance), float(keep_below))
    rule = _attrs._rule(compat)
    if capacity is None:
        cap = None
    elif np.ndim(capacity) == 0:
        cap = np.full(n, int(capacity), np.uint32)
    else:
        cap = np.ascontiguousarray(capacity, np.uint32).reshape(-1)
        assert len(cap) == n, "one capacity per id"
    shape = (max(n, 1), max(int(topn), 1))
    out_n = np.zeros(shape[0], np.uint32)
    win = np.zeros(shape, np.uint64)
    trk = np.zeros(shape, np.uint64) if track else None
    wt = np.zeros(shape, np.float64)
    dest = np.zeros(shape[0], np.uint64)
    dst._chk(lib.sa_store_hand_over(src.h, dst.h, _keep(keep), C.byref(prm), None if rule is None else C.byref(rule), n, _p(ids, u64),
                                    _p(cap, u32), _p(out_n, u32), _p(win, u64), _p(trk, u64), _p(wt, C.c_double), _p(dest, u64)))
    return out_n[:n], win[:n], None if trk is None else trk[:n], wt[:n], dest[:n]


def hand_over(src, dst, ids, topn, max_distance, keep="latest", capacity=None, compat=None, min_votes=1, keep_below=math.inf):
    """The tracks `ids` of src become the queries of one absorb on dst and leave src: ({id: [(winner id, weight, track id), ...]},
    {id: the track of dst that took its rows — a stored one, or itself}), as AbsorbStore.absorb returns them."""
    return AbsorbStore._maps(ids, hand_over_raw(src, dst, ids, topn, max_distance, keep, capacity, compat, min_votes, keep_below))


def last(dst) -> dict:
    """The fields of sa_handover_stats of the last hand-over into dst (or of the last take / remove on it)."""
    st = sa_handover_stats()
    dst._chk(_lib(dst).sa_store_handover_last(dst.h, C.byref(st)))
    return {f: getattr(st, f) for f, _ in sa_handover_stats._fields_}
