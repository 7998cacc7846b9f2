"""ctypes mirror of include/similari_consolidate.h (a store's mutual best pairs merged in one call on the device) and the functions
that are the Python face of it.  They work on any store object of the chain (FeatureStore .. I8Store).

The pass inside one store — tracklets of one identity merged, a gallery de-duplicated — in one call instead of a join, Python between
and a merge (the idiom similari_amd/bestfit.py shows):

    winners, merged = consolidate.consolidate(store, topn=1, max_distance=0.3, keep="best")   # merged: {source id: destination id}
    consolidate.last(store)                                                                    # pairs, launches, host_waits, ..
    merged = consolidate.consolidate_all(store, topn=1, max_distance=0.3)                      # until a call merges no pair

One call merges pairs, not clusters: four tracklets of one identity take two calls.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import attrs as _attrs
from . import handover as _handover
from .attrs import sa_compat
from .bestfit import _result
from .merge import _keep
from .search import STORE, _p, sa_topn_params

u32, u64 = C.c_uint32, C.c_uint64
P = C.POINTER


class sa_consolidate_stats(C.Structure):
    _fields_ = [("step_ms", C.c_double), ("compact_ms", C.c_double), ("pairs", u32), ("rows_moved", u32), ("tracks_moved", u32),
                ("launches", u32), ("host_waits", u32), ("keep", u32), ("qual_upload_bytes", u64)]


# ---- prototypes of every symbol include/similari_consolidate.h declares --------------------------
PROTOTYPES = {
    "sa_store_consolidate": (C.c_int, [STORE, u32, P(sa_topn_params), P(sa_compat), u32, P(u32), P(u64), P(u64), P(C.c_double), P(u64), P(u64)]),
    "sa_store_consolidate_last": (C.c_int, [STORE, P(sa_consolidate_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach the prototypes of similari_search.h .. similari_consolidate.h to a library abi.load_library returned."""
    _handover.bind(lib)
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
    if not getattr(lib, "_sa_consolidate_bound", False):
        bind(lib)
        lib._sa_consolidate_bound = True
    return lib


def consolidate_raw(store, topn, max_distance, keep="latest", capacity=None, compat=None, min_votes=1, keep_below=math.inf, track=True):
    """-> (out_n [T], winners [T][topn], tracks [T][topn] or None, weights [T][topn], ids [T], dest [T]) as sa_store_consolidate writes
    them, T the store's count before the call.  capacity: None (the store's K) or one int for every destination."""
    lib = _lib(store)
    n = len(store)
    prm = sa_topn_params(int(topn), int(min_votes), float(max_distance), float(keep_below))
    rule = _attrs._rule(compat)
    shape = (max(n, 1), max(int(topn), 1))
    out_n = np.zeros(shape[0], np.uint32)
    win = np.zeros(shape, np.uint64)
    trk = np.zeros(shape, np.uint64) if track else None
    wt = np.zeros(shape, np.float64)
    ids = np.zeros(shape[0], np.uint64)
    dest = np.zeros(shape[0], np.uint64)
    store._chk(lib.sa_store_consolidate(store.h, _keep(keep), C.byref(prm), None if rule is None else C.byref(rule),
                                        0 if capacity is None else int(capacity), _p(out_n, u32), _p(win, u64), _p(trk, u64),
                                        _p(wt, C.c_double), _p(ids, u64), _p(dest, u64)))
    return out_n[:n], win[:n], None if trk is None else trk[:n], wt[:n], ids[:n], dest[:n]


def consolidate(store, topn, max_distance, keep="latest", capacity=None, compat=None, min_votes=1, keep_below=math.inf):
    """Every mutual best pair of the store merges into its lower id: ({track: [(winner id, weight, track id), ...]} as
    BestFitStore.join_bestfit returns it, {source id: destination id} for the tracks that left)."""
    out_n, win, trk, wt, ids, dest = consolidate_raw(store, topn, max_distance, keep, capacity, compat, min_votes, keep_below)
    return _result(ids, out_n, win, trk, wt), {int(i): int(d) for i, d in zip(ids, dest) if i != d}


def consolidate_all(store, topn, max_distance, keep="latest", capacity=None, compat=None, min_votes=1, keep_below=math.inf, max_rounds=8):
    """consolidate until a call merges no pair (at most max_rounds calls): {source id: the track that holds its rows in the end}."""
    final = {}
    for _ in range(int(max_rounds)):
        merged = consolidate(store, topn, max_distance, keep, capacity, compat, min_votes, keep_below)[1]
        if not merged:
            break
        for src, dst in final.items():   # a destination of an earlier round may have left in this one
            final[src] = merged.get(dst, dst)
        final.update(merged)
    return final


def last(store) -> dict:
    """The fields of sa_consolidate_stats of the store's last consolidate."""
    st = sa_consolidate_stats()
    store._chk(_lib(store).sa_store_consolidate_last(store.h, C.byref(st)))
    return {f: getattr(st, f) for f, _ in sa_consolidate_stats._fields_}
