"""ctypes mirror of include/similari_gallery.h (track search whose queries are stored tracks) and Gallery, the Python face of it.

Gallery.search_stored(ids, withdraw=True) returns what the reference's `TopNVoting::winners(store.owned_track_distances(ids, ..))`
returns; Gallery.join_topn what the loop of examples/track_merging.rs returns when it is run over every track of a store.  Both are
maps query id -> [(winner id, weight), ...] as FeatureStore.search_topn gives them.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import search
from .search import STORE, FeatureStore, _p, sa_topn_params

u32, u64 = C.c_uint32, C.c_uint64
P = C.POINTER
SA_STORED_WITHDRAW = 1


class sa_join_stats(C.Structure):
    _fields_ = [("tiles", u64), ("tiles_rect", u64), ("blocks", u32), ("reserved", u32)]


# ---- prototypes of every symbol include/similari_gallery.h declares ------------------------------
PROTOTYPES = {
    "sa_store_search_stored": (C.c_int, [STORE, P(sa_topn_params), u32, u32, P(u64), P(u32), P(u64), P(C.c_double), P(C.c_float)]),
    "sa_store_join_topn": (C.c_int, [STORE, P(sa_topn_params), P(u32), P(u64), P(C.c_double), P(C.c_float)]),
    "sa_store_join_last": (C.c_int, [STORE, P(sa_join_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach the prototypes of similari_search.h and similari_gallery.h to a library abi.load_library returned."""
    search.bind(lib)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library(path=None) -> C.CDLL:
    from . import abi

    return bind(abi.load_library(path))


def _result(ids, out_n, win, wt):
    return {int(q): [(int(win[i, r]), float(wt[i, r])) for r in range(int(out_n[i]))] for i, q in enumerate(ids) if out_n[i]}


class Gallery(FeatureStore):
    """A FeatureStore that can be searched with its own tracks, and joined with itself, without a host copy of any bank."""

    def __init__(self, engine, kind: str = "cosine", feature_len: int = 0, max_observations: int = 1):
        super().__init__(engine, kind, feature_len, max_observations)
        bind(self.lib)

    def _search_stored_raw(self, symbol, lead, ids, topn, max_distance, min_votes, keep_below, withdraw, tap, flags):
        """search_stored_raw through `symbol`, whose arguments begin with `lead` (a *_compat call: the rule)."""
        ids = np.ascontiguousarray(ids, np.uint64).reshape(-1)
        fl = (SA_STORED_WITHDRAW if withdraw else 0) if flags is None else int(flags)
        return self._search_call(symbol, len(ids), [*lead, fl, len(ids), _p(ids, u64)], topn, max_distance, min_votes, keep_below, tap)

    def search_stored_raw(self, ids, topn, max_distance, min_votes=1, keep_below=math.inf, withdraw=False, tap=False, flags=None):
        """-> (out_n [n], winners [n][topn], weights [n][topn], cells [n][K][count][K] or None) as the C call writes them.
        flags: the raw flag word (default: SA_STORED_WITHDRAW when withdraw)."""
        return self._search_stored_raw("sa_store_search_stored", (), ids, topn, max_distance, min_votes, keep_below, withdraw, tap, flags)

    def search_stored(self, ids, topn, max_distance, min_votes=1, keep_below=math.inf, withdraw=False, tap=False):
        """{queried id: [(winner id, weight), ...]} (and the cell matrix when tap=True).  withdraw: the queried tracks are out of
        the store for the call, as in TrackStore::owned_track_distances."""
        out_n, win, wt, cells = self.search_stored_raw(ids, topn, max_distance, min_votes, keep_below, withdraw, tap)
        res = _result(np.asarray(ids, np.uint64).reshape(-1), out_n, win, wt)
        return (res, cells) if tap else res

    def join_raw(self, topn, max_distance, min_votes=1, keep_below=math.inf, tap=False):
        """Every stored track as a query, rows in order() order -> (out_n [T], winners [T][topn], weights [T][topn], cells or None)."""
        return self._search_call("sa_store_join_topn", len(self), (), topn, max_distance, min_votes, keep_below, tap)

    def join_topn(self, topn, max_distance, min_votes=1, keep_below=math.inf, tap=False):
        """{stored id: [(winner id, weight), ...]} over the whole store (and the cell matrix [T][K][T][K] when tap=True)."""
        ids = self.order()
        out_n, win, wt, cells = self.join_raw(topn, max_distance, min_votes, keep_below, tap)
        res = _result(ids, out_n, win, wt)
        return (res, cells) if tap else res

    def join_stats(self) -> dict:
        st = sa_join_stats()
        self._chk(self.lib.sa_store_join_last(self.h, C.byref(st)))
        return {"tiles": st.tiles, "tiles_rect": st.tiles_rect, "blocks": st.blocks}
