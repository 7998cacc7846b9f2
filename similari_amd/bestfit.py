"""ctypes mirror of include/similari_bestfit.h (track search under the BestFit vote: one claimant per stored track) and
BestFitStore, the Python face of it.

BestFitStore.search_bestfit returns what the reference's `BestFitVoting::winners(store.foreign_track_distances(..))` returns
(src/track/voting/best.rs:52-128), each query's list cut at `topn`: a map query id -> [(winner id, weight, track id), ...] in the
order of the call's one ranked list.  `track id` is the stored track the entry's group names; `winner id` is that track if the group
holds the claim on it, else the query's own id.  A stored id is a winner at most once in a call.

    top = {q: lst[0][0] for q, lst in store.join_bestfit(1, max_distance).items()}   # every stored track against every other one
    store.merge({q: [w] for q, w in top.items() if q < w and top.get(w) == q})       # mutual pairs: conflict-free as they come
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import attrs as _attrs
from .attrs import AttrStore, sa_compat, sa_track_attrs
from .gallery import SA_STORED_WITHDRAW
from .search import STORE, _p, pack_tracks, sa_topn_params

u32, u64 = C.c_uint32, C.c_uint64
P = C.POINTER


class sa_bestfit_stats(C.Structure):
    _fields_ = [("weigh_ms", C.c_double), ("claim_ms", C.c_double), ("rank_ms", C.c_double), ("groups", u32), ("claimed", u32)]


# ---- prototypes of every symbol include/similari_bestfit.h declares ------------------------------
_OUT = [P(u32), P(u64), P(u64), P(C.c_double), P(C.c_float)]
PROTOTYPES = {
    "sa_store_search_bestfit": (C.c_int, [STORE, P(sa_topn_params), P(sa_compat), u32, P(u64), P(u32), P(C.c_float), P(sa_track_attrs)] + _OUT),
    "sa_store_search_stored_bestfit": (C.c_int, [STORE, P(sa_topn_params), P(sa_compat), u32, u32, P(u64)] + _OUT),
    "sa_store_join_bestfit": (C.c_int, [STORE, P(sa_topn_params), P(sa_compat)] + _OUT),
    "sa_store_bestfit_last": (C.c_int, [STORE, P(sa_bestfit_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach the prototypes of similari_search.h .. similari_bestfit.h to a library abi.load_library returned."""
    _attrs.bind(lib)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library(path=None) -> C.CDLL:
    from . import abi

    return bind(abi.load_library(path))


def _result(ids, out_n, win, trk, wt):
    return {int(q): [(int(win[i, r]), float(wt[i, r]), int(trk[i, r])) for r in range(int(out_n[i]))] for i, q in enumerate(ids) if out_n[i]}


class BestFitStore(AttrStore):
    """An AttrStore whose three searches can also vote BestFit: every surviving group of a call in one ranked list, a stored track
    claimed by the first group that names it."""

    def __init__(self, engine, kind: str = "cosine", feature_len: int = 0, max_observations: int = 1):
        super().__init__(engine, kind, feature_len, max_observations)
        bind(self.lib)

    def _fit_call(self, symbol, n, compat, args, topn, max_distance, min_votes, keep_below, tap, track=True):
        """One BestFit search of n queries through `symbol`: the params, the rule (None: a null pointer, the plain path), `args`, then
        the outputs as the C call writes them: (out_n [n], winners [n][topn], tracks [n][topn] or None, weights [n][topn], cells or None)."""
        prm = sa_topn_params(int(topn), int(min_votes), float(max_distance), float(keep_below))
        rule = _attrs._rule(compat)
        rows, cols = max(n, 1), max(int(topn), 1)
        out_n = np.zeros(rows, np.uint32)
        win = np.zeros((rows, cols), np.uint64)
        trk = np.zeros((rows, cols), np.uint64) if track else None
        wt = np.zeros((rows, cols), np.float64)
        cells = np.empty((n, self.K, len(self), self.K), np.float32) if tap else None
        self._chk(getattr(self.lib, symbol)(self.h, C.byref(prm), None if rule is None else C.byref(rule), *args, _p(out_n, u32), _p(win, u64),
                                            _p(trk, u64), _p(wt, C.c_double), _p(cells, C.c_float)))
        return out_n[:n], win[:n], None if trk is None else trk[:n], wt[:n], cells

    # ---- host-fed queries ----
    def search_bestfit_raw(self, query_ids, query_feats, topn, max_distance, min_votes=1, keep_below=math.inf, tap=False, compat=None,
                           q_attrs=None, track=True):
        """-> (out_n [Q], winners [Q][topn], tracks [Q][topn] or None, weights [Q][topn], cells [Q][K][count][K] or None).  compat: a
        Compat, an sa_compat or None; q_attrs: one sa_track_attrs per query, given exactly when compat is."""
        q_ids, q_n_obs, q_feats = pack_tracks(query_ids, query_feats, self.D)
        qa = _attrs._attrs(q_attrs)
        assert qa is None or len(qa) == len(q_ids), "one sa_track_attrs per query"
        args = [len(q_ids), _p(q_ids, u64), _p(q_n_obs, u32), _p(q_feats, C.c_float), _p(qa, sa_track_attrs)]
        return self._fit_call("sa_store_search_bestfit", len(q_ids), compat, args, topn, max_distance, min_votes, keep_below, tap, track)

    def search_bestfit(self, query_ids, query_feats, topn, max_distance, min_votes=1, keep_below=math.inf, tap=False, compat=None, q_attrs=None):
        """{query id: [(winner id, weight, track id), ...]} (and the cell matrix when tap=True)."""
        out_n, win, trk, wt, cells = self.search_bestfit_raw(query_ids, query_feats, topn, max_distance, min_votes, keep_below, tap, compat, q_attrs)
        res = _result(np.asarray(query_ids, np.uint64).reshape(-1), out_n, win, trk, wt)
        return (res, cells) if tap else res

    # ---- stored queries ----
    def search_stored_bestfit_raw(self, ids, topn, max_distance, min_votes=1, keep_below=math.inf, withdraw=False, tap=False, flags=None,
                                  compat=None, track=True):
        """flags: the raw flag word (default: SA_STORED_WITHDRAW when withdraw)."""
        ids = np.ascontiguousarray(ids, np.uint64).reshape(-1)
        fl = (SA_STORED_WITHDRAW if withdraw else 0) if flags is None else int(flags)
        return self._fit_call("sa_store_search_stored_bestfit", len(ids), compat, [fl, len(ids), _p(ids, u64)], topn, max_distance, min_votes,
                              keep_below, tap, track)

    def search_stored_bestfit(self, ids, topn, max_distance, min_votes=1, keep_below=math.inf, withdraw=False, tap=False, compat=None):
        """{queried id: [(winner id, weight, track id), ...]}.  withdraw: the queried tracks are out of the store for the call, so none
        of them can be claimed."""
        out_n, win, trk, wt, cells = self.search_stored_bestfit_raw(ids, topn, max_distance, min_votes, keep_below, withdraw, tap, compat=compat)
        res = _result(np.asarray(ids, np.uint64).reshape(-1), out_n, win, trk, wt)
        return (res, cells) if tap else res

    # ---- the join ----
    def join_bestfit_raw(self, topn, max_distance, min_votes=1, keep_below=math.inf, tap=False, compat=None, track=True):
        """Every stored track as a query, rows in order() order."""
        return self._fit_call("sa_store_join_bestfit", len(self), compat, [], topn, max_distance, min_votes, keep_below, tap, track)

    def join_bestfit(self, topn, max_distance, min_votes=1, keep_below=math.inf, tap=False, compat=None):
        """{stored id: [(winner id, weight, track id), ...]} over the whole store."""
        ids = self.order()
        out_n, win, trk, wt, cells = self.join_bestfit_raw(topn, max_distance, min_votes, keep_below, tap, compat)
        res = _result(ids, out_n, win, trk, wt)
        return (res, cells) if tap else res

    def bestfit_stats(self) -> dict:
        st = sa_bestfit_stats()
        self._chk(self.lib.sa_store_bestfit_last(self.h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in sa_bestfit_stats._fields_}
