"""ctypes mirror of include/similari_search.h (track search: TopN voting over a device-resident feature store) and FeatureStore,
the Python face of it.

FeatureStore.search_topn returns what the reference's `TopNVoting::winners(store.foreign_track_distances(..))` returns: a map query id ->
[(winner id, weight), ...] ranked by weight (descending), then winner id (ascending); a query without a group is absent from the map.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import abi

u32, u64, i32 = C.c_uint32, C.c_uint64, C.c_int32
P = C.POINTER
STORE = C.c_void_p
TOPN_MAX = 64
MAX_OBSERVATIONS = 32


class sa_store_options(C.Structure):
    _fields_ = [("struct_size", u32), ("visual_kind", i32), ("feature_len", u32), ("max_observations", u32)]


class sa_topn_params(C.Structure):
    _fields_ = [("topn", u32), ("min_votes", u32), ("max_distance", C.c_float), ("keep_below", C.c_float)]


class sa_search_stats(C.Structure):
    _fields_ = [("launch1_ms", C.c_double), ("launch2_ms", C.c_double), ("call_ms", C.c_double), ("groups", u32), ("reruns", u32),
                ("pool_bytes", u64)]


# ---- prototypes of every symbol include/similari_search.h declares -------------------------------
PROTOTYPES = {
    "sa_store_options_default": (None, [P(sa_store_options)]),
    "sa_store_create": (C.c_int, [abi.ENGINE, P(sa_store_options), P(STORE)]),
    "sa_store_destroy": (None, [STORE]),
    "sa_store_upsert": (C.c_int, [STORE, u32, P(u64), P(u32), P(C.c_float)]),
    "sa_store_remove": (C.c_int, [STORE, u32, P(u64)]),
    "sa_store_count": (C.c_int, [STORE, P(u32)]),
    "sa_store_order": (C.c_int, [STORE, P(u64), u32, P(u32)]),
    "sa_store_search_topn": (C.c_int, [STORE, P(sa_topn_params), u32, P(u64), P(u32), P(C.c_float), P(u32), P(u64), P(C.c_double),
                                       P(C.c_float)]),
    "sa_store_last_stats": (C.c_int, [STORE, P(sa_search_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach the prototypes of similari_search.h to a library abi.load_library returned."""
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library(path=None) -> C.CDLL:
    return bind(abi.load_library(path))


def _p(a, ctype):
    return C.cast(None, P(ctype)) if a is None else a.ctypes.data_as(P(ctype))


def pack_tracks(ids, feats_per_track, feature_len):
    """ids + per-track observation arrays ([n_obs][D], or None / empty) -> (ids u64, n_obs u32, feats [sum n_obs][D] f32)."""
    ids = np.ascontiguousarray(ids, np.uint64).reshape(-1)
    rows = [np.zeros((0, feature_len), np.float32) if f is None else np.asarray(f, np.float32).reshape(-1, feature_len)
            for f in feats_per_track]
    assert len(rows) == len(ids), "one observation array per id"
    n_obs = np.array([len(r) for r in rows], np.uint32)
    feats = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, feature_len), np.float32), np.float32)
    return ids, n_obs, feats


class FeatureStore:
    """Feature banks of up to `max_observations` (1..32) observations per track, resident on the engine's GPU."""

    def __init__(self, engine, kind: str = "cosine", feature_len: int = 0, max_observations: int = 1):
        self.engine = engine
        self.lib = bind(engine.lib)
        self.kind = kind
        self.D = int(feature_len)
        self.K = int(max_observations)
        o = sa_store_options()
        self.lib.sa_store_options_default(C.byref(o))
        o.visual_kind = {"cosine": abi.SA_VIS_COSINE, "euclidean": abi.SA_VIS_EUCLIDEAN}[kind]
        o.feature_len = self.D
        o.max_observations = self.K
        self.h = STORE()
        self._chk(self._create(o))

    def _create(self, o) -> int:
        """The creation call itself (-> its return code, the handle in self.h): the one step a subclass replaces (bf16.Bf16Store)."""
        return self.lib.sa_store_create(self.engine.h, C.byref(o), C.byref(self.h))

    def _chk(self, rc):
        if rc != abi.SA_OK:
            from .engine import EngineError

            msg = self.lib.sa_last_error(self.engine.h)
            raise EngineError(rc, msg.decode() if msg else "")

    def close(self):
        if self.h:
            self.lib.sa_store_destroy(self.h)
        self.h = STORE()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def upsert(self, ids, feats_per_track):
        """Insert or replace the whole bank of each track."""
        ids, n_obs, feats = pack_tracks(ids, feats_per_track, self.D)
        self._chk(self.lib.sa_store_upsert(self.h, len(ids), _p(ids, C.c_uint64), _p(n_obs, C.c_uint32), _p(feats, C.c_float)))

    def remove(self, ids):
        ids = np.ascontiguousarray(ids, np.uint64).reshape(-1)
        self._chk(self.lib.sa_store_remove(self.h, len(ids), _p(ids, C.c_uint64)))

    def __len__(self):
        n = u32()
        self._chk(self.lib.sa_store_count(self.h, C.byref(n)))
        return n.value

    def order(self) -> np.ndarray:
        """Stored ids in column order (the columns of the cell matrix search_topn(tap=True) returns)."""
        n = len(self)
        out = np.zeros(max(n, 1), np.uint64)
        m = u32()
        self._chk(self.lib.sa_store_order(self.h, _p(out, C.c_uint64), n, C.byref(m)))
        return out[: m.value].copy()

    def _search_call(self, symbol, n, args, topn, max_distance, min_votes, keep_below, tap):
        """One search of n queries through `symbol`: the params, `args`, then the outputs, which come back as the C call writes them:
        (out_n [n], winners [n][topn], weights [n][topn], cells [n][K][count][K] or None)."""
        prm = sa_topn_params(int(topn), int(min_votes), float(max_distance), float(keep_below))
        out_n = np.zeros(max(n, 1), np.uint32)
        win = np.zeros((max(n, 1), max(int(topn), 1)), np.uint64)
        wt = np.zeros((max(n, 1), max(int(topn), 1)), np.float64)
        cells = np.empty((n, self.K, len(self), self.K), np.float32) if tap else None
        self._chk(getattr(self.lib, symbol)(self.h, C.byref(prm), *args, _p(out_n, C.c_uint32), _p(win, C.c_uint64), _p(wt, C.c_double),
                                            _p(cells, C.c_float)))
        return out_n[:n], win[:n], wt[:n], cells

    def _search_raw(self, symbol, lead, trail, query_ids, query_feats, *params):
        """search_raw through `symbol`, whose arguments are `lead`, the queries, `trail` (a *_compat call: the rule, the queries' attributes)."""
        q_ids, q_n_obs, q_feats = pack_tracks(query_ids, query_feats, self.D)
        args = [*lead, len(q_ids), _p(q_ids, C.c_uint64), _p(q_n_obs, C.c_uint32), _p(q_feats, C.c_float), *trail]
        return self._search_call(symbol, len(q_ids), args, *params)

    def search_raw(self, query_ids, query_feats, topn, max_distance, min_votes=1, keep_below=math.inf, tap=False):
        """-> (out_n [Q], winners [Q][topn], weights [Q][topn], cells [Q][K][count][K] or None) as the C call writes them."""
        return self._search_raw("sa_store_search_topn", (), (), query_ids, query_feats, topn, max_distance, min_votes, keep_below, tap)

    def search_topn(self, query_ids, query_feats, topn, max_distance, min_votes=1, keep_below=math.inf, tap=False):
        """{query id: [(winner id, weight), ...]} (and the cell matrix when tap=True)."""
        out_n, win, wt, cells = self.search_raw(query_ids, query_feats, topn, max_distance, min_votes, keep_below, tap)
        q_ids = np.asarray(query_ids, np.uint64).reshape(-1)
        res = {int(q): [(int(win[i, r]), float(wt[i, r])) for r in range(int(out_n[i]))] for i, q in enumerate(q_ids) if out_n[i]}
        return (res, cells) if tap else res

    def last_stats(self) -> dict:
        st = sa_search_stats()
        self._chk(self.lib.sa_store_last_stats(self.h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in sa_search_stats._fields_}
