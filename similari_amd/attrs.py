"""ctypes mirror of include/similari_attrs.h (track attributes and the compatibility rule of a track search) and AttrStore, the
Python face of it.

AttrStore.search_topn(.., compat=, q_attrs=) returns what the reference returns when `Track::distances` refuses incompatible pairs
(src/track.rs:609) and the store drops them (src/track/store.rs:217-219); `compat` is built by `attrs.compat(..)`:

    rule = attrs.compat(same_key=True, disjoint=True)          # examples/track_merging.rs:222-225
    rule = attrs.compat(query_first=True, ready_at=now)        # store_tests.rs:44-46 with only_baked

Without `compat` every method is the one of MergeStore.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import numpy as np

from . import merge as _merge
from .gallery import _result
from .merge import MergeStore, _keep
from .search import STORE, _p, sa_topn_params

u8, u32, u64, i64 = C.c_uint8, C.c_uint32, C.c_uint64, C.c_int64
P = C.POINTER
SA_COMPAT_SAME_KEY, SA_COMPAT_DISJOINT, SA_COMPAT_QUERY_FIRST, SA_COMPAT_ONLY_READY = 1, 2, 4, 8
INT64_MAX = 2**63 - 1
ATTRS_DTYPE = np.dtype([("key", np.uint64), ("start", np.int64), ("end", np.int64)])


class sa_track_attrs(C.Structure):
    _fields_ = [("key", u64), ("start", i64), ("end", i64)]


class sa_compat(C.Structure):
    _fields_ = [("struct_size", u32), ("flags", u32), ("ready_at", i64)]


class sa_compat_stats(C.Structure):
    _fields_ = [("tiles", u64), ("tiles_skipped", u64)]


# ---- prototypes of every symbol include/similari_attrs.h declares --------------------------------
_OUT = [P(u32), P(u64), P(C.c_double), P(C.c_float)]
PROTOTYPES = {
    "sa_compat_default": (None, [P(sa_compat)]),
    "sa_store_set_attrs": (C.c_int, [STORE, u32, P(u64), P(sa_track_attrs)]),
    "sa_store_get_attrs": (C.c_int, [STORE, u32, P(u64), P(sa_track_attrs), P(u8)]),
    "sa_store_search_topn_compat": (C.c_int, [STORE, P(sa_topn_params), P(sa_compat), u32, P(u64), P(u32), P(C.c_float),
                                              P(sa_track_attrs)] + _OUT),
    "sa_store_search_stored_compat": (C.c_int, [STORE, P(sa_topn_params), P(sa_compat), u32, u32, P(u64)] + _OUT),
    "sa_store_join_topn_compat": (C.c_int, [STORE, P(sa_topn_params), P(sa_compat)] + _OUT),
    "sa_store_merge_compat": (C.c_int, [STORE, P(sa_compat), u32, u32, P(u64), P(u32), P(u64), P(u32)]),
    "sa_store_compat_last": (C.c_int, [STORE, P(sa_compat_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach the prototypes of similari_search.h .. similari_attrs.h to a library abi.load_library returned."""
    _merge.bind(lib)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library(path=None) -> C.CDLL:
    from . import abi

    return bind(abi.load_library(path))


class Compat(NamedTuple):
    """The rule of a call: the flag word and ready_at (SA_COMPAT_ONLY_READY is set when ready_at is given)."""
    flags: int = 0
    ready_at: int = INT64_MAX

    def struct(self) -> sa_compat:
        return sa_compat(C.sizeof(sa_compat), int(self.flags), int(self.ready_at))


def compat(same_key=False, disjoint=False, query_first=False, ready_at: Optional[int] = None) -> Compat:
    flags = (SA_COMPAT_SAME_KEY if same_key else 0) | (SA_COMPAT_DISJOINT if disjoint else 0) | (SA_COMPAT_QUERY_FIRST if query_first else 0)
    if ready_at is not None:
        flags |= SA_COMPAT_ONLY_READY
    return Compat(flags, INT64_MAX if ready_at is None else int(ready_at))


def pack_attrs(keys, starts, ends) -> np.ndarray:
    """Three columns -> the array of sa_track_attrs (ATTRS_DTYPE) the C calls read."""
    keys = np.asarray(keys, np.uint64).reshape(-1)
    out = np.zeros(len(keys), ATTRS_DTYPE)
    out["key"], out["start"], out["end"] = keys, np.asarray(starts, np.int64).reshape(-1), np.asarray(ends, np.int64).reshape(-1)
    return out


def _attrs(a):
    return None if a is None else np.ascontiguousarray(a, ATTRS_DTYPE).reshape(-1)


def _rule(c):
    return None if c is None else (c if isinstance(c, sa_compat) else c.struct())


class AttrStore(MergeStore):
    """A MergeStore whose tracks carry (key, start, end) and whose searches, join and merge can run under a compatibility rule."""

    def __init__(self, engine, kind: str = "cosine", feature_len: int = 0, max_observations: int = 1):
        super().__init__(engine, kind, feature_len, max_observations)
        bind(self.lib)

    # ---- the table ----
    def set_attrs_raw(self, ids, attrs):
        ids = np.ascontiguousarray(ids, np.uint64).reshape(-1)
        a = _attrs(attrs)
        assert a is None or len(a) == len(ids), "one sa_track_attrs per id"
        self._chk(self.lib.sa_store_set_attrs(self.h, len(ids), _p(ids, u64), _p(a, sa_track_attrs)))

    def set_attrs(self, ids, keys, starts, ends):
        self.set_attrs_raw(ids, pack_attrs(keys, starts, ends))

    def get_attrs_raw(self, ids):
        """-> (attrs [n] of ATTRS_DTYPE, known [n] bool)"""
        ids = np.ascontiguousarray(ids, np.uint64).reshape(-1)
        out = np.zeros(max(len(ids), 1), ATTRS_DTYPE)
        known = np.zeros(max(len(ids), 1), np.uint8)
        self._chk(self.lib.sa_store_get_attrs(self.h, len(ids), _p(ids, u64), _p(out, sa_track_attrs), _p(known, u8)))
        return out[: len(ids)], known[: len(ids)].astype(bool)

    def get_attrs(self, ids):
        """{id: (key, start, end)} of the ids the store holds."""
        out, known = self.get_attrs_raw(ids)
        return {int(i): (int(a["key"]), int(a["start"]), int(a["end"])) for i, a, k in zip(np.asarray(ids).reshape(-1), out, known) if k}

    # ---- searches ----
    def search_raw(self, query_ids, query_feats, topn, max_distance, min_votes=1, keep_below=math.inf, tap=False, compat=None, q_attrs=None):
        if compat is None:
            return super().search_raw(query_ids, query_feats, topn, max_distance, min_votes, keep_below, tap)
        qa = _attrs(q_attrs)
        assert qa is None or len(qa) == np.size(query_ids), "one sa_track_attrs per query"
        rule = _rule(compat)
        return self._search_raw("sa_store_search_topn_compat", [C.byref(rule)], [_p(qa, sa_track_attrs)], query_ids, query_feats, topn,
                                max_distance, min_votes, keep_below, tap)

    def search_topn(self, query_ids, query_feats, topn, max_distance, min_votes=1, keep_below=math.inf, tap=False, compat=None, q_attrs=None):
        out_n, win, wt, cells = self.search_raw(query_ids, query_feats, topn, max_distance, min_votes, keep_below, tap, compat, q_attrs)
        res = _result(np.asarray(query_ids, np.uint64).reshape(-1), out_n, win, wt)
        return (res, cells) if tap else res

    def search_stored_raw(self, ids, topn, max_distance, min_votes=1, keep_below=math.inf, withdraw=False, tap=False, flags=None, compat=None):
        if compat is None:
            return super().search_stored_raw(ids, topn, max_distance, min_votes, keep_below, withdraw, tap, flags)
        rule = _rule(compat)
        return self._search_stored_raw("sa_store_search_stored_compat", [C.byref(rule)], ids, topn, max_distance, min_votes, keep_below,
                                       withdraw, tap, flags)

    def search_stored(self, ids, topn, max_distance, min_votes=1, keep_below=math.inf, withdraw=False, tap=False, compat=None):
        out_n, win, wt, cells = self.search_stored_raw(ids, topn, max_distance, min_votes, keep_below, withdraw, tap, compat=compat)
        res = _result(np.asarray(ids, np.uint64).reshape(-1), out_n, win, wt)
        return (res, cells) if tap else res

    def join_raw(self, topn, max_distance, min_votes=1, keep_below=math.inf, tap=False, compat=None):
        if compat is None:
            return super().join_raw(topn, max_distance, min_votes, keep_below, tap)
        rule = _rule(compat)
        return self._search_call("sa_store_join_topn_compat", len(self), [C.byref(rule)], topn, max_distance, min_votes, keep_below, tap)

    def join_topn(self, topn, max_distance, min_votes=1, keep_below=math.inf, tap=False, compat=None):
        ids = self.order()
        out_n, win, wt, cells = self.join_raw(topn, max_distance, min_votes, keep_below, tap, compat)
        res = _result(ids, out_n, win, wt)
        return (res, cells) if tap else res

    # ---- merge ----
    def merge_raw(self, rule, keep, dst, n_src, src, capacity=None):
        """sa_store_merge_compat on arrays; rule: a Compat, an sa_compat, or None (a null pointer: refused)."""
        dst = np.ascontiguousarray(dst, np.uint64).reshape(-1)
        n_src = np.ascontiguousarray(n_src, np.uint32).reshape(-1)
        src = np.ascontiguousarray(src, np.uint64).reshape(-1)
        r = _rule(rule)
        self._chk(self.lib.sa_store_merge_compat(self.h, None if r is None else C.byref(r), _keep(keep), len(dst), _p(dst, u64),
                                                 _p(n_src, u32), _p(src, u64), _p(capacity, u32)))

    def merge(self, pairs, keep="latest", capacity=None, compat=None):
        """MergeStore.merge; with `compat` the attributes merge too: every source must be live against its destination as merged so
        far (a rule without bits tests nothing), the destination then spans both.  An incompatible source refuses the whole call."""
        if compat is None:
            return super().merge(pairs, keep, capacity)
        dst = np.array([int(d) for d in pairs], np.uint64)
        n_src = np.array([len(v) for v in pairs.values()], np.uint32)
        src = np.array([int(x) for v in pairs.values() for x in v], np.uint64)
        self.merge_raw(compat, keep, dst, n_src, src, self._capacity(capacity, dst))

    def compat_stats(self) -> dict:
        st = sa_compat_stats()
        self._chk(self.lib.sa_store_compat_last(self.h, C.byref(st)))
        return {"tiles": st.tiles, "tiles_skipped": st.tiles_skipped}
