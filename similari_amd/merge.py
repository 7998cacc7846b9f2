"""ctypes mirror of include/similari_merge.h (bank upkeep on the device: append, merge, fetch) and MergeStore, the Python face of it.

MergeStore.append is the reference's `TrackStore::add` for many tracks at once, MergeStore.merge its `fetch_tracks(src)` +
`merge_external(dst, &src)`, MergeStore.fetch its `fetch_tracks` as a read.  Features stay on the device: a merge sends ids only.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import gallery
from .gallery import Gallery
from .search import STORE, _p, pack_tracks

u32, u64 = C.c_uint32, C.c_uint64
P = C.POINTER
SA_KEEP_LATEST, SA_KEEP_BEST = 0, 1
KEEP = {"latest": SA_KEEP_LATEST, "best": SA_KEEP_BEST}


class sa_merge_stats(C.Structure):
    _fields_ = [("device_ms", C.c_double), ("bytes_moved", u64), ("rows_rewritten", u64), ("tracks_moved", u32), ("launches", u32)]


# ---- prototypes of every symbol include/similari_merge.h declares --------------------------------
PROTOTYPES = {
    "sa_store_append": (C.c_int, [STORE, u32, u32, P(u64), P(u32), P(C.c_float), P(C.c_float), P(u32)]),
    "sa_store_merge": (C.c_int, [STORE, u32, u32, P(u64), P(u32), P(u64), P(u32)]),
    "sa_store_fetch": (C.c_int, [STORE, u32, P(u64), P(u32), P(C.c_float), P(C.c_float)]),
    "sa_store_merge_last": (C.c_int, [STORE, P(sa_merge_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach the prototypes of similari_search.h, similari_gallery.h and similari_merge.h to a library abi.load_library returned."""
    gallery.bind(lib)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library(path=None) -> C.CDLL:
    from . import abi

    return bind(abi.load_library(path))


def _keep(keep) -> int:
    return KEEP[keep] if isinstance(keep, str) else int(keep)   # an int goes through as it is (the library refuses unknown ones)


class MergeStore(Gallery):
    """A Gallery whose banks grow, merge and can be read back where they lie.  Every observation carries a quality (0 for rows an
    upsert wrote); `keep` names what a bank retains beyond its capacity: "latest" (the last C) or "best" (the C of highest quality,
    earlier first among equals — the bank then lies in that order)."""

    def __init__(self, engine, kind: str = "cosine", feature_len: int = 0, max_observations: int = 1):
        super().__init__(engine, kind, feature_len, max_observations)
        bind(self.lib)

    def _capacity(self, capacity, keys):
        if capacity is None:
            return None
        if isinstance(capacity, dict):
            return np.array([capacity.get(int(k), self.K) for k in keys], np.uint32)
        if np.ndim(capacity) == 0:
            return np.full(len(keys), int(capacity), np.uint32)
        cap = np.ascontiguousarray(capacity, np.uint32).reshape(-1)
        assert len(cap) == len(keys), "one capacity per destination"
        return cap

    def append(self, ids, feats_per_track, quality=None, keep="latest", capacity=None):
        """bank = old bank ++ the given rows, then the rule once.  quality: per track, an array [n_obs] (or None: zeros), or None for
        all; capacity: None (K), one int, one per id, or {id: C}.  Unknown ids are created; an id without rows stays as it is."""
        ids, n_obs, feats = pack_tracks(ids, feats_per_track, self.D)
        q = None
        if quality is not None:
            assert len(quality) == len(ids), "one quality array per id"
            parts = [np.zeros(int(m), np.float32) if x is None else np.asarray(x, np.float32).reshape(-1) for x, m in zip(quality, n_obs)]
            assert all(len(x) == m for x, m in zip(parts, n_obs)), "one quality per observation"
            q = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0, np.float32), np.float32)
        cap = self._capacity(capacity, ids)
        self._chk(self.lib.sa_store_append(self.h, _keep(keep), len(ids), _p(ids, u64), _p(n_obs, u32), _p(feats, C.c_float),
                                           _p(q, C.c_float), _p(cap, u32)))

    def merge(self, pairs, keep="latest", capacity=None):
        """pairs {dst: [src, ...]}: bank(dst) = dst ++ src0 ++ src1 .., then the rule (always); the sources leave the store as
        remove(all sources in this order) would take them."""
        dst = np.array([int(d) for d in pairs], np.uint64)
        n_src = np.array([len(v) for v in pairs.values()], np.uint32)
        src = np.array([int(x) for v in pairs.values() for x in v], np.uint64)
        cap = self._capacity(capacity, dst)
        self._chk(self.lib.sa_store_merge(self.h, _keep(keep), len(dst), _p(dst, u64), _p(n_src, u32), _p(src, u64), _p(cap, u32)))

    def fetch_raw(self, ids):
        """-> (n_obs [n], feats [n][K][D], quality [n][K]) as the C call writes them."""
        ids = np.ascontiguousarray(ids, np.uint64).reshape(-1)
        n = len(ids)
        n_obs = np.zeros(max(n, 1), np.uint32)
        feats = np.zeros((max(n, 1), self.K, self.D), np.float32)
        qual = np.zeros((max(n, 1), self.K), np.float32)
        self._chk(self.lib.sa_store_fetch(self.h, n, _p(ids, u64), _p(n_obs, u32), _p(feats, C.c_float), _p(qual, C.c_float)))
        return n_obs[:n], feats[:n], qual[:n]

    def fetch(self, ids):
        """{id: (feats [n_obs][D], quality [n_obs])} in bank order; an id the store does not hold has no observations."""
        n_obs, feats, qual = self.fetch_raw(ids)
        return {int(i): (feats[k, : n_obs[k]].copy(), qual[k, : n_obs[k]].copy()) for k, i in enumerate(np.asarray(ids).reshape(-1))}

    def merge_stats(self) -> dict:
        st = sa_merge_stats()
        self._chk(self.lib.sa_store_merge_last(self.h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in sa_merge_stats._fields_}
