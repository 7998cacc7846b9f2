"""ctypes mirror of include/similari_absorb.h (a frame's tracks absorbed in one call) and AbsorbStore, the Python face of it.

AbsorbStore.absorb is the reference's incremental loop for one batch of new tracks (examples/incremental_track_build.rs,
benches/feature_tracker.rs): a BestFit search, then every matched query's rows join its winner's bank and every other query becomes a
track under its own id — what search_bestfit followed by append leaves, bit for bit, in one call whose step runs on the device.

    winners, dest = store.absorb(ids, feats, topn=1, max_distance=0.3, capacity=3)
    new = [q for q in ids if dest[q] == q]          # the tracks this frame created
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import attrs as _attrs
from . import devrows as _devrows
from .attrs import sa_compat, sa_track_attrs
from .devrows import DeviceRowsStore, _rows, sa_dev_rows
from .f16 import SA_ELEM_F32
from .search import STORE, _p, pack_tracks, sa_topn_params

u32, u64 = C.c_uint32, C.c_uint64
P = C.POINTER


class sa_absorb_stats(C.Structure):
    _fields_ = [("step_ms", C.c_double), ("matched", u32), ("created", u32), ("rows_moved", u32), ("launches", u32), ("host_waits", u32)]


# ---- prototypes of every symbol include/similari_absorb.h declares -------------------------------
_TAIL = [P(sa_track_attrs), P(C.c_float), P(u32), P(u32), P(u64), P(u64), P(C.c_double), P(u64)]
PROTOTYPES = {
    "sa_store_absorb": (C.c_int, [STORE, P(sa_topn_params), P(sa_compat), u32, P(u64), P(u32), P(C.c_float)] + _TAIL),
    "sa_store_absorb_dev": (C.c_int, [STORE, P(sa_topn_params), P(sa_compat), u32, P(u64), P(u32), P(sa_dev_rows)] + _TAIL),
    "sa_store_absorb_last": (C.c_int, [STORE, P(sa_absorb_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach the prototypes of similari_search.h .. similari_absorb.h to a library abi.load_library returned."""
    _devrows.bind(lib)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library(path=None) -> C.CDLL:
    from . import abi

    return bind(abi.load_library(path))


def _quality(quality, n_obs):
    """Per query an array [n_obs] (or None: zeros), or None for all -> one f32 per observation in call order, or None."""
    if quality is None:
        return None
    assert len(quality) == len(n_obs), "one quality array per query"
    parts = [np.zeros(int(m), np.float32) if x is None else np.asarray(x, np.float32).reshape(-1) for x, m in zip(quality, n_obs)]
    assert all(len(x) == m for x, m in zip(parts, n_obs)), "one quality per observation"
    return np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0, np.float32), np.float32)


class AbsorbStore(DeviceRowsStore):
    """A DeviceRowsStore that absorbs a frame's tracks in one call.  The retention rule is "keep the last C" (capacity as
    MergeStore.append takes it)."""

    def __init__(self, engine, kind: str = "cosine", feature_len: int = 0, max_observations: int = 1, elem: int = SA_ELEM_F32):
        super().__init__(engine, kind, feature_len, max_observations, elem)
        bind(self.lib)

    def _absorb_call(self, symbol, ids, n_obs, rows_arg, topn, max_distance, min_votes, keep_below, quality, capacity, compat, attrs, track):
        n = len(ids)
        prm = sa_topn_params(int(topn), int(min_votes), float(max_distance), float(keep_below))
        rule = _attrs._rule(compat)
        qa = _attrs._attrs(attrs)
        assert qa is None or len(qa) == n, "one sa_track_attrs per query"
        q = None if quality is None else np.ascontiguousarray(quality, np.float32).reshape(-1)
        assert q is None or len(q) == int(n_obs.sum()), "one quality per observation"
        cap = self._capacity(capacity, ids)
        shape = (max(n, 1), max(int(topn), 1))
        out_n = np.zeros(shape[0], np.uint32)
        win = np.zeros(shape, np.uint64)
        trk = np.zeros(shape, np.uint64) if track else None
        wt = np.zeros(shape, np.float64)
        dest = np.zeros(shape[0], np.uint64)
        self._chk(getattr(self.lib, symbol)(self.h, C.byref(prm), None if rule is None else C.byref(rule), n, _p(ids, u64), _p(n_obs, u32),
                                            rows_arg, _p(qa, sa_track_attrs), _p(q, C.c_float), _p(cap, u32), _p(out_n, u32),
                                            _p(win, u64), _p(trk, u64), _p(wt, C.c_double), _p(dest, u64)))
        return out_n[:n], win[:n], None if trk is None else trk[:n], wt[:n], dest[:n]

    def absorb_raw(self, ids, feats_per_track, topn, max_distance, min_votes=1, keep_below=math.inf, quality=None, capacity=None,
                   compat=None, attrs=None, track=True):
        """-> (out_n [Q], winners [Q][topn], tracks [Q][topn] or None, weights [Q][topn], dest [Q]) as the C call writes them.
        quality: per query an array [n_obs] (or None: zeros), or None for all."""
        ids, n_obs, feats = pack_tracks(ids, feats_per_track, self.D)
        return self._absorb_call("sa_store_absorb", ids, n_obs, _p(feats, C.c_float), topn, max_distance, min_votes, keep_below,
                                 _quality(quality, n_obs), capacity, compat, attrs, track)

    def absorb_rows_raw(self, ids, n_obs, rows, topn, max_distance, min_votes=1, keep_below=math.inf, quality=None, capacity=None,
                        compat=None, attrs=None, track=True):
        """absorb_raw with the query rows in device memory (a DeviceRows); quality: one f32 per observation in call order, or None."""
        ids, n_obs = self._table(ids, n_obs)
        alive, r = _rows(rows)
        return self._absorb_call("sa_store_absorb_dev", ids, n_obs, r, topn, max_distance, min_votes, keep_below, quality, capacity,
                                 compat, attrs, track)

    @staticmethod
    def _maps(ids, out):
        out_n, win, trk, wt, dest = out
        ids = np.asarray(ids, np.uint64).reshape(-1)
        res = {int(q): [(int(win[i, r]), float(wt[i, r]), int(trk[i, r])) for r in range(int(out_n[i]))] for i, q in enumerate(ids) if out_n[i]}
        return res, {int(q): int(dest[i]) for i, q in enumerate(ids)}

    def absorb(self, ids, feats_per_track, topn, max_distance, min_votes=1, keep_below=math.inf, quality=None, capacity=None, compat=None,
               attrs=None):
        """({query id: [(winner id, weight, track id), ...]}, {query id: the track that took its rows — a stored one, or itself})."""
        return self._maps(ids, self.absorb_raw(ids, feats_per_track, topn, max_distance, min_votes, keep_below, quality, capacity, compat, attrs))

    def absorb_rows(self, ids, n_obs, rows, topn, max_distance, min_votes=1, keep_below=math.inf, quality=None, capacity=None, compat=None,
                    attrs=None):
        """absorb with the query rows in device memory."""
        return self._maps(ids, self.absorb_rows_raw(ids, n_obs, rows, topn, max_distance, min_votes, keep_below, quality, capacity, compat, attrs))

    def absorb_stats(self) -> dict:
        """{"step_ms", "matched", "created", "rows_moved", "launches", "host_waits"} of the last absorb."""
        st = sa_absorb_stats()
        self._chk(self.lib.sa_store_absorb_last(self.h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in sa_absorb_stats._fields_}
