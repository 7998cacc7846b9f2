"""ctypes mirror of include/similari_retain.h (a frame's tracks absorbed under either retention rule) and RetainStore, the Python
face of it.

RetainStore.absorb_keep is AbsorbStore.absorb with the rule as an argument: keep="best" is the loop of examples/track_merging.rs and
of VisualSORT's feature banks — the bank stays sorted by quality, the C best observations survive — what search_bestfit followed by
append(keep="best") leaves, bit for bit, in one call whose step runs on the device.

    winners, dest = store.absorb_keep(ids, feats, topn=1, max_distance=0.3, quality=q, capacity=3)     # keep="best"
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import absorb as _absorb
from . import attrs as _attrs
from .absorb import _TAIL, AbsorbStore, _quality
from .attrs import sa_compat, sa_track_attrs
from .devrows import _rows, sa_dev_rows
from .f16 import SA_ELEM_F32
from .merge import _keep
from .search import STORE, _p, pack_tracks, sa_topn_params

u32, u64 = C.c_uint32, C.c_uint64
P = C.POINTER


class sa_retain_stats(C.Structure):
    _fields_ = [("step_ms", C.c_double), ("matched", u32), ("created", u32), ("rows_moved", u32), ("launches", u32), ("host_waits", u32),
                ("keep", u32), ("qual_upload_bytes", u64)]


# ---- prototypes of every symbol include/similari_retain.h declares -------------------------------
PROTOTYPES = {
    "sa_store_absorb_keep": (C.c_int, [STORE, u32, P(sa_topn_params), P(sa_compat), u32, P(u64), P(u32), P(C.c_float)] + _TAIL),
    "sa_store_absorb_keep_dev": (C.c_int, [STORE, u32, P(sa_topn_params), P(sa_compat), u32, P(u64), P(u32), P(sa_dev_rows)] + _TAIL),
    "sa_store_retain_last": (C.c_int, [STORE, P(sa_retain_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach the prototypes of similari_search.h .. similari_retain.h to a library abi.load_library returned."""
    _absorb.bind(lib)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library(path=None) -> C.CDLL:
    from . import abi

    return bind(abi.load_library(path))


class RetainStore(AbsorbStore):
    """An AbsorbStore whose absorb takes the retention rule: "best" (the default here) or "latest"."""

    def __init__(self, engine, kind: str = "cosine", feature_len: int = 0, max_observations: int = 1, elem: int = SA_ELEM_F32):
        super().__init__(engine, kind, feature_len, max_observations, elem)
        bind(self.lib)

    def _keep_call(self, symbol, keep, ids, n_obs, rows_arg, topn, max_distance, min_votes, keep_below, quality, capacity, compat, attrs, track):
        """AbsorbStore._absorb_call with the rule behind the store handle."""
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
        self._chk(getattr(self.lib, symbol)(self.h, _keep(keep), C.byref(prm), None if rule is None else C.byref(rule), n, _p(ids, u64),
                                            _p(n_obs, u32), rows_arg, _p(qa, sa_track_attrs), _p(q, C.c_float), _p(cap, u32),
                                            _p(out_n, u32), _p(win, u64), _p(trk, u64), _p(wt, C.c_double), _p(dest, u64)))
        return out_n[:n], win[:n], None if trk is None else trk[:n], wt[:n], dest[:n]

    def absorb_keep_raw(self, ids, feats_per_track, topn, max_distance, keep="best", min_votes=1, keep_below=math.inf, quality=None,
                        capacity=None, compat=None, attrs=None, track=True):
        """AbsorbStore.absorb_raw under the rule `keep`: -> (out_n, winners, tracks or None, weights, dest)."""
        ids, n_obs, feats = pack_tracks(ids, feats_per_track, self.D)
        return self._keep_call("sa_store_absorb_keep", keep, ids, n_obs, _p(feats, C.c_float), topn, max_distance, min_votes, keep_below,
                               _quality(quality, n_obs), capacity, compat, attrs, track)

    def absorb_keep_rows_raw(self, ids, n_obs, rows, topn, max_distance, keep="best", min_votes=1, keep_below=math.inf, quality=None,
                             capacity=None, compat=None, attrs=None, track=True):
        """AbsorbStore.absorb_rows_raw under the rule `keep` (quality: one f32 per observation in call order, or None)."""
        ids, n_obs = self._table(ids, n_obs)
        alive, r = _rows(rows)
        return self._keep_call("sa_store_absorb_keep_dev", keep, ids, n_obs, r, topn, max_distance, min_votes, keep_below, quality, capacity,
                               compat, attrs, track)

    def absorb_keep(self, ids, feats_per_track, topn, max_distance, keep="best", min_votes=1, keep_below=math.inf, quality=None,
                    capacity=None, compat=None, attrs=None):
        """({query id: [(winner id, weight, track id), ...]}, {query id: the track that took its rows}), as AbsorbStore.absorb."""
        return self._maps(ids, self.absorb_keep_raw(ids, feats_per_track, topn, max_distance, keep, min_votes, keep_below, quality, capacity,
                                                    compat, attrs))

    def absorb_keep_rows(self, ids, n_obs, rows, topn, max_distance, keep="best", min_votes=1, keep_below=math.inf, quality=None,
                         capacity=None, compat=None, attrs=None):
        """absorb_keep with the query rows in device memory."""
        return self._maps(ids, self.absorb_keep_rows_raw(ids, n_obs, rows, topn, max_distance, keep, min_votes, keep_below, quality, capacity,
                                                         compat, attrs))

    def retain_stats(self) -> dict:
        """The fields of absorb_stats() plus "keep" and "qual_upload_bytes", of the last absorb through any entry point."""
        st = sa_retain_stats()
        self._chk(self.lib.sa_store_retain_last(self.h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in sa_retain_stats._fields_}
