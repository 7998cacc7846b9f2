"""ctypes mirror of include/similari_devrows.h (feature rows read from device memory) and DeviceRowsStore, the Python face of it.

A DeviceRowsStore is an F16Store of any of the three element types whose upsert, append and host-fed searches also take their rows
where a ReID network left them: f32, f16 or bf16 elements in device memory, strided and optionally gathered by a row index.  A *_rows
call returns, and leaves in the store, exactly the bits the host call returns and leaves when it is fed the same values widened to f32.

    with register_tensor(engine, emb):                       # emb: a [B, W] fp16 tensor on the store's GPU
        rows = DeviceRows.from_tensor(emb[:, 4:4 + 512])     # a column slice: the row stride is W
        store.upsert_rows(ids, n_obs, rows)                  # rows must be final: synchronize the producer's stream first
        out_n, win, wt, _ = store.search_rows_raw(q_ids, q_n_obs, rows, topn=5, max_distance=0.4)
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math

import numpy as np

from . import attrs as _attrs
from . import f16 as _f16
from .attrs import sa_compat, sa_track_attrs
from .f16 import SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_F32, F16Store
from .merge import _keep
from .search import STORE, _p, sa_topn_params

u32, u64, i32 = C.c_uint32, C.c_uint64, C.c_int32
P = C.POINTER
SA_VOTE_TOPN, SA_VOTE_BESTFIT = 0, 1
VOTE = {"topn": SA_VOTE_TOPN, "bestfit": SA_VOTE_BESTFIT}
ELEM_BYTES = {SA_ELEM_F32: 4, SA_ELEM_BF16: 2, SA_ELEM_F16: 2}
ELEM_OF_DTYPE = {"float32": SA_ELEM_F32, "float16": SA_ELEM_F16, "bfloat16": SA_ELEM_BF16}


class sa_dev_rows(C.Structure):
    _fields_ = [("struct_size", u32), ("elem", i32), ("base", C.c_void_p), ("n_rows", u64), ("row_stride", u64), ("index", P(u32))]


class sa_devrows_stats(C.Structure):
    _fields_ = [("struct_size", u32), ("reserved", u32), ("rows", u64), ("wide_rows", u64), ("src_bytes", u64)]


# ---- prototypes of every symbol include/similari_devrows.h declares ------------------------------
PROTOTYPES = {
    "sa_store_upsert_dev": (C.c_int, [STORE, u32, P(u64), P(u32), P(sa_dev_rows)]),
    "sa_store_append_dev": (C.c_int, [STORE, u32, u32, P(u64), P(u32), P(sa_dev_rows), P(C.c_float), P(u32)]),
    "sa_store_search_dev": (C.c_int, [STORE, P(sa_topn_params), u32, P(sa_compat), u32, P(u64), P(u32), P(sa_dev_rows), P(sa_track_attrs),
                                      P(u32), P(u64), P(u64), P(C.c_double), P(C.c_float)]),
    "sa_store_devrows_last": (C.c_int, [STORE, P(sa_devrows_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach the prototypes of similari_search.h .. similari_devrows.h to a library abi.load_library returned."""
    _f16.bind(lib)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library(path=None) -> C.CDLL:
    from . import abi

    return bind(abi.load_library(path))


class DeviceRows:
    """The descriptor of rows in device memory: `ptr` is the device address of element 0 of row 0, `row_stride` counts ELEMENTS, `elem`
    is SA_ELEM_F32 / SA_ELEM_BF16 / SA_ELEM_F16, `index` (or None: 0, 1, 2, ...) names the source row of each observation in call order."""

    def __init__(self, ptr, n_rows, row_stride, elem, index=None):
        self.ptr, self.n_rows, self.row_stride, self.elem = int(ptr), int(n_rows), int(row_stride), int(elem)
        self.index = None if index is None else np.ascontiguousarray(index, np.uint32).reshape(-1)

    @classmethod
    def from_tensor(cls, t, index=None):
        """From any 2-D object with data_ptr(), dtype, shape and stride() — a torch tensor on the GPU, float32 / float16 / bfloat16 —
        whose last stride is 1.  Any row stride: a column slice of a wider tensor works."""
        name = str(t.dtype).rsplit(".", 1)[-1]
        if name not in ELEM_OF_DTYPE:
            raise TypeError(f"DeviceRows.from_tensor: dtype {t.dtype} (float32, float16 or bfloat16)")
        if len(t.shape) != 2:
            raise ValueError("DeviceRows.from_tensor: a 2-D tensor [rows][D]")
        if t.shape[1] > 1 and t.stride()[1] != 1:
            raise ValueError("DeviceRows.from_tensor: the last stride must be 1")
        if t.shape[0] > 1 and t.stride()[0] < t.shape[1]:
            raise ValueError("DeviceRows.from_tensor: rows overlap (row stride below the row length)")
        stride = t.stride()[0] if t.shape[0] > 1 else max(int(t.stride()[0]), int(t.shape[1]))
        return cls(t.data_ptr(), t.shape[0], stride, ELEM_OF_DTYPE[name], index)

    def struct(self) -> sa_dev_rows:
        """The C struct; it borrows self.index, so self must outlive the call."""
        ix = C.cast(None, P(u32)) if self.index is None else self.index.ctypes.data_as(P(u32))
        return sa_dev_rows(C.sizeof(sa_dev_rows), self.elem, C.c_void_p(self.ptr), self.n_rows, self.row_stride, ix)


def _rows(rows):
    """(keep-alive, pointer) of a DeviceRows, an sa_dev_rows or None (a null pointer)."""
    if rows is None:
        return None, None
    st = rows if isinstance(rows, sa_dev_rows) else rows.struct()
    return (rows, st), C.byref(st)


@contextlib.contextmanager
def register_tensor(engine, t):
    """Registers the whole storage under tensor `t` with engine.register_device_block for the body and unregisters it on exit."""
    st = t.untyped_storage()
    ptr = st.data_ptr()
    engine.register_device_block(ptr, st.nbytes())
    try:
        yield t
    finally:
        engine.unregister_device_block(ptr)


def devrows_stats(store) -> dict:
    """sa_store_devrows_last of any store (zeros before its first *_dev call)."""
    bind(store.lib)
    st = sa_devrows_stats()
    store._chk(store.lib.sa_store_devrows_last(store.h, C.byref(st)))
    return {"rows": int(st.rows), "wide_rows": int(st.wide_rows), "src_bytes": int(st.src_bytes)}


class DeviceRowsStore(F16Store):
    """An F16Store (elem: any of the three element types) whose rows can come from device memory."""

    def __init__(self, engine, kind: str = "cosine", feature_len: int = 0, max_observations: int = 1, elem: int = SA_ELEM_F16):
        super().__init__(engine, kind, feature_len, max_observations, elem)
        bind(self.lib)

    @staticmethod
    def _table(ids, n_obs):
        ids = np.ascontiguousarray(ids, np.uint64).reshape(-1)
        n_obs = np.ascontiguousarray(n_obs, np.uint32).reshape(-1)
        assert len(ids) == len(n_obs), "one observation count per id"
        return ids, n_obs

    def upsert_rows(self, ids, n_obs, rows):
        """upsert with the banks' rows in device memory: track i takes the next n_obs[i] rows (of rows.index, or 0, 1, 2, ...)."""
        ids, n_obs = self._table(ids, n_obs)
        alive, r = _rows(rows)
        self._chk(self.lib.sa_store_upsert_dev(self.h, len(ids), _p(ids, u64), _p(n_obs, u32), r))

    def append_rows(self, ids, n_obs, rows, quality=None, capacity=None, keep="latest"):
        """append with the new rows in device memory.  quality: one f32 per observation in call order, or None (zeros); capacity as
        MergeStore.append takes it."""
        ids, n_obs = self._table(ids, n_obs)
        q = None if quality is None else np.ascontiguousarray(quality, np.float32).reshape(-1)
        assert q is None or len(q) == int(n_obs.sum()), "one quality per observation"
        cap = self._capacity(capacity, ids)
        alive, r = _rows(rows)
        self._chk(self.lib.sa_store_append_dev(self.h, _keep(keep), len(ids), _p(ids, u64), _p(n_obs, u32), r, _p(q, C.c_float), _p(cap, u32)))

    def search_rows_raw(self, q_ids, q_n_obs, rows, topn, max_distance, min_votes=1, keep_below=math.inf, vote="topn", compat=None,
                        q_attrs=None, tap=False, track=True):
        """What search_raw (vote "topn": (out_n, winners, weights, cells)) or search_bestfit_raw (vote "bestfit": (out_n, winners,
        tracks, weights, cells)) returns, for query rows in device memory.  vote may also be the raw integer."""
        q_ids, q_n_obs = self._table(q_ids, q_n_obs)
        n = len(q_ids)
        v = VOTE[vote] if isinstance(vote, str) else int(vote)
        fit = v == SA_VOTE_BESTFIT
        prm = sa_topn_params(int(topn), int(min_votes), float(max_distance), float(keep_below))
        rule = _attrs._rule(compat)
        qa = _attrs._attrs(q_attrs)
        assert qa is None or len(qa) == n, "one sa_track_attrs per query"
        shape = (max(n, 1), max(int(topn), 1))
        out_n = np.zeros(shape[0], np.uint32)
        win = np.zeros(shape, np.uint64)
        trk = np.zeros(shape, np.uint64) if fit and track else None
        wt = np.zeros(shape, np.float64)
        cells = np.empty((n, self.K, len(self), self.K), np.float32) if tap else None
        alive, r = _rows(rows)
        self._chk(self.lib.sa_store_search_dev(self.h, C.byref(prm), v, None if rule is None else C.byref(rule), n, _p(q_ids, u64),
                                               _p(q_n_obs, u32), r, _p(qa, sa_track_attrs), _p(out_n, u32), _p(win, u64), _p(trk, u64),
                                               _p(wt, C.c_double), _p(cells, C.c_float)))
        if fit:
            return out_n[:n], win[:n], None if trk is None else trk[:n], wt[:n], cells
        return out_n[:n], win[:n], wt[:n], cells

    def search_rows(self, q_ids, q_n_obs, rows, topn, max_distance, min_votes=1, keep_below=math.inf, vote="topn", compat=None,
                    q_attrs=None, tap=False):
        """What search_topn / search_bestfit return: {query id: [(winner id, weight[, track id]), ...]} (and the cells when tap=True)."""
        out = self.search_rows_raw(q_ids, q_n_obs, rows, topn, max_distance, min_votes, keep_below, vote, compat, q_attrs, tap)
        ids = np.asarray(q_ids, np.uint64).reshape(-1)
        if len(out) == 5:
            out_n, win, trk, wt, cells = out
            res = {int(q): [(int(win[i, r]), float(wt[i, r]), int(trk[i, r])) for r in range(int(out_n[i]))] for i, q in enumerate(ids) if out_n[i]}
        else:
            out_n, win, wt, cells = out
            res = {int(q): [(int(win[i, r]), float(wt[i, r])) for r in range(int(out_n[i]))] for i, q in enumerate(ids) if out_n[i]}
        return (res, cells) if tap else res

    def devrows_stats(self) -> dict:
        """{"rows", "wide_rows", "src_bytes"} of the last *_rows call."""
        return devrows_stats(self)
