"""The cases of tests/golden/store_rows_parent.npz, shared by its recorder (tests/golden/make_store_rows_golden.py) and its test
(tests/test_gpu_store_rows_golden.py): host-fed calls on a feature store of every element type, at the smallest shapes at which the
fill of padded rows and their norms can go wrong.

Inputs are integer arithmetic, no RNG stream: the fixture holds outputs only and the cases are the same anywhere.

  stores  f32 cosine / euclidean, bf16 cosine, f16 cosine / euclidean, i8 cosine; K = 3 (Kp = 4)
  widths  5    odd, one chunk, the f32 store's one-element-per-lane norm order
          64   D == Dp
          100  the f32 store's float4 order with a row ending mid-step
          129  the second step of a 16-bit store, with a pair that is half padding
          260  the second step of the f32 float4 order and of the i8 store's four-per-lane order, with one live lane
  special one +-inf row and one NaN row, stored and queried, in the D = 100 case of every store (bytes are compared, so they count)
  calls   upsert of 5 tracks with 3, 1, 0, 2, 3 observations; append (keep latest) of one row to a full track and to a track of one,
          and of a new track of two; a tapped search of 4 queries with 2, 0, 3, 1 observations; fetch of everything
  null    per store, at D = 64: an upsert and a search in which every count is 0 and the feature pointer is null
"""
import ctypes as C
import hashlib

import numpy as np

from similari_amd.f16 import SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_F32
from similari_amd.i8 import I8Store
from similari_amd.retain import RetainStore
from similari_amd.search import _p

u32, u64 = np.uint32, np.uint64
K = 3
FAR = 3.0e38   # above every distance
TOPN = 3
ELEM = {"f32": SA_ELEM_F32, "bf16": SA_ELEM_BF16, "f16": SA_ELEM_F16}
STORES = [("f32", "cosine"), ("f32", "euclidean"), ("bf16", "cosine"), ("f16", "cosine"), ("f16", "euclidean"), ("i8", "cosine")]
WIDTHS = [5, 64, 100, 129, 260]
SPECIAL_D, NULL_D = 100, 64
UPSERT_IDS, UPSERT_OBS = [1, 2, 3, 4, 5], [3, 1, 0, 2, 3]
APPEND_IDS, APPEND_OBS = [1, 2, 6], [1, 1, 2]
QUERY_IDS, QUERY_OBS = [1001, 1002, 1003, 1004], [2, 0, 3, 1]
FULL_BYTES = 8192   # a fetched row image above this is recorded as its SHA-256
OUTPUTS = ("out_n", "winners", "weights", "cells", "n_obs", "feats", "quality")

# (store, kind, D, null) of every case, in the order they are recorded
CASES = [(s, kind, D, False) for s, kind in STORES for D in WIDTHS] + [(s, kind, NULL_D, True) for s, kind in STORES]


def case_name(case):
    s, kind, D, null = case
    return "%s_%s_d%d%s" % (s, kind, D, "_null" if null else "")


def rows(n, D, salt, special=False):
    """[n][D] f32: ((r * 131 + k * 71 + salt) % 257 - 128) / 64, multiples of 1/64 in [-2, 2]; special: +-inf in row 1, NaNs in row 4."""
    r = np.arange(n, dtype=np.int64)[:, None]
    k = np.arange(D, dtype=np.int64)[None, :]
    x = (((r * 131 + k * 71 + salt) % 257 - 128) / 64.0).astype(np.float32)
    if special:
        x[1, D - 1], x[1, 0] = np.inf, -np.inf
        x[4, D // 2], x[4, 0] = np.nan, -np.nan
    return x


def banks(x, n_obs):
    """The per-track arrays of a call whose observations are the rows of x in order."""
    off = np.concatenate([[0], np.cumsum(n_obs)])
    return [x[off[i]: off[i + 1]] for i in range(len(n_obs))]


def make_store(engine, case):
    s, kind, D, _ = case
    return I8Store(engine, kind, D, K) if s == "i8" else RetainStore(engine, kind, D, K, ELEM[s])


def run_case(engine, case):
    """-> {name: array} for OUTPUTS: what the search returned (tapped) and what the store then holds."""
    _, _, D, null = case
    store = make_store(engine, case)
    try:
        if null:
            ids, none = np.array(UPSERT_IDS, u64), np.zeros(len(UPSERT_IDS), u32)
            store._chk(store.lib.sa_store_upsert(store.h, len(ids), _p(ids, C.c_uint64), _p(none, C.c_uint32), None))
            q_ids, q_none = np.array(QUERY_IDS, u64), np.zeros(len(QUERY_IDS), u32)
            args = [len(q_ids), _p(q_ids, C.c_uint64), _p(q_none, C.c_uint32), None]
            found = store._search_call("sa_store_search_topn", len(q_ids), args, TOPN, FAR, 1, np.inf, True)
        else:
            special = D == SPECIAL_D
            store.upsert(UPSERT_IDS, banks(rows(sum(UPSERT_OBS), D, 0, special), UPSERT_OBS))
            store.append(APPEND_IDS, banks(rows(sum(APPEND_OBS), D, 37), APPEND_OBS), keep="latest")
            found = store.search_raw(QUERY_IDS, banks(rows(sum(QUERY_OBS), D, 90, special), QUERY_OBS), TOPN, FAR, tap=True)
        held = store.fetch_raw(store.order())
    finally:
        store.close()
    return dict(zip(OUTPUTS, (*found, *held)))


def recorded(out):
    """The outputs of a case as the fixture keeps them: every array in full, but a large row image as its SHA-256 (uint8 [32])."""
    out = {k: np.ascontiguousarray(v) for k, v in out.items()}
    if out["feats"].nbytes > FULL_BYTES:
        out["feats"] = np.frombuffer(hashlib.sha256(out["feats"].tobytes()).digest(), np.uint8)
    return out
