"""ctypes mirror of include/similari_f16.h (feature stores whose rows are IEEE binary16) and F16Store, the Python face of it.

An F16Store is a BestFitStore — search, stored search, join, append / merge / fetch, the *_compat calls, the BestFit calls — whose rows
are rounded once to f16 on the way in and contracted on the f16 matrix instruction with f32 accumulators.  It behaves as an f32 store
fed with `f16(x)` for every feature value x, of stored rows and of query rows alike; the calls keep taking and returning f32 rows.
Cosine AND euclidean; half the memory of an f32 store; rows that are f16-representable (a ReID network's fp16 embeddings) are stored
without loss.

    store = F16Store(engine, "euclidean", feature_len=512, max_observations=32)
    store.info()           # {"struct_size": 24, "elem": 2, "Dp": 512, "Kp": 32, "feature_bytes": ...}
    store.expand_stats()   # {"cells": ..., "tiles": ...}: what launch 1 of the last search recomputed directly
"""
from __future__ import annotations

import ctypes as C

from . import bf16 as _bf16
from .bestfit import BestFitStore
from .bf16 import SA_ELEM_BF16, SA_ELEM_F32, sa_store_info, store_info   # noqa: F401  (the element types side by side)
from .search import STORE

u32, u64 = C.c_uint32, C.c_uint64
P = C.POINTER
SA_ELEM_F16 = 2


class sa_expand_stats(C.Structure):
    _fields_ = [("struct_size", u32), ("reserved", u32), ("cells", u64), ("tiles", u64)]


# ---- prototypes of every symbol include/similari_f16.h declares ----------------------------------
PROTOTYPES = {
    "sa_store_expand_last": (C.c_int, [STORE, P(sa_expand_stats)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach the prototypes of similari_search.h .. similari_f16.h to a library abi.load_library returned."""
    _bf16.bind(lib)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library(path=None) -> C.CDLL:
    from . import abi

    return bind(abi.load_library(path))


def expand_stats(store) -> dict:
    """sa_store_expand_last of any store (zeros unless it is an f16 euclidean store that has searched)."""
    bind(store.lib)
    st = sa_expand_stats()
    store._chk(store.lib.sa_store_expand_last(store.h, C.byref(st)))
    return {"cells": int(st.cells), "tiles": int(st.tiles)}


class F16Store(BestFitStore):
    """A BestFitStore whose rows are f16 (elem: SA_ELEM_F16), for either metric."""

    def __init__(self, engine, kind: str = "cosine", feature_len: int = 0, max_observations: int = 1, elem: int = SA_ELEM_F16):
        self.elem = int(elem)
        super().__init__(engine, kind, feature_len, max_observations)

    def _create(self, o) -> int:
        bind(self.lib)
        return self.lib.sa_store_create_elem(self.engine.h, C.byref(o), self.elem, C.byref(self.h))

    def info(self) -> dict:
        """{"struct_size", "elem", "Dp", "Kp", "feature_bytes"}: the fields of sa_store_info."""
        return store_info(self)

    def expand_stats(self) -> dict:
        """{"cells", "tiles"}: flagged cells launch 1 of the last search recomputed directly, and tiles that recomputed any."""
        return expand_stats(self)
