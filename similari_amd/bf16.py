"""ctypes mirror of include/similari_bf16.h (feature stores whose rows are bf16) and Bf16Store, the Python face of it.

A Bf16Store is a BestFitStore — search, stored search, join, append / merge / fetch, the *_compat calls, the BestFit calls — whose rows
are rounded once to bf16 on the way in and contracted on the bf16 matrix instruction with f32 accumulators.  It behaves as an f32 store
fed with `bf16(x)` for every feature value x, of stored rows and of query rows alike; the calls keep taking and returning f32 rows.
Cosine only; half the memory of an f32 store.

    store = Bf16Store(engine, "cosine", feature_len=512, max_observations=32)
    store.info()   # {"struct_size": 24, "elem": 1, "Dp": 512, "Kp": 32, "feature_bytes": ...}
"""
from __future__ import annotations

import ctypes as C

from . import abi
from . import bestfit as _bestfit
from .bestfit import BestFitStore
from .search import STORE, sa_store_options

u32, u64, i32 = C.c_uint32, C.c_uint64, C.c_int32
P = C.POINTER
SA_ELEM_F32, SA_ELEM_BF16 = 0, 1


class sa_store_info(C.Structure):
    _fields_ = [("struct_size", u32), ("elem", i32), ("Dp", u32), ("Kp", u32), ("feature_bytes", u64)]


# ---- prototypes of every symbol include/similari_bf16.h declares ---------------------------------
PROTOTYPES = {
    "sa_store_create_elem": (C.c_int, [abi.ENGINE, P(sa_store_options), i32, P(STORE)]),
    "sa_store_get_info": (C.c_int, [STORE, P(sa_store_info)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach the prototypes of similari_search.h .. similari_bf16.h to a library abi.load_library returned."""
    _bestfit.bind(lib)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library(path=None) -> C.CDLL:
    return bind(abi.load_library(path))


def store_info(store) -> dict:
    """sa_store_get_info of any store (an f32 store answers elem 0)."""
    bind(store.lib)
    st = sa_store_info()
    store._chk(store.lib.sa_store_get_info(store.h, C.byref(st)))
    return {f: getattr(st, f) for f, _ in sa_store_info._fields_}


class Bf16Store(BestFitStore):
    """A BestFitStore whose rows are bf16 (elem: SA_ELEM_BF16; SA_ELEM_F32 creates what BestFitStore creates)."""

    def __init__(self, engine, kind: str = "cosine", feature_len: int = 0, max_observations: int = 1, elem: int = SA_ELEM_BF16):
        self.elem = int(elem)
        super().__init__(engine, kind, feature_len, max_observations)

    def _create(self, o) -> int:
        bind(self.lib)
        return self.lib.sa_store_create_elem(self.engine.h, C.byref(o), self.elem, C.byref(self.h))

    def info(self) -> dict:
        """{"struct_size", "elem", "Dp", "Kp", "feature_bytes"}: the fields of sa_store_info."""
        return store_info(self)
