"""ctypes mirror of include/similari_i8.h (feature stores whose rows are int8 codes) and I8Store, the Python face of it.

An I8Store is a RetainStore — search, stored search, join, append / merge / fetch, the *_compat calls, the BestFit calls, rows from
device memory, absorb under either rule — whose rows are replaced by their int8 codes on the way in (127 / absmax per row, round half
to even) and contracted on the int8 matrix instruction with exact i32 accumulators.  A per-row scale cancels in the cosine, so the
store keeps none: it behaves as an f32 store fed with `codes(x)` for every row x, of stored rows and of query rows alike; the calls
keep taking and returning f32 rows, and fetch returns the codes (integers in -127 .. 127).  Cosine only; a quarter of the memory of
an f32 store; feature_len <= 131072.

    store = I8Store(engine, "cosine", feature_len=512, max_observations=32)
    store.info()           # {"struct_size": 24, "elem": 8, "Dp": 512, "Kp": 32, "feature_bytes": ...}
"""
from __future__ import annotations

import ctypes as C

from . import abi
from . import retain as _retain
from .bf16 import SA_ELEM_BF16, SA_ELEM_F32   # noqa: F401  (the element types side by side)
from .f16 import SA_ELEM_F16   # noqa: F401
from .retain import RetainStore
from .search import STORE, sa_store_options

P = C.POINTER
SA_ELEM_I8 = 8
SA_I8_MAX_FEATURE_LEN = 131072

# ---- prototypes of every symbol include/similari_i8.h declares -----------------------------------
PROTOTYPES = {
    "sa_store_create_i8": (C.c_int, [abi.ENGINE, P(sa_store_options), P(STORE)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach the prototypes of similari_search.h .. similari_i8.h to a library abi.load_library returned."""
    _retain.bind(lib)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library(path=None) -> C.CDLL:
    return bind(abi.load_library(path))


class I8Store(RetainStore):
    """A RetainStore whose rows are int8 codes (elem: SA_ELEM_I8), cosine only."""

    def __init__(self, engine, kind: str = "cosine", feature_len: int = 0, max_observations: int = 1):
        super().__init__(engine, kind, feature_len, max_observations, SA_ELEM_I8)

    def _create(self, o) -> int:
        bind(self.lib)
        return self.lib.sa_store_create_i8(self.engine.h, C.byref(o), C.byref(self.h))
