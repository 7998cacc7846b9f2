"""The f16 store as a library boundary: include/similari_f16.h adds one element type to sa_store_create_elem and declares one
function beside those of similari_search.h .. similari_bf16.h, the library exports it, and similari_amd.f16 binds exactly that."""
import ctypes as C
import re
from pathlib import Path

import pytest

from similari_amd import abi, attrs, bestfit, bf16, build, f16, gallery, merge, search

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "similari_f16.h"
DECL = re.compile(r"^\s*(?:const\s+)?(?:int|void|uint32_t|uint64_t|double|const char\s*\*)\s*\*?\s*(sa_[a-z0-9_]+)\s*\(", re.M)
NAMES = ["sa_store_expand_last"]
EARLIER = ("similari_assoc.h", "similari_tracker.h", "similari_search.h", "similari_gallery.h", "similari_merge.h", "similari_attrs.h",
           "similari_bestfit.h", "similari_bf16.h")


def declared(header=HEADER):
    text = re.sub(r"/\*.*?\*/", "", Path(header).read_text(), flags=re.S)
    return sorted(set(DECL.findall(text)))


@pytest.fixture(scope="module")
def lib():
    return f16.load_library(build.build_lib())


def test_the_header_declares_the_constant_and_the_one_function():
    assert declared() == NAMES
    text = HEADER.read_text()
    assert '#include "similari_bf16.h"' in text
    assert re.search(r"#define SA_ELEM_F16\s+2\b", text)
    assert (f16.SA_ELEM_F32, f16.SA_ELEM_BF16, f16.SA_ELEM_F16) == (0, 1, 2)
    assert (f16.SA_ELEM_F32, f16.SA_ELEM_BF16) == (bf16.SA_ELEM_F32, bf16.SA_ELEM_BF16)
    assert re.search(r"typedef struct sa_expand_stats \{ uint32_t struct_size; uint32_t reserved; uint64_t cells, tiles; \}", text)
    for h in EARLIER:   # nothing of it went into a header that was there before
        assert not [n for n in declared(ROOT / "include" / h) if n in NAMES], h
        assert "SA_ELEM_F16" not in re.sub(r"/\*.*?\*/", "", (ROOT / "include" / h).read_text(), flags=re.S), h


def test_every_declared_function_is_exported(lib):
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_the_binding_is_the_header():
    assert set(f16.PROTOTYPES) == set(declared())
    for other in (abi, search, gallery, merge, attrs, bestfit, bf16):
        assert not set(f16.PROTOTYPES) & set(other.PROTOTYPES), other.__name__
    assert issubclass(f16.F16Store, bestfit.BestFitStore) and not issubclass(f16.F16Store, bf16.Bf16Store)
    assert callable(f16.F16Store.info) and callable(f16.F16Store.expand_stats)
    assert "_create" in vars(f16.F16Store)


def test_struct_layout():
    st = f16.sa_expand_stats
    assert C.sizeof(st) == 24
    assert (st.struct_size.offset, st.reserved.offset, st.cells.offset, st.tiles.offset) == (0, 4, 8, 16)
    assert C.sizeof(search.sa_store_options) == 16   # the options did not grow


def gpu_visible() -> bool:
    import os

    return os.path.exists("/dev/kfd")


@pytest.mark.parametrize("kind", [abi.SA_VIS_COSINE, abi.SA_VIS_EUCLIDEAN])
def test_a_null_engine_is_refused_with_a_message(lib, kind):
    """Without a device the answer is SA_ERR_NO_DEVICE, as sa_store_create gives it; with one, a null engine is a bad argument."""
    o = search.sa_store_options()
    lib.sa_store_options_default(C.byref(o))
    o.feature_len = 8
    o.visual_kind = kind
    h = search.STORE()
    rc = lib.sa_store_create_elem(None, C.byref(o), f16.SA_ELEM_F16, C.byref(h))
    assert rc == (abi.SA_ERR_BAD_ARG if gpu_visible() else abi.SA_ERR_NO_DEVICE) and not h.value
    msg = lib.sa_last_error(None)
    assert msg and (b"null engine" in msg if gpu_visible() else b"no CPU fallback" in msg)


def test_null_handles_are_refused(lib):
    st = f16.sa_expand_stats()
    assert lib.sa_store_expand_last(None, C.byref(st)) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_expand_last(None, None) == abi.SA_ERR_BAD_ARG


def test_the_header_and_the_source_are_part_of_the_build():
    assert "sa_f16.hip" in build.SOURCES
    assert HEADER in build.HEADERS
    assert '#include "../../include/similari_f16.h"' in (build.CSRC / "sa_store.h").read_text()
    gemm = (build.CSRC / "sa_gemm.hip").read_text()
    assert "k_search_tile_f16" in gemm and "__builtin_amdgcn_mfma_f32_32x32x16_f16" in gemm
    # no pad kernel of its own: the 16-bit DST branch of the one pad kernel rounds on the way in
    texts = {f.name: f.read_text() for f in build.CSRC.iterdir()}
    assert not [f for f, t in texts.items() for k in ("k_pad_features_bf16", "k_pad_features_f16", "k_pad_features_i8") if k in t]
    pad = (build.CSRC / "sa_devrows.hip").read_text()
    assert "} else if (DST != SA_ELEM_F32) {" in pad and "DST == SA_ELEM_BF16 ? bf16_bits(x) : f16_bits(x)" in pad and "f16_widen(b)" in pad
    assert "SA_ELEM_F16" in (build.CSRC / "sa_bf16.hip").read_text()   # the creation call names the third constant
