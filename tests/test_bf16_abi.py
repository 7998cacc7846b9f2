"""The bf16 store as a library boundary: include/similari_bf16.h declares two functions beside those of similari_search.h ..
similari_bestfit.h, the library exports them, and similari_amd.bf16 binds exactly those.  sa_store_options keeps its 16 bytes: the
element type travels as an argument of its own."""
import ctypes as C
import re
from pathlib import Path

import pytest

from similari_amd import abi, attrs, bestfit, bf16, build, gallery, merge, search

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "similari_bf16.h"
DECL = re.compile(r"^\s*(?:const\s+)?(?:int|void|uint32_t|uint64_t|double|const char\s*\*)\s*\*?\s*(sa_[a-z0-9_]+)\s*\(", re.M)
NAMES = ["sa_store_create_elem", "sa_store_get_info"]
EARLIER = ("similari_assoc.h", "similari_tracker.h", "similari_search.h", "similari_gallery.h", "similari_merge.h", "similari_attrs.h",
           "similari_bestfit.h")


def declared(header=HEADER):
    text = re.sub(r"/\*.*?\*/", "", Path(header).read_text(), flags=re.S)
    return sorted(set(DECL.findall(text)))


@pytest.fixture(scope="module")
def lib():
    return bf16.load_library(build.build_lib())


def test_the_header_declares_exactly_the_two_functions():
    assert declared() == NAMES
    text = HEADER.read_text()
    assert '#include "similari_bestfit.h"' in text
    assert re.search(r"#define SA_ELEM_F32\s+0\b", text) and re.search(r"#define SA_ELEM_BF16\s+1\b", text)
    assert (bf16.SA_ELEM_F32, bf16.SA_ELEM_BF16) == (0, 1)
    assert re.search(r"typedef struct sa_store_info \{ uint32_t struct_size; int32_t elem; uint32_t Dp, Kp; uint64_t feature_bytes; \}", text)
    for h in EARLIER:   # nothing of it went into a header that was there before
        assert not [n for n in declared(ROOT / "include" / h) if n in NAMES], h


def test_every_declared_function_is_exported(lib):
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_the_binding_is_the_header():
    assert set(bf16.PROTOTYPES) == set(declared())
    for other in (abi, search, gallery, merge, attrs, bestfit):
        assert not set(bf16.PROTOTYPES) & set(other.PROTOTYPES), other.__name__
    assert issubclass(bf16.Bf16Store, bestfit.BestFitStore)
    assert callable(bf16.Bf16Store.info)
    # one overridable creation step, not a copied constructor chain
    assert "_create" in vars(search.FeatureStore) and "_create" in vars(bf16.Bf16Store)
    for cls in (gallery.Gallery, merge.MergeStore, attrs.AttrStore, bestfit.BestFitStore):
        assert "_create" not in vars(cls), cls.__name__


def test_struct_layout():
    st = bf16.sa_store_info
    assert C.sizeof(st) == 24
    assert (st.struct_size.offset, st.elem.offset, st.Dp.offset, st.Kp.offset, st.feature_bytes.offset) == (0, 4, 8, 12, 16)
    assert C.sizeof(search.sa_store_options) == 16   # the options did not grow


def gpu_visible() -> bool:
    import os

    return os.path.exists("/dev/kfd")


@pytest.mark.parametrize("elem", [bf16.SA_ELEM_F32, bf16.SA_ELEM_BF16])
def test_a_null_engine_is_refused_with_a_message(lib, elem):
    """Without a device the answer is SA_ERR_NO_DEVICE, as sa_store_create gives it; with one, a null engine is a bad argument."""
    o = search.sa_store_options()
    lib.sa_store_options_default(C.byref(o))
    o.feature_len = 8
    h = search.STORE()
    rc = lib.sa_store_create_elem(None, C.byref(o), elem, C.byref(h))
    assert rc == (abi.SA_ERR_BAD_ARG if gpu_visible() else abi.SA_ERR_NO_DEVICE) and not h.value
    msg = lib.sa_last_error(None)
    assert msg and (b"null engine" in msg if gpu_visible() else b"no CPU fallback" in msg)


def test_null_handles_are_refused(lib):
    st = bf16.sa_store_info()
    assert lib.sa_store_get_info(None, C.byref(st)) == abi.SA_ERR_BAD_ARG


def test_the_header_and_the_source_are_part_of_the_build():
    assert "sa_bf16.hip" in build.SOURCES
    assert HEADER in build.HEADERS
    assert '#include "../../include/similari_bf16.h"' in (build.CSRC / "sa_store.h").read_text()
    gemm = (build.CSRC / "sa_gemm.hip").read_text()
    assert "k_search_tile_bf16" in gemm and "__builtin_amdgcn_mfma_f32_32x32x16_bf16" in gemm
    assert re.search(r"template <bool EU, bool JOIN, bool COMPAT>\n__global__ [^\n]* void k_search_tile\(", gemm)   # the f32 tile kept its three parameters
