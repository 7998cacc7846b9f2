"""The i8 store as a library boundary: include/similari_i8.h adds one element type and one creation call beside those of
similari_search.h .. similari_retain.h, the library exports it, and similari_amd.i8 binds exactly that."""
import ctypes as C
import re
from pathlib import Path

import pytest

from similari_amd import abi, absorb, attrs, bestfit, bf16, build, devrows, f16, gallery, i8, merge, retain, search

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "similari_i8.h"
DECL = re.compile(r"^\s*(?:const\s+)?(?:int|void|uint32_t|uint64_t|double|const char\s*\*)\s*\*?\s*(sa_[a-z0-9_]+)\s*\(", re.M)
NAMES = ["sa_store_create_i8"]
EARLIER = ("similari_assoc.h", "similari_tracker.h", "similari_search.h", "similari_gallery.h", "similari_merge.h", "similari_attrs.h",
           "similari_bestfit.h", "similari_bf16.h", "similari_f16.h", "similari_devrows.h", "similari_absorb.h", "similari_retain.h")


def declared(header=HEADER):
    text = re.sub(r"/\*.*?\*/", "", Path(header).read_text(), flags=re.S)
    return sorted(set(DECL.findall(text)))


@pytest.fixture(scope="module")
def lib():
    return i8.load_library(build.build_lib())


def test_the_header_declares_the_constant_and_the_one_function():
    assert declared() == NAMES
    text = HEADER.read_text()
    assert '#include "similari_retain.h"' in text
    assert re.search(r"#define SA_ELEM_I8\s+8\b", text) and re.search(r"#define SA_I8_MAX_FEATURE_LEN\s+131072u\b", text)
    assert (i8.SA_ELEM_F32, i8.SA_ELEM_BF16, i8.SA_ELEM_F16, i8.SA_ELEM_I8) == (0, 1, 2, 8)
    assert i8.SA_I8_MAX_FEATURE_LEN == 131072 and 127 * 127 * i8.SA_I8_MAX_FEATURE_LEN < 2**31
    for h in EARLIER:   # nothing of it went into a header that was there before
        assert not [n for n in declared(ROOT / "include" / h) if n in NAMES], h
        assert "SA_ELEM_I8" not in re.sub(r"/\*.*?\*/", "", (ROOT / "include" / h).read_text(), flags=re.S), h


def test_the_library_exports_the_creation_call(lib):
    """Fails on a library built before the i8 store."""
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_the_binding_is_the_header():
    assert set(i8.PROTOTYPES) == set(declared())
    for other in (abi, search, gallery, merge, attrs, bestfit, bf16, f16, devrows, absorb, retain):
        assert not set(i8.PROTOTYPES) & set(other.PROTOTYPES), other.__name__
    assert issubclass(i8.I8Store, retain.RetainStore)
    assert "_create" in vars(i8.I8Store)
    assert C.sizeof(search.sa_store_options) == 16   # the options did not grow


def test_bind_attaches_the_prototype():
    fresh = C.CDLL(str(build.build_lib()))
    assert fresh.sa_store_create_i8.argtypes is None
    i8.bind(fresh)
    res, args = i8.PROTOTYPES["sa_store_create_i8"]
    assert fresh.sa_store_create_i8.restype is res and list(fresh.sa_store_create_i8.argtypes) == args
    assert fresh.sa_store_absorb_keep.argtypes is not None   # and everything below it (similari_retain.h ..)


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
    rc = lib.sa_store_create_i8(None, C.byref(o), C.byref(h))
    assert rc == (abi.SA_ERR_BAD_ARG if gpu_visible() else abi.SA_ERR_NO_DEVICE) and not h.value
    msg = lib.sa_last_error(None)
    assert msg and (b"null engine" in msg if gpu_visible() else b"no CPU fallback" in msg)


def test_create_elem_keeps_its_three_element_types(lib):
    """sa_store_create_elem is as it was: the i8 store has a call of its own."""
    text = (build.CSRC / "sa_bf16.hip").read_text()
    assert "unknown element type %d (SA_ELEM_F32, SA_ELEM_BF16, SA_ELEM_F16)" in text and "SA_ELEM_I8" not in text


def test_the_header_and_the_source_are_part_of_the_build():
    assert "sa_i8.hip" in build.SOURCES
    assert HEADER in build.HEADERS
    assert '#include "../../include/similari_i8.h"' in (build.CSRC / "sa_store.h").read_text()
    gemm = (build.CSRC / "sa_gemm.hip").read_text()
    assert "k_search_tile_i8" in gemm and "__builtin_amdgcn_mfma_i32_32x32x32_i8" in gemm
    # no pad kernel of its own: the codes are taken by the i8 DST branch of the one pad kernel
    texts = {f.name: f.read_text() for f in build.CSRC.iterdir()}
    assert not [f for f, t in texts.items() for k in ("k_pad_features_bf16", "k_pad_features_f16", "k_pad_features_i8") if k in t]
    assert "k_pad_rows<SRC, SA_ELEM_I8>" in (build.CSRC / "sa_devrows.hip").read_text()
