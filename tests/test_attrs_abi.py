"""The attribute calls as a library boundary: include/similari_attrs.h declares eight functions beside those of similari_search.h,
similari_gallery.h and similari_merge.h, the library exports them, and similari_amd.attrs binds exactly those."""
import ctypes as C
import re
from pathlib import Path

import pytest

from similari_amd import abi, attrs, build, gallery, merge, search

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "similari_attrs.h"
DECL = re.compile(r"^\s*(?:const\s+)?(?:int|void|uint32_t|uint64_t|double|const char\s*\*)\s*\*?\s*(sa_[a-z0-9_]+)\s*\(", re.M)
NAMES = ["sa_compat_default", "sa_store_compat_last", "sa_store_get_attrs", "sa_store_join_topn_compat", "sa_store_merge_compat",
         "sa_store_search_stored_compat", "sa_store_search_topn_compat", "sa_store_set_attrs"]


def declared():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(DECL.findall(text)))


@pytest.fixture(scope="module")
def lib():
    return attrs.load_library(build.build_lib())


def test_the_header_declares_exactly_the_eight_functions():
    assert declared() == NAMES
    text = HEADER.read_text()
    assert '#include "similari_merge.h"' in text
    for name, value in (("SAME_KEY", 1), ("DISJOINT", 2), ("QUERY_FIRST", 4), ("ONLY_READY", 8)):
        assert re.search(rf"#define\s+SA_COMPAT_{name}\s+{value}u", text)


def test_every_declared_function_is_exported(lib):
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_the_binding_is_the_header():
    assert set(attrs.PROTOTYPES) == set(declared())
    for other in (abi, search, gallery, merge):
        assert not set(attrs.PROTOTYPES) & set(other.PROTOTYPES), other.__name__
    assert (attrs.SA_COMPAT_SAME_KEY, attrs.SA_COMPAT_DISJOINT, attrs.SA_COMPAT_QUERY_FIRST, attrs.SA_COMPAT_ONLY_READY) == (1, 2, 4, 8)


def test_struct_layout(lib):
    assert C.sizeof(attrs.sa_track_attrs) == 24 and attrs.ATTRS_DTYPE.itemsize == 24
    assert C.sizeof(attrs.sa_compat) == 16 and attrs.sa_compat.ready_at.offset == 8
    assert C.sizeof(attrs.sa_compat_stats) == 16
    c = attrs.sa_compat(0, 77, 5)
    lib.sa_compat_default(C.byref(c))
    assert (c.struct_size, c.flags, c.ready_at) == (16, 0, 2**63 - 1)   # the C side wrote its own sizeof
    lib.sa_compat_default(None)
    assert attrs.compat() == attrs.Compat(0, 2**63 - 1)
    assert attrs.compat(same_key=True, disjoint=True) == (3, 2**63 - 1) and attrs.compat(query_first=True, ready_at=-4) == (12, -4)
    packed = attrs.pack_attrs([2**64 - 1], [-(2**63)], [2**63 - 1])
    raw = C.cast(packed.ctypes.data, C.POINTER(attrs.sa_track_attrs))[0]
    assert (raw.key, raw.start, raw.end) == (2**64 - 1, -(2**63), 2**63 - 1)


def test_null_handles_are_refused(lib):
    c = attrs.compat().struct()
    st = attrs.sa_compat_stats()
    assert lib.sa_store_set_attrs(None, 0, None, None) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_get_attrs(None, 0, None, None, None) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_search_topn_compat(None, None, C.byref(c), 0, None, None, None, None, None, None, None, None) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_search_stored_compat(None, None, C.byref(c), 0, 0, None, None, None, None, None) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_join_topn_compat(None, None, C.byref(c), None, None, None, None) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_merge_compat(None, C.byref(c), 0, 0, None, None, None, None) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_compat_last(None, C.byref(st)) == abi.SA_ERR_BAD_ARG


def test_the_header_and_the_sources_are_part_of_the_build():
    assert "sa_attrs.hip" in build.SOURCES
    assert HEADER in build.HEADERS
    assert build.CSRC / "sa_compat.h" in build.HEADERS
    assert '#include "../../include/similari_attrs.h"' in (build.CSRC / "sa_store.h").read_text()
