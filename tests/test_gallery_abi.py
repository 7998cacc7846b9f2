"""The gallery calls as a library boundary: include/similari_gallery.h declares three functions beside the nine of similari_search.h,
the library exports them, and similari_amd.gallery binds exactly those."""
import ctypes as C
import re
from pathlib import Path

import pytest

from similari_amd import abi, build, gallery, search

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "similari_gallery.h"
DECL = re.compile(r"^\s*(?:const\s+)?(?:int|void|uint32_t|uint64_t|double|const char\s*\*)\s*\*?\s*(sa_[a-z0-9_]+)\s*\(", re.M)
NAMES = ["sa_store_join_last", "sa_store_join_topn", "sa_store_search_stored"]


def declared():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(DECL.findall(text)))


@pytest.fixture(scope="module")
def lib():
    return gallery.load_library(build.build_lib())


def test_the_header_declares_exactly_the_three_functions():
    assert declared() == NAMES
    text = HEADER.read_text()
    assert '#include "similari_search.h"' in text and re.search(r"#define\s+SA_STORED_WITHDRAW\s+1u", text)


def test_every_declared_function_is_exported(lib):
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_the_binding_is_the_header():
    assert set(gallery.PROTOTYPES) == set(declared())
    assert not set(gallery.PROTOTYPES) & set(abi.PROTOTYPES)
    assert not set(gallery.PROTOTYPES) & set(search.PROTOTYPES)
    assert gallery.SA_STORED_WITHDRAW == 1


def test_struct_layout():
    assert C.sizeof(gallery.sa_join_stats) == 24
    assert gallery.sa_join_stats.blocks.offset == 16


def test_null_handles_are_refused(lib):
    st = gallery.sa_join_stats()
    assert lib.sa_store_search_stored(None, None, 0, 0, None, None, None, None, None) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_join_topn(None, None, None, None, None, None) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_join_last(None, C.byref(st)) == abi.SA_ERR_BAD_ARG


def test_the_header_and_the_sources_are_part_of_the_build():
    assert "sa_gallery.hip" in build.SOURCES
    assert HEADER in build.HEADERS
    assert build.CSRC / "sa_join_tiles.h" in build.HEADERS and build.CSRC / "sa_store.h" in build.HEADERS
