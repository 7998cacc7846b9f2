"""Bank upkeep as a library boundary: include/similari_merge.h declares four functions beside those of similari_search.h and
similari_gallery.h, the library exports them, and similari_amd.merge binds exactly those."""
import ctypes as C
import re
from pathlib import Path

import pytest

from similari_amd import abi, build, gallery, merge, search

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "similari_merge.h"
DECL = re.compile(r"^\s*(?:const\s+)?(?:int|void|uint32_t|uint64_t|double|const char\s*\*)\s*\*?\s*(sa_[a-z0-9_]+)\s*\(", re.M)
NAMES = ["sa_store_append", "sa_store_fetch", "sa_store_merge", "sa_store_merge_last"]


def declared():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(DECL.findall(text)))


@pytest.fixture(scope="module")
def lib():
    return merge.load_library(build.build_lib())


def test_the_header_declares_exactly_the_four_functions():
    assert declared() == NAMES
    text = HEADER.read_text()
    assert '#include "similari_gallery.h"' in text
    assert re.search(r"#define\s+SA_KEEP_LATEST\s+0u", text) and re.search(r"#define\s+SA_KEEP_BEST\s+1u", text)


def test_every_declared_function_is_exported(lib):
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_the_binding_is_the_header():
    assert set(merge.PROTOTYPES) == set(declared())
    for other in (abi, search, gallery):
        assert not set(merge.PROTOTYPES) & set(other.PROTOTYPES)
    assert (merge.SA_KEEP_LATEST, merge.SA_KEEP_BEST) == (0, 1)
    assert merge.KEEP == {"latest": 0, "best": 1}


def test_struct_layout():
    assert C.sizeof(merge.sa_merge_stats) == 32
    assert merge.sa_merge_stats.launches.offset == 28


def test_null_handles_are_refused(lib):
    st = merge.sa_merge_stats()
    assert lib.sa_store_append(None, 0, 0, None, None, None, None, None) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_merge(None, 0, 0, None, None, None, None) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_fetch(None, 0, None, None, None, None) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_merge_last(None, C.byref(st)) == abi.SA_ERR_BAD_ARG


def test_the_header_and_the_sources_are_part_of_the_build():
    assert "sa_merge.hip" in build.SOURCES
    assert HEADER in build.HEADERS
    assert build.CSRC / "sa_merge_plan.h" in build.HEADERS
    # the two older public headers know nothing of this one
    for h in ("similari_search.h", "similari_gallery.h"):
        assert "similari_merge" not in (ROOT / "include" / h).read_text()
