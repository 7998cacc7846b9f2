"""Track search as a library boundary: every function include/similari_search.h declares is exported, similari_amd.search binds
exactly those, and without a gfx950 device there is no store (SA_ERR_NO_DEVICE), as there is no engine."""
import ctypes as C
import os
import re
from pathlib import Path

import pytest

from similari_amd import abi, build, search

ROOT = Path(__file__).resolve().parent.parent
DECL = re.compile(r"^\s*(?:const\s+)?(?:int|void|uint32_t|uint64_t|double|const char\s*\*)\s*\*?\s*(sa_[a-z0-9_]+)\s*\(", re.M)


def declared():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "similari_search.h").read_text(), flags=re.S)
    return sorted(set(DECL.findall(text)))


@pytest.fixture(scope="module")
def lib():
    return search.load_library(build.build_lib())


def test_every_declared_function_is_exported(lib):
    names = declared()
    assert len(names) == 9, names
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


def test_the_binding_is_the_header():
    assert set(search.PROTOTYPES) == set(declared())
    assert not set(search.PROTOTYPES) & set(abi.PROTOTYPES)


def test_the_header_is_part_of_the_build():
    assert "sa_search.hip" in build.SOURCES
    assert ROOT / "include" / "similari_search.h" in build.HEADERS


def test_struct_layouts(lib):
    o = search.sa_store_options()
    lib.sa_store_options_default(C.byref(o))
    assert o.struct_size == C.sizeof(search.sa_store_options) == 16
    assert o.visual_kind == abi.SA_VIS_COSINE and o.max_observations == 1 and o.feature_len == 0
    assert C.sizeof(search.sa_topn_params) == 16 and C.sizeof(search.sa_search_stats) == 40


def test_store_refuses_to_exist_without_a_gpu(lib):
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is visible")
    o = search.sa_store_options()
    lib.sa_store_options_default(C.byref(o))
    o.feature_len = 16
    h = search.STORE()
    assert lib.sa_store_create(None, C.byref(o), C.byref(h)) == abi.SA_ERR_NO_DEVICE
    assert not h.value
    assert b"no CPU fallback" in lib.sa_last_error(None)


def test_null_handles_are_refused(lib):
    n = C.c_uint32()
    assert lib.sa_store_count(None, C.byref(n)) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_upsert(None, 0, None, None, None) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_search_topn(None, None, 0, None, None, None, None, None, None, None) == abi.SA_ERR_BAD_ARG
    lib.sa_store_destroy(None)
