"""The absorb as a library boundary: include/similari_absorb.h declares three functions beside those of similari_search.h ..
similari_devrows.h, the library exports them, and similari_amd.absorb binds exactly that."""
import ctypes as C
import re
from pathlib import Path

import pytest

from similari_amd import abi, absorb, attrs, bestfit, bf16, build, devrows, f16, gallery, merge, search

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "similari_absorb.h"
DECL = re.compile(r"^\s*(?:const\s+)?(?:int|void|uint32_t|uint64_t|double|const char\s*\*)\s*\*?\s*(sa_[a-z0-9_]+)\s*\(", re.M)
NAMES = ["sa_store_absorb", "sa_store_absorb_dev", "sa_store_absorb_last"]
EARLIER = ("similari_assoc.h", "similari_tracker.h", "similari_search.h", "similari_gallery.h", "similari_merge.h", "similari_attrs.h",
           "similari_bestfit.h", "similari_bf16.h", "similari_f16.h", "similari_devrows.h")


def declared(header=HEADER):
    text = re.sub(r"/\*.*?\*/", "", Path(header).read_text(), flags=re.S)
    return sorted(set(DECL.findall(text)))


@pytest.fixture(scope="module")
def lib():
    return absorb.load_library(build.build_lib())


def test_the_header_declares_exactly_the_three_functions():
    assert declared() == NAMES
    text = HEADER.read_text()
    assert '#include "similari_devrows.h"' in text
    assert "SA_KEEP_BEST is not offered here" in text   # the known follow-up is stated where a caller reads it
    for h in EARLIER:   # nothing of it went into a header that was there before
        code = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / h).read_text(), flags=re.S)
        assert not [n for n in declared(ROOT / "include" / h) if n in NAMES], h
        for word in ("sa_absorb_stats", "similari_absorb.h"):
            assert word not in code, (h, word)


def test_every_declared_function_is_exported(lib):
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_the_binding_is_the_header():
    assert set(absorb.PROTOTYPES) == set(declared())
    for other in (abi, search, gallery, merge, attrs, bestfit, bf16, f16, devrows):
        assert not set(absorb.PROTOTYPES) & set(other.PROTOTYPES), other.__name__
    assert issubclass(absorb.AbsorbStore, devrows.DeviceRowsStore)
    for name in ("absorb", "absorb_raw", "absorb_rows", "absorb_rows_raw", "absorb_stats"):
        assert callable(getattr(absorb.AbsorbStore, name)), name
    # the two entry points differ in the row source alone
    host, dev = absorb.PROTOTYPES["sa_store_absorb"][1], absorb.PROTOTYPES["sa_store_absorb_dev"][1]
    assert len(host) == len(dev) == 15 and [a is b for a, b in zip(host, dev)].count(False) == 1
    assert host[6] is C.POINTER(C.c_float) and dev[6] is C.POINTER(devrows.sa_dev_rows)


def test_struct_layout():
    st = absorb.sa_absorb_stats
    assert C.sizeof(st) == 32
    assert (st.step_ms.offset, st.matched.offset, st.created.offset, st.rows_moved.offset, st.launches.offset, st.host_waits.offset) == (0, 8, 12, 16, 20, 24)
    assert re.search(r"\} sa_absorb_stats;\s*/\* 32 B \*/", HEADER.read_text())


def test_null_handles_are_refused(lib):
    st = absorb.sa_absorb_stats()
    rows = devrows.sa_dev_rows()
    prm = search.sa_topn_params(1, 1, 1.0, 1.0)
    c = attrs.compat().struct()
    for rule in (None, C.byref(c)):
        assert lib.sa_store_absorb(None, C.byref(prm), rule, 0, None, None, None, None, None, None, None, None, None, None, None) == abi.SA_ERR_BAD_ARG
        assert lib.sa_store_absorb_dev(None, C.byref(prm), rule, 0, None, None, C.byref(rows), None, None, None, None, None, None, None,
                                       None) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_absorb_last(None, C.byref(st)) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_absorb_last(None, None) == abi.SA_ERR_BAD_ARG


def test_the_header_and_the_source_are_part_of_the_build():
    assert "sa_absorb.hip" in build.SOURCES
    assert HEADER in build.HEADERS
    assert '#include "../../include/similari_absorb.h"' in (build.CSRC / "sa_store.h").read_text()
    src = (build.CSRC / "sa_absorb.hip").read_text()
    for k in ("k_absorb_match", "k_absorb_rank", "k_absorb_move"):
        assert k in src
    assert "sa_store_search_topn_impl" in src and "k_fit_" not in src   # the vote is the search's own body, not a copy of it
