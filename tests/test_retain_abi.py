"""The absorb under either retention rule as a library boundary: include/similari_retain.h declares three functions beside those of
similari_search.h .. similari_absorb.h, the library exports them, and similari_amd.retain binds exactly that."""
import ctypes as C
import re
from pathlib import Path

import pytest

from similari_amd import abi, absorb, attrs, bestfit, bf16, build, devrows, f16, gallery, merge, retain, search

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "similari_retain.h"
DECL = re.compile(r"^\s*(?:const\s+)?(?:int|void|uint32_t|uint64_t|double|const char\s*\*)\s*\*?\s*(sa_[a-z0-9_]+)\s*\(", re.M)
NAMES = ["sa_store_absorb_keep", "sa_store_absorb_keep_dev", "sa_store_retain_last"]
EARLIER = ("similari_assoc.h", "similari_tracker.h", "similari_search.h", "similari_gallery.h", "similari_merge.h", "similari_attrs.h",
           "similari_bestfit.h", "similari_bf16.h", "similari_f16.h", "similari_devrows.h", "similari_absorb.h")


def declared(header=HEADER):
    text = re.sub(r"/\*.*?\*/", "", Path(header).read_text(), flags=re.S)
    return sorted(set(DECL.findall(text)))


@pytest.fixture(scope="module")
def lib():
    return retain.load_library(build.build_lib())


def test_the_header_declares_exactly_the_three_functions():
    assert declared() == NAMES
    text = HEADER.read_text()
    assert '#include "similari_absorb.h"' in text
    assert "SA_KEEP_BEST is not offered here" in re.sub(r"\s*\n \*\s*", " ", text)   # it says whose follow-up it is
    for h in EARLIER:   # nothing of it went into a header that was there before
        code = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / h).read_text(), flags=re.S)
        assert not [n for n in declared(ROOT / "include" / h) if n in NAMES], h
        for word in ("sa_retain_stats", "similari_retain.h", "qual_upload_bytes"):
            assert word not in code, (h, word)


def test_every_declared_function_is_exported(lib):
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_the_binding_is_the_header():
    assert set(retain.PROTOTYPES) == set(declared())
    for other in (abi, search, gallery, merge, attrs, bestfit, bf16, f16, devrows, absorb):
        assert not set(retain.PROTOTYPES) & set(other.PROTOTYPES), other.__name__
    assert issubclass(retain.RetainStore, absorb.AbsorbStore)
    for name in ("absorb_keep", "absorb_keep_raw", "absorb_keep_rows", "absorb_keep_rows_raw", "retain_stats"):
        assert callable(getattr(retain.RetainStore, name)), name
    # each entry point is its sa_store_absorb twin with `uint32_t keep` behind the store
    for new, old in (("sa_store_absorb_keep", "sa_store_absorb"), ("sa_store_absorb_keep_dev", "sa_store_absorb_dev")):
        a, b = retain.PROTOTYPES[new][1], absorb.PROTOTYPES[old][1]
        assert len(a) == 16 and a[0] is b[0] and a[1] is C.c_uint32 and all(x is y for x, y in zip(a[2:], b[1:])), new
    sig = re.sub(r"\s+", " ", HEADER.read_text())
    assert "int sa_store_absorb_keep(sa_store* s, uint32_t keep, const sa_topn_params* p," in sig
    assert "int sa_store_absorb_keep_dev(sa_store* s, uint32_t keep, const sa_topn_params* p," in sig


def test_struct_layout():
    st = retain.sa_retain_stats
    assert C.sizeof(st) == 40
    assert (st.step_ms.offset, st.matched.offset, st.created.offset, st.rows_moved.offset, st.launches.offset, st.host_waits.offset,
            st.keep.offset, st.qual_upload_bytes.offset) == (0, 8, 12, 16, 20, 24, 28, 32)
    assert re.search(r"\} sa_retain_stats;\s*/\* 40 B \*/", HEADER.read_text())
    # the fields of sa_absorb_stats lead, under their names and at their offsets
    for name, _ in absorb.sa_absorb_stats._fields_:
        assert getattr(st, name).offset == getattr(absorb.sa_absorb_stats, name).offset, name


def test_null_handles_are_refused(lib):
    st = retain.sa_retain_stats()
    rows = devrows.sa_dev_rows()
    prm = search.sa_topn_params(1, 1, 1.0, 1.0)
    c = attrs.compat().struct()
    for keep in (merge.SA_KEEP_LATEST, merge.SA_KEEP_BEST, 7):
        for rule in (None, C.byref(c)):
            assert lib.sa_store_absorb_keep(None, keep, C.byref(prm), rule, 0, None, None, None, None, None, None, None, None, None, None,
                                            None) == abi.SA_ERR_BAD_ARG
            assert lib.sa_store_absorb_keep_dev(None, keep, C.byref(prm), rule, 0, None, None, C.byref(rows), None, None, None, None, None,
                                                None, None, None) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_retain_last(None, C.byref(st)) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_retain_last(None, None) == abi.SA_ERR_BAD_ARG


def test_the_header_and_the_kernel_are_part_of_the_build():
    assert HEADER in build.HEADERS
    assert '#include "../../include/similari_retain.h"' in (build.CSRC / "sa_store.h").read_text()
    src = (build.CSRC / "sa_absorb.hip").read_text()
    assert "k_absorb_move_best" in src and src.index("void k_absorb_move(") < src.index("void k_absorb_move_best(")   # beside k_absorb_move
    assert "k_fit_" not in src   # the vote is still the search's own body
    store = (build.CSRC / "sa_store.h").read_text()
    assert "d_qual" in store and "qual_dirty" in store
