"""The BestFit calls as a library boundary: include/similari_bestfit.h declares four functions beside those of similari_search.h ..
similari_attrs.h, the library exports them, and similari_amd.bestfit binds exactly those."""
import ctypes as C
import re
from pathlib import Path

import pytest

from similari_amd import abi, attrs, bestfit, build, gallery, merge, search

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "similari_bestfit.h"
DECL = re.compile(r"^\s*(?:const\s+)?(?:int|void|uint32_t|uint64_t|double|const char\s*\*)\s*\*?\s*(sa_[a-z0-9_]+)\s*\(", re.M)
NAMES = ["sa_store_bestfit_last", "sa_store_join_bestfit", "sa_store_search_bestfit", "sa_store_search_stored_bestfit"]
EARLIER = ("similari_assoc.h", "similari_tracker.h", "similari_search.h", "similari_gallery.h", "similari_merge.h", "similari_attrs.h")


def declared(header=HEADER):
    text = re.sub(r"/\*.*?\*/", "", Path(header).read_text(), flags=re.S)
    return sorted(set(DECL.findall(text)))


@pytest.fixture(scope="module")
def lib():
    return bestfit.load_library(build.build_lib())


def test_the_header_declares_exactly_the_four_functions():
    assert declared() == NAMES
    text = HEADER.read_text()
    assert '#include "similari_attrs.h"' in text
    assert re.search(r"typedef struct sa_bestfit_stats \{ double weigh_ms, claim_ms, rank_ms; uint32_t groups; uint32_t claimed; \}", text)
    for h in EARLIER:   # nothing of it went into a header that was there before
        assert not [n for n in declared(ROOT / "include" / h) if "bestfit" in n], h


def test_every_declared_function_is_exported(lib):
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_the_binding_is_the_header():
    assert set(bestfit.PROTOTYPES) == set(declared())
    for other in (abi, search, gallery, merge, attrs):
        assert not set(bestfit.PROTOTYPES) & set(other.PROTOTYPES), other.__name__
    assert issubclass(bestfit.BestFitStore, attrs.AttrStore)
    for name in ("search_bestfit", "search_stored_bestfit", "join_bestfit"):
        assert callable(getattr(bestfit.BestFitStore, name)) and callable(getattr(bestfit.BestFitStore, name + "_raw"))
    assert callable(bestfit.BestFitStore.bestfit_stats)


def test_struct_layout():
    st = bestfit.sa_bestfit_stats
    assert C.sizeof(st) == 32
    assert (st.weigh_ms.offset, st.claim_ms.offset, st.rank_ms.offset, st.groups.offset, st.claimed.offset) == (0, 8, 16, 24, 28)


def test_null_handles_are_refused(lib):
    c = attrs.compat().struct()
    st = bestfit.sa_bestfit_stats()
    for rule in (None, C.byref(c)):
        assert lib.sa_store_search_bestfit(None, None, rule, 0, None, None, None, None, None, None, None, None, None) == abi.SA_ERR_BAD_ARG
        assert lib.sa_store_search_stored_bestfit(None, None, rule, 0, 0, None, None, None, None, None, None) == abi.SA_ERR_BAD_ARG
        assert lib.sa_store_join_bestfit(None, None, rule, None, None, None, None, None) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_bestfit_last(None, C.byref(st)) == abi.SA_ERR_BAD_ARG


def test_the_header_and_the_sources_are_part_of_the_build():
    assert "sa_bestfit.hip" in build.SOURCES
    assert HEADER in build.HEADERS
    assert build.CSRC / "sa_vote_weight.h" in build.HEADERS
    assert '#include "../../include/similari_bestfit.h"' in (build.CSRC / "sa_store.h").read_text()
    for src in ("sa_search.hip", "sa_bestfit.hip"):   # one statement of the weights under both votes
        text = (build.CSRC / src).read_text()
        assert '#include "sa_vote_weight.h"' in text and "double block_weight" not in text
