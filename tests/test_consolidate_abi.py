"""The consolidation as a library boundary: include/similari_consolidate.h adds two calls and one stats struct beside those of
similari_search.h .. similari_handover.h, the library exports them, similari_amd.consolidate binds exactly that, and the step runs
behind the join's own body and the absorb's own moves, not behind copies of them."""
import ctypes as C
import re
from pathlib import Path

import pytest

from similari_amd import abi, absorb, attrs, bestfit, bf16, build, consolidate, devrows, f16, gallery, handover, i8, merge, retain, search

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "similari_consolidate.h"
DECL = re.compile(r"^\s*(?:const\s+)?(?:int|void|uint32_t|uint64_t|double|const char\s*\*)\s*\*?\s*(sa_[a-z0-9_]+)\s*\(", re.M)
NAMES = ["sa_store_consolidate", "sa_store_consolidate_last"]
EARLIER = ("similari_assoc.h", "similari_tracker.h", "similari_search.h", "similari_gallery.h", "similari_merge.h", "similari_attrs.h",
           "similari_bestfit.h", "similari_bf16.h", "similari_f16.h", "similari_devrows.h", "similari_absorb.h", "similari_retain.h",
           "similari_i8.h", "similari_framerows.h", "similari_handover.h")


def declared(header=HEADER):
    text = re.sub(r"/\*.*?\*/", "", Path(header).read_text(), flags=re.S)
    return sorted(set(DECL.findall(text)))


@pytest.fixture(scope="module")
def lib():
    return consolidate.load_library(build.build_lib())


def test_the_header_declares_exactly_the_two_calls():
    assert declared() == NAMES
    text = HEADER.read_text()
    assert '#include "similari_handover.h"' in text
    assert re.search(r"typedef struct sa_consolidate_stats \{.*?\} sa_consolidate_stats; /\* 48 B \*/", text, flags=re.S)
    assert "pairs, not clusters" in text
    for h in EARLIER:
        assert not [n for n in declared(ROOT / "include" / h) if n in NAMES], h
        assert "consolidate" not in (ROOT / "include" / h).read_text(), h


def test_the_library_exports_them(lib):
    """Fails on a library built before the consolidation."""
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_the_binding_is_the_header():
    assert set(consolidate.PROTOTYPES) == set(declared())
    for other in (abi, search, gallery, merge, attrs, bestfit, bf16, f16, devrows, absorb, retain, i8, handover):
        assert not set(consolidate.PROTOTYPES) & set(other.PROTOTYPES), other.__name__
    for f in ("consolidate_raw", "consolidate", "consolidate_all", "last", "bind", "load_library"):
        assert callable(getattr(consolidate, f))
    # the outputs are the join's, then the ids and the destinations
    assert consolidate.PROTOTYPES["sa_store_consolidate"][1][5:9] == bestfit._OUT[:4]


def test_the_struct_as_the_header_lays_it_out():
    st = consolidate.sa_consolidate_stats
    assert C.sizeof(st) == 48
    want = {"step_ms": 0, "compact_ms": 8, "pairs": 16, "rows_moved": 20, "tracks_moved": 24, "launches": 28, "host_waits": 32, "keep": 36,
            "qual_upload_bytes": 40}
    assert {f: getattr(st, f).offset for f, _ in st._fields_} == want
    fields = re.search(r"typedef struct sa_consolidate_stats \{(.*?)\}", HEADER.read_text(), flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f for f, _ in st._fields_]


def test_bind_attaches_the_prototypes():
    fresh = C.CDLL(str(build.build_lib()))
    assert fresh.sa_store_consolidate.argtypes is None
    consolidate.bind(fresh)
    for name, (res, args) in consolidate.PROTOTYPES.items():
        fn = getattr(fresh, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert fresh.sa_store_hand_over.argtypes is not None   # and everything below it (similari_handover.h ..)


def test_null_handles_are_refused(lib):
    """No store can exist without a device, so what runs here is what both calls answer to a null handle."""
    assert lib.sa_store_consolidate(None, 0, None, None, 0, None, None, None, None, None, None) == abi.SA_ERR_BAD_ARG
    st = consolidate.sa_consolidate_stats()
    st.pairs = 7
    assert lib.sa_store_consolidate_last(None, C.byref(st)) == abi.SA_ERR_BAD_ARG and st.pairs == 7
    assert lib.sa_store_consolidate_last(None, None) == abi.SA_ERR_BAD_ARG


def test_the_header_and_the_source_are_part_of_the_build():
    assert "sa_consolidate.hip" in build.SOURCES
    assert HEADER in build.HEADERS
    assert '#include "../../include/similari_consolidate.h"' in (build.CSRC / "sa_store.h").read_text()
    src = (build.CSRC / "sa_consolidate.hip").read_text()
    assert "sa_store_join_topn_impl" in src and "k_fit_" not in src   # the vote is the join's own body, not a copy of it
    for k in ("k_consolidate_pair", "k_consolidate_merge", "k_consolidate_merge_best", "sa_store_remove_slots"):
        assert k in src
    # the moves are the absorb's, once: both sources call the shared header
    shared = (build.CSRC / "sa_bank_move.h").read_text()
    for f in ("sa_bank_find_slot", "sa_bank_take_latest", "sa_bank_take_best"):
        assert f in shared and f in src and f in (build.CSRC / "sa_absorb.hip").read_text(), f
    # the join body calls the step's check and prepare
    join = (build.CSRC / "sa_gallery.hip").read_text()
    join = join[join.index("int sa_store_join_topn_impl("):]
    assert "step->check" in join and "step->prepare()" in join
