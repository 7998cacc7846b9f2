"""The waste as a library boundary: include/similari_waste.h adds four calls and one stats struct beside those of
similari_search.h .. similari_consolidate.h, the library exports them, similari_amd.waste binds exactly that, and the calls run the
append's and the absorb's own bodies behind one new kernel, not copies of them."""
import ctypes as C
import re
from pathlib import Path

import pytest

from similari_amd import abi, absorb, attrs, bestfit, bf16, build, consolidate, devrows, f16, gallery, handover, i8, merge, retain, search, trackers, waste

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "similari_waste.h"
DECL = re.compile(r"^\s*(?:const\s+)?(?:int|void|uint32_t|uint64_t|double|const char\s*\*)\s*\*?\s*(sa_[a-z0-9_]+)\s*\(", re.M)
NAMES = ["sa_store_waste_last", "sa_tracker_waste_into", "sa_tracks_waste", "sa_tracks_waste_absorb"]
EARLIER = ("similari_assoc.h", "similari_tracker.h", "similari_search.h", "similari_gallery.h", "similari_merge.h", "similari_attrs.h",
           "similari_bestfit.h", "similari_bf16.h", "similari_f16.h", "similari_devrows.h", "similari_absorb.h", "similari_retain.h",
           "similari_i8.h", "similari_framerows.h", "similari_handover.h", "similari_consolidate.h")


def declared(header=HEADER):
    text = re.sub(r"/\*.*?\*/", "", Path(header).read_text(), flags=re.S)
    return sorted(set(DECL.findall(text)))


@pytest.fixture(scope="module")
def lib():
    return waste.load_library(build.build_lib())


def test_the_header_declares_exactly_the_four_calls():
    assert declared() == NAMES
    text = HEADER.read_text()
    assert '#include "similari_consolidate.h"' in text and '#include "similari_tracker.h"' in text
    assert re.search(r"typedef struct sa_waste_stats \{.*?\} sa_waste_stats; /\* 56 B \*/", text, flags=re.S)
    assert "one store per shard is a follow-up" in text
    assert "no later than the wasted() call that reports it" in text
    for h in EARLIER:
        assert not [n for n in declared(ROOT / "include" / h) if n in NAMES], h


def test_the_library_exports_them(lib):
    """Fails on a library built before the waste."""
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_the_binding_is_the_header():
    assert set(waste.PROTOTYPES) == set(declared())
    for other in (abi, search, gallery, merge, attrs, bestfit, bf16, f16, devrows, absorb, retain, i8, handover, consolidate):
        assert not set(waste.PROTOTYPES) & set(other.PROTOTYPES), other.__name__
    for f in ("waste_raw", "waste", "waste_absorb_raw", "waste_absorb", "waste_into", "last", "bind", "load_library"):
        assert callable(getattr(waste, f))
    assert callable(trackers._Tracker.waste_into)
    # the absorb form: the hand-over's arguments with the engine, the scenes and the ids in place of src and ids, and q_attrs
    ho, wa = handover.PROTOTYPES["sa_store_hand_over"][1], waste.PROTOTYPES["sa_tracks_waste_absorb"][1]
    assert wa[2:5] == ho[2:5] and wa[10:] == ho[7:] and wa[9] == C.POINTER(attrs.sa_track_attrs)
    assert wa[5:9] == waste.PROTOTYPES["sa_tracks_waste"][1][3:7] == abi.PROTOTYPES["sa_tracks_remove_many"][1][1:]


def test_the_struct_as_the_header_lays_it_out():
    st = waste.sa_waste_stats
    assert C.sizeof(st) == 56
    want = {"struct_size": 0, "tracks": 4, "launches_capture": 8, "reserved": 12, "rows": 16, "feature_bytes_h2d": 24, "feature_bytes_d2h": 32,
            "table_bytes_d2h": 40, "capture_ms": 48}
    assert {f: getattr(st, f).offset for f, _ in st._fields_} == want
    fields = re.search(r"typedef struct sa_waste_stats \{(.*?)\}", HEADER.read_text(), flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f for f, _ in st._fields_]


def test_bind_attaches_the_prototypes():
    fresh = C.CDLL(str(build.build_lib()))
    assert fresh.sa_tracks_waste.argtypes is None
    waste.bind(fresh)
    for name, (res, args) in waste.PROTOTYPES.items():
        fn = getattr(fresh, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert fresh.sa_store_consolidate.argtypes is not None   # and everything below it (similari_consolidate.h ..)


def test_null_arguments_are_refused(lib):
    """No engine, store or tracker can exist without a device, so what runs here is what the calls answer to null handles."""
    n_obs = (C.c_uint32 * 1)()
    assert lib.sa_tracks_waste(None, None, 0, 0, None, None, None, None, n_obs) == abi.SA_ERR_BAD_ARG
    assert lib.sa_tracks_waste_absorb(None, None, 0, None, None, 0, None, None, None, None, None, None, None, None, None, None) == abi.SA_ERR_BAD_ARG
    assert lib.sa_tracker_waste_into(None, None, 0, 0) == abi.SA_ERR_BAD_ARG
    st = waste.sa_waste_stats()
    st.tracks = 7
    assert lib.sa_store_waste_last(None, C.byref(st)) == abi.SA_ERR_BAD_ARG and st.tracks == 7
    assert lib.sa_store_waste_last(None, None) == abi.SA_ERR_BAD_ARG


def test_the_header_and_the_source_are_part_of_the_build():
    assert "sa_waste.hip" in build.SOURCES
    assert HEADER in build.HEADERS
    assert '#include "../../include/similari_waste.h"' in (build.CSRC / "sa_store.h").read_text()
    src = (build.CSRC / "sa_waste.hip").read_text()
    # the bodies are the append's, the absorb's and the removal's own; the one new kernel is the capture
    for k in ("k_waste_capture", "sa_store_append_impl", "sa_store_absorb_impl", "sa_tracks_remove_many", "SaRowSource::of_own", "sa_engine_waste_resolve"):
        assert k in src, k
    assert "k_pad_rows" not in src.split("namespace {", 1)[1] and "hipMemcpyDeviceToDevice" not in src
    assert "__shared__" not in src
    for f in ("sa_merge.hip", "sa_search.hip"):   # the bodies do not switch on the row source: the one fill does, and pads f32 rows the library owns
        text = (build.CSRC / f).read_text()
        assert "sa_rows_fill(s, R" in text and "SaRowSource::OWN" not in text and "sa_devrows_pad_own" not in text, f
    fill = (build.CSRC / "sa_devrows.hip").read_text()
    fill = fill[fill.index("int sa_rows_prepare("): fill.index('extern "C" {')]
    assert "SaRowSource::OWN" in fill and "sa_devrows_pad_own(s, R" in fill and "int elem = SA_ELEM_F32" in (build.CSRC / "sa_store.h").read_text()
    trk = (build.CSRC / "sa_tracker.cpp").read_text()
    assert "sa_tracks_waste(" in trk and "first_epoch" in trk
