"""A frame's rows from device memory as a library boundary: include/similari_framerows.h declares ten functions beside those of
similari_devrows.h and similari_tracker.h, the library exports them, similari_amd.framerows binds exactly that, and nothing of it
went into a header that was there before."""
import ctypes as C
import re
from pathlib import Path

import pytest

from similari_amd import abi, absorb, attrs, bestfit, bf16, build, devrows, f16, framerows, gallery, i8, merge, retain, search

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "similari_framerows.h"
DECL = re.compile(r"^\s*(?:const\s+)?(?:int|void|uint32_t|uint64_t|double|sa_engine\s*\*|const char\s*\*)\s*\*?\s*(sa_[a-z0-9_]+)\s*\(", re.M)
NAMES = sorted(["sa_associate_dev", "sa_batch_add_dev", "sa_batch_add_deferred_dev", "sa_associate_batch_dev", "sa_pipe_stage_dev",
                "sa_pipe_submit_dev", "sa_tracker_predict_dev", "sa_tracker_predict_batch_begin_dev", "sa_framerows_last"])
EARLIER = ("similari_assoc.h", "similari_tracker.h", "similari_search.h", "similari_gallery.h", "similari_merge.h", "similari_attrs.h",
           "similari_bestfit.h", "similari_bf16.h", "similari_f16.h", "similari_devrows.h", "similari_absorb.h", "similari_retain.h",
           "similari_i8.h")
OTHERS = (abi, search, gallery, merge, attrs, bestfit, bf16, f16, devrows, absorb, retain, i8)


def declared(header=HEADER):
    text = re.sub(r"/\*.*?\*/", "", Path(header).read_text(), flags=re.S)
    return sorted(set(DECL.findall(text)))


@pytest.fixture(scope="module")
def lib():
    return framerows.load_library(build.build_lib())


def test_the_header_declares_exactly_its_functions():
    """The eight *_dev calls, sa_framerows_last and, with the struct it fills, nothing else: nine functions plus one typedef make the ten
    declarations of the header."""
    assert declared() == NAMES
    text = HEADER.read_text()
    assert '#include "similari_devrows.h"' in text and '#include "similari_tracker.h"' in text
    assert re.search(r"typedef struct sa_framerows_stats \{[^}]*\} sa_framerows_stats;\s*/\* 32 B \*/", text)


def test_the_row_none_constant_is_pinned():
    assert re.search(r"#define SA_ROW_NONE\s+0xFFFFFFFFu\b", HEADER.read_text())
    assert framerows.SA_ROW_NONE == 0xFFFFFFFF


def test_every_declared_function_is_exported(lib):
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_the_binding_is_the_header():
    assert set(framerows.PROTOTYPES) == set(declared())
    for other in OTHERS:
        assert not set(framerows.PROTOTYPES) & set(other.PROTOTYPES), other.__name__
    for name in ("associate_rows", "batch_add_rows", "make_requests_rows", "associate_batch_rows", "pipe_stage_rows", "pipe_submit_rows",
                 "framerows_stats", "predict_rows", "predict_batch_rows"):
        assert callable(getattr(framerows, name)), name
    assert framerows.DeviceRows is devrows.DeviceRows and framerows.register_tensor is devrows.register_tensor
    assert "import torch" not in (ROOT / "similari_amd" / "framerows.py").read_text()


def test_struct_layout():
    st = framerows.sa_framerows_stats
    assert C.sizeof(st) == 32
    assert (st.struct_size.offset, st.launches.offset, st.rows.offset, st.wide_rows.offset, st.src_bytes.offset) == (0, 4, 8, 16, 24)


def test_the_old_headers_are_as_they_were():
    """68 and 21 functions in the two headers of the per-frame surface, and none of the new names or types in any earlier header."""
    assert len(declared(ROOT / "include" / "similari_assoc.h")) == 68
    assert len(declared(ROOT / "include" / "similari_tracker.h")) == 21
    for h in EARLIER:
        code = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / h).read_text(), flags=re.S)
        assert not [n for n in declared(ROOT / "include" / h) if n in NAMES], h
        for word in ("sa_framerows_stats", "SA_ROW_NONE", "similari_framerows.h"):
            assert word not in code, (h, word)
    bound = set(abi.PROTOTYPES)
    assert bound == set(declared(ROOT / "include" / "similari_assoc.h")) | set(declared(ROOT / "include" / "similari_tracker.h"))


def test_null_handles_are_refused(lib):
    st = framerows.sa_framerows_stats()
    rows = devrows.sa_dev_rows()
    det = abi.sa_detections()
    rp = (framerows.ROWS_P * 1)(C.pointer(rows))
    t, h = C.c_uint64(), C.c_void_p()
    bad = abi.SA_ERR_BAD_ARG
    assert lib.sa_framerows_last(None, C.byref(st)) == bad and lib.sa_framerows_last(None, None) == bad
    assert lib.sa_associate_dev(None, 0, 0, C.byref(det), C.byref(rows), None, None) == bad
    assert lib.sa_batch_add_dev(None, 0, 0, C.byref(det), C.byref(rows), None) == bad
    assert lib.sa_batch_add_deferred_dev(None, 0, 0, C.byref(det), C.byref(rows), None) == bad
    assert lib.sa_associate_batch_dev(None, 0, None, rp, None) == bad
    assert lib.sa_pipe_stage_dev(None, 0, None, rp, C.byref(t)) == bad
    assert lib.sa_pipe_submit_dev(None, 0, None, rp, C.byref(t)) == bad
    assert lib.sa_tracker_predict_dev(None, 0, 0, None, C.byref(rows), None) == bad
    assert lib.sa_tracker_predict_batch_begin_dev(None, 0, None, None, None, rp, C.byref(h)) == bad


def test_the_header_and_the_source_are_part_of_the_build():
    assert "sa_framerows.hip" in build.SOURCES
    assert HEADER in build.HEADERS
    src = (build.CSRC / "sa_framerows.hip").read_text()
    assert "k_widen_rows" in src and '#include "sa_widen.h"' in src
    # widen itself is written once, in the header the pad kernel of the track search reads it from too
    assert "widen16" in (build.CSRC / "sa_widen.h").read_text() and '#include "sa_widen.h"' in (build.CSRC / "sa_devrows.hip").read_text()
    assert '#include "../../include/similari_framerows.h"' in (build.CSRC / "sa_framerows.h").read_text()
