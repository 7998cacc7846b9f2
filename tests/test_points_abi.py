"""The point bank as a library boundary: include/similari_points.h adds fourteen calls and three structs beside those of
similari_devrows.h and similari_framerows.h, the library exports them, similari_amd.points binds exactly that, and the kernel runs the
arithmetic of sa_kalman_point.h, the file the host tests compile."""
import ctypes as C
import re
from pathlib import Path

import pytest

from similari_amd import abi, absorb, attrs, bestfit, bf16, build, consolidate, devrows, f16, framerows, gallery, handover, i8, merge, points, retain, search, waste

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "similari_points.h"
DECL = re.compile(r"^\s*(?:const\s+)?(?:int|void|uint32_t|uint64_t|double|const char\s*\*)\s*\*?\s*(sa_[a-z0-9_]+)\s*\(", re.M)
NAMES = sorted(["sa_points_options_default", "sa_points_create", "sa_points_destroy", "sa_points_initiate", "sa_points_predict", "sa_points_update",
                "sa_points_distance", "sa_points_step", "sa_points_remove", "sa_points_count", "sa_points_order", "sa_points_get_state",
                "sa_points_set_state", "sa_points_last"])
EARLIER = ("similari_assoc.h", "similari_tracker.h", "similari_search.h", "similari_gallery.h", "similari_merge.h", "similari_attrs.h",
           "similari_bestfit.h", "similari_bf16.h", "similari_f16.h", "similari_devrows.h", "similari_absorb.h", "similari_retain.h",
           "similari_i8.h", "similari_framerows.h", "similari_handover.h", "similari_consolidate.h", "similari_waste.h", "similari_frames.h")


def declared(header=HEADER):
    text = re.sub(r"/\*.*?\*/", "", Path(header).read_text(), flags=re.S)
    return sorted(set(DECL.findall(text)))


@pytest.fixture(scope="module")
def lib():
    return points.load_library(build.build_lib())


def test_the_header_declares_exactly_the_calls():
    assert declared() == NAMES
    text = HEADER.read_text()
    assert '#include "similari_devrows.h"' in text and '#include "similari_framerows.h"' in text
    assert re.search(r"typedef struct sa_points_options \{.*?\} sa_points_options; /\* 16 B \*/", text, flags=re.S)
    assert re.search(r"typedef struct sa_point_rows \{.*?\} sa_point_rows; /\* 40 B \*/", text, flags=re.S)
    assert re.search(r"typedef struct sa_points_stats \{.*?\} sa_points_stats; /\* 64 B \*/", text, flags=re.S)
    for k, v in (("SA_POINT_D2", 0), ("SA_POINT_COST", 1), ("SA_POINT_COST_INVERTED", 2)):
        assert re.search(rf"#define {k} {v}u\b", text), k
    for h in EARLIER:
        assert not [n for n in declared(ROOT / "include" / h) if n.startswith("sa_point")], h


def test_the_library_exports_them(lib):
    """Fails on a library built before the point bank."""
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_the_binding_is_the_header():
    assert set(points.PROTOTYPES) == set(declared())
    for other in (abi, search, gallery, merge, attrs, bestfit, bf16, f16, devrows, framerows, absorb, retain, i8, handover, consolidate, waste):
        assert not set(points.PROTOTYPES) & set(other.PROTOTYPES), other.__name__
    for f in ("initiate", "predict", "update", "distance", "step", "remove", "order", "state", "set_state", "last", "close"):
        assert callable(getattr(points.PointBank, f)), f
    assert callable(points.bind) and callable(points.load_library)
    assert (points.SA_POINT_D2, points.SA_POINT_COST, points.SA_POINT_COST_INVERTED) == (0, 1, 2)
    assert points.SA_ROW_NONE == framerows.SA_ROW_NONE if hasattr(framerows, "SA_ROW_NONE") else points.SA_ROW_NONE == 0xFFFFFFFF


def fields_of(struct):
    body = re.search(r"typedef struct %s \{(.*?)\}" % struct, HEADER.read_text(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            decl = re.sub(r"^(const\s+)?\w+\s*\*?\s*", "", decl, count=1)
            names += [n.strip().lstrip("*").strip() for n in decl.split(",")]
    return names


def test_the_structs_as_the_header_lays_them_out():
    o, r, s = points.sa_points_options, points.sa_point_rows, points.sa_points_stats
    assert (C.sizeof(o), C.sizeof(r), C.sizeof(s)) == (16, 40, 64)
    off = lambda st: {f: getattr(st, f).offset for f, _ in st._fields_}   # noqa: E731
    assert off(o) == {"struct_size": 0, "points": 4, "position_weight": 8, "velocity_weight": 12}
    assert off(r) == {"struct_size": 0, "comps": 4, "min_score": 8, "reserved": 12, "host": 16, "present": 24, "dev": 32}
    assert off(s) == {"struct_size": 0, "tracks": 4, "launches": 8, "capacity": 12, "points": 16, "present": 24, "bytes_h2d": 32,
                      "bytes_d2h": 40, "src_bytes": 48, "device_ms": 56}
    for name, st in (("sa_points_options", o), ("sa_point_rows", r), ("sa_points_stats", s)):
        assert fields_of(name) == [f for f, _ in st._fields_], name


def test_the_defaults(lib):
    o = points.sa_points_options()
    lib.sa_points_options_default(C.byref(o))
    assert o.struct_size == 16 and o.points == 17
    import numpy as np

    assert np.float32(o.position_weight) == np.float32(1) / np.float32(20) and np.float32(o.velocity_weight) == np.float32(1) / np.float32(160)
    lib.sa_points_options_default(None)


def test_bind_attaches_the_prototypes():
    fresh = C.CDLL(str(build.build_lib()))
    assert fresh.sa_points_step.argtypes is None
    points.bind(fresh)
    for name, (res, args) in points.PROTOTYPES.items():
        fn = getattr(fresh, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert fresh.sa_store_search_dev.argtypes is not None and fresh.sa_associate_dev.argtypes is not None   # the two headers it includes


def test_null_handles_are_refused(lib):
    """No engine and no bank can exist without a device, so what runs here is what the calls answer to null handles."""
    ids = (C.c_uint64 * 1)(5)
    xy = (C.c_float * 34)()
    rows = points.sa_point_rows(40, 2, 0.0, 0, xy, None, None)
    B = abi.SA_ERR_BAD_ARG
    assert lib.sa_points_initiate(None, 1, ids, C.byref(rows)) == B
    assert lib.sa_points_predict(None, 1, ids, xy) == B and lib.sa_points_predict(None, 0, None, None) == B
    assert lib.sa_points_update(None, 1, ids, C.byref(rows), xy) == B
    assert lib.sa_points_distance(None, 1, ids, C.byref(rows), 0, xy) == B
    assert lib.sa_points_step(None, 1, ids, C.byref(rows), xy) == B
    assert lib.sa_points_remove(None, 1, ids) == B
    n = C.c_uint32(7)
    assert lib.sa_points_count(None, C.byref(n)) == B and lib.sa_points_order(None, ids, 1, C.byref(n)) == B and n.value == 7
    assert lib.sa_points_get_state(None, 5, None, None, None) == B and lib.sa_points_set_state(None, 5, None, None, None) == B
    st = points.sa_points_stats()
    st.tracks = 7
    assert lib.sa_points_last(None, C.byref(st)) == B and st.tracks == 7
    lib.sa_points_destroy(None)


def test_no_bank_without_a_device(lib):
    import os

    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is visible: tests/test_gpu_points.py creates banks")
    o = points.sa_points_options()
    lib.sa_points_options_default(C.byref(o))
    h = points.POINTS()
    assert lib.sa_points_create(None, C.byref(o), C.byref(h)) == abi.SA_ERR_NO_DEVICE and not h.value
    assert b"no CPU fallback" in lib.sa_last_error(None)


def test_the_header_and_the_source_are_part_of_the_build():
    assert "sa_points.hip" in build.SOURCES
    assert HEADER in build.HEADERS and build.CSRC / "sa_kalman_point.h" in build.HEADERS
    src = (build.CSRC / "sa_points.hip").read_text()
    for k in ('#include "sa_kalman_point.h"', "sa_point_at<SRC>", "sa_point_rows_stage", "sa_pkf_step", "sa_pkf_distance", "k_points_move"):
        assert k in src, k
    assert "__shared__" not in src and "atomic" not in src   # no LDS; values are written with plain stores
    # the read of a point, the check of the rows and the choice of the source type are sa_point_rows.h's, shared with the vote and pose NMS
    assert build.CSRC / "sa_point_rows.h" in build.HEADERS and '#include "sa_point_rows.h"' in (build.CSRC / "sa_points_impl.h").read_text()
    rows = (build.CSRC / "sa_point_rows.h").read_text()
    for k in ('#include "sa_widen.h"', "load_elem<SRC>", "sa_point_present(", "sa_dev_rows_layout", "sa_dev_rows_span"):
        assert k in rows, k
    assert src.count("hipLaunchKernelGGL(k_points<") == 1 and "sa_point_elem(elem" in src   # one launch site, instantiated per source type
    for elem in ("SA_ELEM_F16", "SA_ELEM_BF16", "SA_ELEM_F32"):
        assert rows.count("std::integral_constant<int, %s>{}" % elem) == 1, elem   # ... of which a call takes one
    kal = (build.CSRC / "sa_kalman_point.h").read_text()
    assert "fma" not in kal.lower() and "SA_HD" in kal
    emu = (ROOT / "tests" / "emu_points" / "emu_points.cpp").read_text()
    assert '#include "../../similari_amd/csrc/sa_kalman_point.h"' in emu
    assert "-ffp-contract=off" in build.FLAGS
