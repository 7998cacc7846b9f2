"""Rows from device memory as a library boundary: include/similari_devrows.h declares four functions beside those of
similari_search.h .. similari_f16.h, the library exports them, and similari_amd.devrows binds exactly that."""
import ctypes as C
import re
from pathlib import Path

import pytest

from similari_amd import abi, attrs, bestfit, bf16, build, devrows, f16, gallery, merge, search

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "similari_devrows.h"
DECL = re.compile(r"^\s*(?:const\s+)?(?:int|void|uint32_t|uint64_t|double|const char\s*\*)\s*\*?\s*(sa_[a-z0-9_]+)\s*\(", re.M)
NAMES = ["sa_store_append_dev", "sa_store_devrows_last", "sa_store_search_dev", "sa_store_upsert_dev"]
EARLIER = ("similari_assoc.h", "similari_tracker.h", "similari_search.h", "similari_gallery.h", "similari_merge.h", "similari_attrs.h",
           "similari_bestfit.h", "similari_bf16.h", "similari_f16.h")


def declared(header=HEADER):
    text = re.sub(r"/\*.*?\*/", "", Path(header).read_text(), flags=re.S)
    return sorted(set(DECL.findall(text)))


@pytest.fixture(scope="module")
def lib():
    return devrows.load_library(build.build_lib())


def test_the_header_declares_exactly_the_four_functions():
    assert declared() == NAMES
    text = HEADER.read_text()
    assert '#include "similari_f16.h"' in text
    assert re.search(r"#define SA_VOTE_TOPN\s+0u?\b", text) and re.search(r"#define SA_VOTE_BESTFIT\s+1u?\b", text)
    assert (devrows.SA_VOTE_TOPN, devrows.SA_VOTE_BESTFIT) == (0, 1)
    for h in EARLIER:   # nothing of it went into a header that was there before
        code = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / h).read_text(), flags=re.S)
        assert not [n for n in declared(ROOT / "include" / h) if n in NAMES], h
        for word in ("sa_dev_rows", "sa_devrows_stats", "SA_VOTE_TOPN", "SA_VOTE_BESTFIT", "similari_devrows.h"):
            assert word not in code, (h, word)


def test_every_declared_function_is_exported(lib):
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_the_binding_is_the_header():
    assert set(devrows.PROTOTYPES) == set(declared())
    for other in (abi, search, gallery, merge, attrs, bestfit, bf16, f16):
        assert not set(devrows.PROTOTYPES) & set(other.PROTOTYPES), other.__name__
    assert issubclass(devrows.DeviceRowsStore, f16.F16Store)
    for name in ("upsert_rows", "append_rows", "search_rows", "search_rows_raw", "devrows_stats"):
        assert callable(getattr(devrows.DeviceRowsStore, name)), name
    assert callable(devrows.DeviceRows.from_tensor) and callable(devrows.register_tensor)
    assert "import torch" not in (ROOT / "similari_amd" / "devrows.py").read_text()


def test_struct_layout():
    r = devrows.sa_dev_rows
    assert C.sizeof(r) == 40
    assert (r.struct_size.offset, r.elem.offset, r.base.offset, r.n_rows.offset, r.row_stride.offset, r.index.offset) == (0, 4, 8, 16, 24, 32)
    st = devrows.sa_devrows_stats
    assert C.sizeof(st) == 32
    assert (st.struct_size.offset, st.reserved.offset, st.rows.offset, st.wide_rows.offset, st.src_bytes.offset) == (0, 4, 8, 16, 24)
    text = HEADER.read_text()
    assert "sizeof(sa_dev_rows) = 40" in text and re.search(r"sa_devrows_stats;\s*/\* 32 B \*/", text)


def test_the_descriptor_from_a_strided_tensor():
    class T:   # what from_tensor reads of a tensor: a column slice t[:, 4:4 + 5] of a [7][16] fp16 tensor
        dtype, shape = "torch.float16", (7, 5)

        def data_ptr(self):
            return 0x7000 + 8

        def stride(self):
            return (16, 1)

    d = devrows.DeviceRows.from_tensor(T(), index=[3, 0, 3])
    assert (d.ptr, d.n_rows, d.row_stride, d.elem) == (0x7008, 7, 16, f16.SA_ELEM_F16)
    st = d.struct()
    assert (st.struct_size, st.elem, st.base, st.n_rows, st.row_stride) == (40, 2, 0x7008, 7, 16)
    assert [st.index[i] for i in range(3)] == [3, 0, 3]
    T.dtype = "torch.int8"
    with pytest.raises(TypeError):
        devrows.DeviceRows.from_tensor(T())


def test_null_handles_are_refused(lib):
    st = devrows.sa_devrows_stats()
    rows = devrows.sa_dev_rows()
    assert lib.sa_store_devrows_last(None, C.byref(st)) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_devrows_last(None, None) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_upsert_dev(None, 0, None, None, C.byref(rows)) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_append_dev(None, 0, 0, None, None, C.byref(rows), None, None) == abi.SA_ERR_BAD_ARG
    prm = search.sa_topn_params(1, 1, 1.0, 1.0)
    assert lib.sa_store_search_dev(None, C.byref(prm), 0, None, 0, None, None, C.byref(rows), None, None, None, None, None, None) == abi.SA_ERR_BAD_ARG


def test_the_header_and_the_source_are_part_of_the_build():
    assert "sa_devrows.hip" in build.SOURCES
    assert HEADER in build.HEADERS
    assert '#include "../../include/similari_devrows.h"' in (build.CSRC / "sa_store.h").read_text()
    src = (build.CSRC / "sa_devrows.hip").read_text()
    assert "k_pad_rows" in src and "sa_in_device_block" in src
    assert "sa_in_device_block" in (build.CSRC / "sa_engine.hip").read_text()
