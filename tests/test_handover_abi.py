"""The hand-over as a library boundary: include/similari_handover.h adds five calls and one stats struct beside those of
similari_search.h .. similari_i8.h, the library exports them, similari_amd.handover binds exactly that, and the removal they share
plans its moves with sa_merge_compaction (similari_amd/csrc/sa_merge_plan.h), which is held here against a sequential removal."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from similari_amd import abi, absorb, attrs, bestfit, bf16, build, devrows, f16, gallery, handover, i8, merge, retain, search

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "similari_handover.h"
DECL = re.compile(r"^\s*(?:const\s+)?(?:int|void|uint32_t|uint64_t|double|const char\s*\*)\s*\*?\s*(sa_[a-z0-9_]+)\s*\(", re.M)
NAMES = ["sa_store_hand_over", "sa_store_handover_last", "sa_store_ready", "sa_store_take"]
EARLIER = ("similari_assoc.h", "similari_tracker.h", "similari_search.h", "similari_gallery.h", "similari_merge.h", "similari_attrs.h",
           "similari_bestfit.h", "similari_bf16.h", "similari_f16.h", "similari_devrows.h", "similari_absorb.h", "similari_retain.h",
           "similari_i8.h", "similari_framerows.h")


def declared(header=HEADER):
    text = re.sub(r"/\*.*?\*/", "", Path(header).read_text(), flags=re.S)
    return sorted(set(DECL.findall(text)))


@pytest.fixture(scope="module")
def lib():
    return handover.load_library(build.build_lib())


def test_the_header_declares_the_calls_and_the_stats():
    """Four functions and the struct of the fifth declaration; nothing of it went into a header that was there before."""
    assert declared() == NAMES
    text = HEADER.read_text()
    assert '#include "similari_i8.h"' in text
    assert re.search(r"typedef struct sa_handover_stats \{.*?\} sa_handover_stats;", text, flags=re.S)
    for h in EARLIER:
        assert not [n for n in declared(ROOT / "include" / h) if n in NAMES], h
        assert "sa_handover_stats" not in (ROOT / "include" / h).read_text(), h


def test_the_library_exports_them(lib):
    """Fails on a library built before the hand-over."""
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_the_binding_is_the_header():
    assert set(handover.PROTOTYPES) == set(declared())
    for other in (abi, search, gallery, merge, attrs, bestfit, bf16, f16, devrows, absorb, retain, i8):
        assert not set(handover.PROTOTYPES) & set(other.PROTOTYPES), other.__name__
    for f in ("ready", "take", "hand_over", "last"):
        assert callable(getattr(handover, f))
    # the struct as the header lays it out: four u32, three u64, two doubles
    assert C.sizeof(handover.sa_handover_stats) == 56
    fields = re.search(r"typedef struct sa_handover_stats \{(.*?)\}", HEADER.read_text(), flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f for f, _ in handover.sa_handover_stats._fields_]
    # the tail of sa_store_hand_over is the tail of the absorb calls without the rows, attributes and qualities
    assert handover.PROTOTYPES["sa_store_hand_over"][1][-6:] == absorb._TAIL[2:]


def test_bind_attaches_the_prototypes():
    fresh = C.CDLL(str(build.build_lib()))
    assert fresh.sa_store_hand_over.argtypes is None
    handover.bind(fresh)
    for name, (res, args) in handover.PROTOTYPES.items():
        fn = getattr(fresh, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert fresh.sa_store_create_i8.argtypes is not None   # and everything below it (similari_i8.h ..)


def test_null_stores_are_refused_and_the_struct_size_is_written(lib):
    """No store can exist without a device, so what runs here is what every call answers to a null handle — and that the stats call
    refuses one too rather than writing through it."""
    n = C.c_uint32(7)
    ids = np.array([1], np.uint64)
    p = ids.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib.sa_store_ready(None, 0, None, 0, C.byref(n)) == abi.SA_ERR_BAD_ARG and n.value == 7
    assert lib.sa_store_take(None, 1, p, None, None, None, None) == abi.SA_ERR_BAD_ARG
    assert lib.sa_store_hand_over(None, None, 0, None, None, 1, p, None, None, None, None, None, None) == abi.SA_ERR_BAD_ARG
    st = handover.sa_handover_stats()
    assert lib.sa_store_handover_last(None, C.byref(st)) == abi.SA_ERR_BAD_ARG and st.struct_size == 0
    text = (build.CSRC / "sa_handover.hip").read_text()
    assert "out->struct_size = sizeof *out;" in text   # (tests/test_gpu_handover.py reads it back from a live store)


def test_the_header_and_the_source_are_part_of_the_build():
    assert "sa_handover.hip" in build.SOURCES
    assert HEADER in build.HEADERS
    assert '#include "../../include/similari_handover.h"' in (build.CSRC / "sa_store.h").read_text()
    src = (build.CSRC / "sa_handover.hip").read_text()
    assert "k_handover_rows" in src and "sa_merge_compaction" in src and "sa_store_launch_compact" in src
    assert "sa_devrows_pad_own" in (build.CSRC / "sa_devrows.hip").read_text()
    assert "sa_in_device_block" not in src   # the library's own banks are not registered blocks; sa_devrows_check stays the public gate
    search_text = (build.CSRC / "sa_search.hip").read_text()
    remove = search_text[search_text.index("int sa_store_remove("): search_text.index("int sa_store_count(")]
    assert "sa_store_remove_slots" in remove and "hipMemcpyAsync" not in remove   # one launch, not two copies per id


# ---- the planned moves of a removal against sequential last-into-hole ---------------------------
DRIVER = r"""
#include <cstdio>
#include <iostream>
#include "sa_merge_plan.h"
// stdin, one case per line: T n removed{n}  ->  nperm perm{nperm} nmoves (from to){nmoves}
int main() {
  uint32_t T, n;
  while (std::cin >> T >> n) {
    std::vector<uint32_t> removed(n), perm;
    for (auto& r : removed) std::cin >> r;
    std::vector<SaMergeMove> moves;
    sa_merge_compaction(T, removed, perm, moves);
    std::printf("%zu", perm.size());
    for (uint32_t p : perm) std::printf(" %u", p);
    std::printf(" %zu", moves.size());
    for (const auto& m : moves) std::printf(" %u %u", m.from, m.to);
    std::printf("\n");
  }
  return 0;
}
"""


def sequential_remove(T, removed):
    """sa_store_remove one id at a time: the last track moves into the hole.  -> final slot -> original slot"""
    at = list(range(T))
    for o in removed:
        p = at.index(o)
        at[p] = at[-1]
        at.pop()
    return at


def removed_sets(T):
    """The sets of the issue, each in ascending and in descending call order."""
    sets = [[], [T - 1], [0], list(range(T)), list(range(0, T, 2)), [T - 3, T - 2, T - 1, T // 2]]
    return sets + [s[::-1] for s in sets if len(s) > 1]


def test_planned_moves_reproduce_sequential_removal(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    (tmp_path / "drv.cpp").write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", str(build.CSRC), str(tmp_path / "drv.cpp"), "-o", str(tmp_path / "drv")],
                   check=True)
    cases = [(T, rem) for T in (7, 70) for rem in removed_sets(T)]
    lines = [" ".join([str(T), str(len(rem))] + [str(r) for r in rem]) for T, rem in cases]
    out = subprocess.run([str(tmp_path / "drv")], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    res = [[int(x) for x in line.split()] for line in out.splitlines()]
    assert len(res) == len(cases)
    for (T, rem), o in zip(cases, res):
        n = o[0]
        perm, nm = o[1: 1 + n], o[1 + n]
        moves = np.array(o[2 + n:], np.int64).reshape(nm, 2)
        assert n == T - len(rem) and perm == sequential_remove(T, rem), (T, rem)
        # applied in one go to the table as it stood: every move reads a slot that no move writes
        table = list(range(T))
        after = list(table)
        for frm, to in moves.tolist():
            after[to] = table[frm]
        assert after[:n] == perm, (T, rem)
        assert np.all(moves[:, 0] >= n) and np.all(moves[:, 1] < n) and len(set(moves[:, 0].tolist())) == nm
