"""similari_amd/csrc/sa_slot_out.h, the one home of a slot's result block (ids | votes | stats | winning columns | completion word): its
offsets against the expressions the engine's readers used to spell out, and the properties the block's users rely on.  Host only: a
driver compiled with the host compiler."""
import shutil
import subprocess

import pytest

from similari_amd import build

COUNTS = [0, 1, 7, 8, 9, 63, 64, 65, 1000, 4096]

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sa_slot_out.h"
// argv: counts  ->  per count: n ids votes stats cols done bytes, then the same offsets through a View over a base of 4096, then gave_up
// of a block whose STAT_GAVE_UP word is set
int main(int argc, char** argv) {
  using namespace sa_slot_out;
  for (int k = 1; k < argc; ++k) {
    const size_t n = (size_t)strtoull(argv[k], nullptr, 10);
    std::vector<uint64_t> block(bytes(n) / 8 + 1, 0);
    View v(block.data(), n);
    uint8_t* b = (uint8_t*)block.data();
    v.stats()[STAT_GAVE_UP] = 1;
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d\n", n, ids_off(n), votes_off(n), stats_off(n), cols_off(n), done_off(n), bytes(n),
           (size_t)((uint8_t*)v.ids() - b), (size_t)(v.votes() - b), (size_t)((uint8_t*)v.stats() - b), (size_t)((uint8_t*)v.cols() - b),
           (int)v.gave_up(), (int)STAT_EUCLID_ILL, (int)STAT_GAVE_UP, (int)STAT_LEFTOVER);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("slot_out")
    (d / "drv.cpp").write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", str(build.CSRC), str(d / "drv.cpp"), "-o", str(d / "drv")], check=True)
    out = subprocess.run([str(d / "drv")] + [str(n) for n in COUNTS], capture_output=True, text=True, check=True).stdout
    res = [[int(x) for x in line.split()] for line in out.splitlines()]
    assert [r[0] for r in res] == COUNTS
    return res


def test_offsets_equal_the_expressions_they_replace(rows):
    for n, ids, votes, stats, cols, done, size, *_ in rows:
        assert ids == 0
        assert votes == (n if n else 1) * 8
        assert stats == ((n if n else 1) * 9 + 7) & ~7
        assert cols == (((n if n else 1) * 9 + 7) & ~7) + 16
        assert done == ((n * 13 + 48 + 127) & ~127)
        assert size == done + 128


def test_regions_do_not_overlap_and_are_aligned(rows):
    for n, ids, votes, stats, cols, done, size, *_ in rows:
        n1 = max(n, 1)
        assert ids + 8 * n1 <= votes
        assert votes + n1 <= stats
        assert stats + 16 <= cols
        assert stats % 8 == 0 and cols % 4 == 0
        # the completion word: a 128-byte line of its own past the end of the columns, inside the block
        assert done % 128 == 0 and cols + 4 * n1 <= done and done + 8 <= size


def test_the_view_uses_the_same_offsets(rows):
    for n, ids, votes, stats, cols, done, size, v_ids, v_votes, v_stats, v_cols, gave_up, *_ in rows:
        assert (v_ids, v_votes, v_stats, v_cols) == (ids, votes, stats, cols)
        assert gave_up == (1 if n else 0)      # an empty frame runs no tail: its mark is not looked at


def test_stats_words(rows):
    assert rows[0][-3:] == [0, 1, 2]
