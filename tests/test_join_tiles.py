"""Which tiles the join's first launch runs (similari_amd/csrc/sa_join_tiles.h), walked on the host: the header is compiled with the
host compiler and every workgroup index of every grid up to 300 tile rows is decoded, in both tile shapes (64 x 64: a triangle;
32 x 128: a staircase)."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "similari_amd" / "csrc"
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sa_join_tiles.h"
// walk BM BN Rmax: per R = 1..Rmax one line "R count rect wanted visited bad"
//   wanted: tiles (i, j) of the R x C grid with n0 + BN > m0; visited: distinct ones of them the decode reached;
//   bad: indices decoded outside the grid, onto a tile below the diagonal, or onto a tile reached before
// at BM BN idx R: "i j" of one index
int main(int argc, char** argv) {
  if (argc == 5 && argv[1][0] == 'w') {
    const uint32_t BM = std::strtoul(argv[2], 0, 10), BN = std::strtoul(argv[3], 0, 10), Rmax = std::strtoul(argv[4], 0, 10), r = BN / BM;
    for (uint32_t R = 1; R <= Rmax; ++R) {
      const uint32_t C = (R + r - 1) / r;
      unsigned long long wanted = 0, visited = 0, bad = 0;
      for (uint32_t i = 0; i < R; ++i)
        for (uint32_t j = 0; j < C; ++j) wanted += (unsigned long long)j * BN + BN > (unsigned long long)i * BM;
      std::vector<char> seen((size_t)R * C, 0);
      const unsigned long long n = sa_join_tile_count(R, r);
      for (unsigned long long x = 0; x < n; ++x) {
        uint32_t i, j;
        sa_join_tile_decode(x, r, &i, &j);
        if (i >= R || j >= C || !((unsigned long long)j * BN + BN > (unsigned long long)i * BM) || seen[(size_t)i * C + j]) { ++bad; continue; }
        seen[(size_t)i * C + j] = 1;
        ++visited;
      }
      std::printf("%u %llu %llu %llu %llu %llu\n", R, n, (unsigned long long)sa_join_tile_rect(R, r), wanted, visited, bad);
    }
    return 0;
  }
  if (argc == 6 && argv[1][0] == 'a') {
    const uint32_t BM = std::strtoul(argv[2], 0, 10), BN = std::strtoul(argv[3], 0, 10);
    uint32_t i, j;
    sa_join_tile_decode(std::strtoull(argv[4], 0, 10), BN / BM, &i, &j);
    std::printf("%u %u %llu\n", i, j, (unsigned long long)sa_join_tile_count((uint32_t)std::strtoul(argv[5], 0, 10), BN / BM));
    return 0;
  }
  if (argc == 3 && argv[1][0] == 'g') {   // grid tiles: "gx gy first last" — the index of the grid's first and last workgroup
    const unsigned long long tiles = std::strtoull(argv[2], 0, 10);
    uint32_t gx, gy;
    sa_join_grid(tiles, &gx, &gy);
    std::printf("%u %u %llu %llu\n", gx, gy, (unsigned long long)sa_join_grid_index(0, 0, gx),
                (unsigned long long)sa_join_grid_index(gx - 1, gy - 1, gx));
    return 0;
  }
  return 2;
}
"""
SHAPES = [(64, 64), (32, 128)]


def closed_form(R, r):
    C = -(-R // r)
    return r * C * (C - 1) // 2 + R


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("join_tiles")
    (d / "drv.cpp").write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", str(CSRC), str(d / "drv.cpp"), "-o", str(d / "drv")], check=True)

    def run(*args):
        out = subprocess.run([str(d / "drv"), *[str(a) for a in args]], capture_output=True, text=True, check=True).stdout
        return [[int(x) for x in line.split()] for line in out.splitlines()]

    return run


@pytest.mark.parametrize("bm,bn", SHAPES)
def test_every_tile_on_or_above_the_diagonal_once_and_no_other(drv, bm, bn):
    lines = drv("walk", bm, bn, 300)
    assert [l[0] for l in lines] == list(range(1, 301))
    r = bn // bm
    for R, count, rect, wanted, visited, bad in lines:
        assert bad == 0, (R, bad)
        assert count == wanted == visited == closed_form(R, r), (R, count, wanted, visited)
        assert rect == R * -(-R // r)
        assert count < rect or R <= r


@pytest.mark.parametrize("bm,bn", SHAPES)
def test_first_and_last_indices_at_the_largest_extents(drv, bm, bn):
    rows = 65535 * 32                      # SA_SEARCH_MAX_QUERY_SLOTS: the most observation slots a join can have
    R, r = -(-rows // bm), bn // bm
    C = -(-R // r)
    n = closed_form(R, r)
    threads = 256 if bm == 64 else 512
    assert n * threads >= 2**32            # more work-items than one grid dimension of a dispatch holds: the grid is two-dimensional
    (gx, gy, first, last), = drv("grid", n)
    assert gx * threads < 2**32 and gy <= 65535
    assert first == 0 and n - 1 <= last < n - 1 + gx   # every tile has its workgroup; fewer than one grid row of them is spare
    assert drv("at", bm, bn, 0, R) == [[0, 0, n]]
    assert drv("at", bm, bn, n - 1, R) == [[R - 1, C - 1, n]]
    first_of_last = r * C * (C - 1) // 2
    assert drv("at", bm, bn, first_of_last, R) == [[0, C - 1, n]]
    assert drv("at", bm, bn, first_of_last - 1, R) == [[(C - 1) * r - 1, C - 2, n]]


def test_the_triangle_is_a_triangle():
    assert [closed_form(R, 1) for R in (1, 2, 3, 4)] == [1, 3, 6, 10]
    # 32 x 128: column j runs its first 4 (j + 1) row tiles, the last column all R of them
    assert [closed_form(R, 4) for R in (1, 4, 5, 8, 9)] == [1, 4, 4 + 5, 4 + 8, 4 + 8 + 9]


@pytest.mark.parametrize("tiles", [1, 2, 65535, 65536, 65537, 2**24 - 1, 2**24, 2**24 + 1, 2**29, 536_903_679])
def test_the_grid_holds_every_tile_within_one_dispatch(drv, tiles):
    """gx * gy workgroups cover the tiles with less than one grid row to spare, and neither dimension exceeds what a dispatch takes
    with 512 threads per workgroup (fewer than 2^32 work-items per dimension; y kept within 65535 as the search grids are)."""
    (gx, gy, first, last), = drv("grid", tiles)
    assert 1 <= gx <= 65536 and gx * 512 < 2**32 and 1 <= gy <= 65535
    assert gx * gy >= tiles > gx * (gy - 1)
    assert first == 0 and last == gx * gy - 1
