"""The extents a track search can index (similari_amd/csrc/sa_search_limits.h), probed at their edges on the host: the header is compiled
with the host compiler and asked the same question sa_store_upsert / sa_store_search_topn ask before they touch the device."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "similari_amd" / "csrc"
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "sa_search_limits.h"
int main(int argc, char** argv) {
  if (argc == 1) {
    std::printf("%llu %llu %llu %u\n", (unsigned long long)SA_STORE_MAX_SLOTS, (unsigned long long)SA_SEARCH_MAX_QUERY_SLOTS,
                (unsigned long long)SA_SEARCH_MAX_PAIRS, (unsigned)SA_STORE_MAX_FEATURE_LEN);
    return 0;
  }
  for (int i = 1; i + 3 < argc; i += 4)
    std::printf("%d\n", sa_search_extent(std::strtoull(argv[i], 0, 10), std::strtoull(argv[i + 1], 0, 10), (uint32_t)std::strtoul(argv[i + 2], 0, 10),
                                         (uint32_t)std::strtoul(argv[i + 3], 0, 10)));
  return 0;
}
"""
OK, FEATURE_LEN, STORED, QUERIES, PAIRS = range(5)


@pytest.fixture(scope="module")
def extent(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("limits")
    (d / "drv.cpp").write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", str(CSRC), str(d / "drv.cpp"), "-o", str(d / "drv")], check=True)

    def ask(*shapes):
        args = [str(v) for shape in shapes for v in shape]
        out = subprocess.run([str(d / "drv"), *args], capture_output=True, text=True, check=True).stdout.split()
        return [int(x) for x in out]

    ask.limits = [int(x) for x in subprocess.run([str(d / "drv")], capture_output=True, text=True, check=True).stdout.split()]
    return ask


def test_every_accepted_shape_keeps_the_kernels_indices_in_range(extent):
    max_slots, max_query_slots, max_pairs, max_d = extent.limits
    dp = (max_d + 31) // 32 * 32
    assert 64 * dp < 2**32                   # a cosine tile's own offsets (row * Dp + k, 64 rows) in gemm_mainloop's 32 bits
    assert max_slots < 2**31                 # T * Kp: column numbers and T << lgK in 32 bits
    assert -(-max_query_slots // 32) <= 65535 and -(-max_query_slots // 64) <= 65535   # grid y of both tiles
    assert max_pairs < 2**32 - 1             # pool blocks below the no-group mark


def test_a_gallery_of_sixteen_gigabytes_and_more_is_a_valid_store(extent):
    """262 145 tracks x 32 observations x 512-d = 2^32 floats and more: addressed with 64-bit tile bases, accepted."""
    assert extent((262145, 0, 32, 512), (1 << 20, 64, 32, 512), (1 << 22, 0, 32, 4096)) == [OK, OK, OK]


@pytest.mark.parametrize("kp", [1, 2, 4, 8, 16, 32])
def test_stored_slots_edge(extent, kp):
    n = (2**31 - 1) // kp
    assert extent((n, 0, kp, 64), (n + 1, 0, kp, 64)) == [OK, STORED]


@pytest.mark.parametrize("kp", [1, 4, 32])
def test_query_slots_edge(extent, kp):
    n = 65535 * 32 // kp
    assert extent((10, n, kp, 64), (10, n + 1, kp, 64)) == [OK, QUERIES]


def test_pairs_and_feature_len_edges(extent):
    assert extent((2**31 - 1, 2, 1, 8), (2**31 - 1, 3, 1, 8)) == [OK, PAIRS]
    assert extent((1, 1, 1, 2**24), (1, 1, 1, 2**24 + 1)) == [OK, FEATURE_LEN]
    assert extent((2**40, 0, 1, 8), (2**33, 1, 1, 8)) == [STORED, STORED]   # no wrap in the products
