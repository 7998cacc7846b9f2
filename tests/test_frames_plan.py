"""The plan of an NMS or own-area call (similari_amd/csrc/sa_frames_plan.h) — of the scenes of sa_own_areas_batch / sa_nms_batch and
of the one scene of sa_own_areas / sa_nms — on the host: the header is compiled with the host compiler behind a small driver, and
its segment table, launch shape and refusals are compared with the same arithmetic written out here."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "similari_amd" / "csrc"
FITS, TOO_MANY_SCENES, SCENE_TOO_LARGE, TOO_MANY_ROWS = 0, 1, 2, 3
DRIVER = r"""
#include <cstdio>
#include <iostream>
#include <string>
#include "sa_frames_plan.h"
// stdin, one case per line:
//   P nms n counts{n}   ->  refusal bad_scene total max_count max_W sweep_S mask_words n (first count W mask_off){n}
//   R nms n value       ->  the same for n scenes of `value` boxes each, without the table (n may be large)
//   S spilled           ->  launches of the spill path
int main() {
  static_assert(sizeof(SaFrameSeg) == 24, "the device reads this layout");
  std::string tag;
  while (std::cin >> tag) {
    if (tag == "P" || tag == "R") {
      uint32_t nms, n;
      std::cin >> nms >> n;
      std::vector<uint32_t> counts(n);
      if (tag == "P") for (auto& c : counts) std::cin >> c;
      else { uint32_t v; std::cin >> v; for (auto& c : counts) c = v; }
      SaFramesPlan p;
      uint32_t bad = 77;
      const int r = (int)sa_frames_plan(n, counts.data(), nms != 0, &p, &bad);
      std::printf("%d %u %u %u %u %u %llu", r, bad, p.total, p.max_count, p.max_W, p.sweep_S, (unsigned long long)p.mask_words);
      if (tag == "P" && r == 0) {
        std::printf(" %zu", p.segs.size());
        for (const auto& g : p.segs) std::printf(" %u %u %u %llu", g.first, g.count, g.W, (unsigned long long)g.mask_off);
      } else std::printf(" 0");
      std::printf("\n");
    } else if (tag == "S") {
      uint32_t n;
      std::cin >> n;
      std::printf("%u\n", sa_frames_spill_launches(n));
    } else {
      return 2;
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("frames_plan")
    (d / "drv.cpp").write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", str(CSRC), str(d / "drv.cpp"), "-o", str(d / "drv")], check=True)

    def run(lines):
        out = subprocess.run([str(d / "drv")], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        res = [[int(x) for x in line.split()] for line in out.splitlines()]
        assert len(res) == len(lines)
        return res

    return run


def plan(drv, counts, nms):
    (out,) = drv([" ".join(["P", str(int(nms)), str(len(counts))] + [str(c) for c in counts])])
    head, n = out[:7], out[7]
    return head, np.array(out[8:], np.int64).reshape(n, 4)


def expected(counts, nms):
    """The table written out: segments back to back, W = ceil(count / 64), masks back to back in words."""
    first = words = 0
    rows = []
    for c in counts:
        W = (c + 63) // 64 if nms else 0
        rows.append((first, c, W, words))
        first += c
        words += c * W
    max_W = max([r[2] for r in rows] + [0])
    S = (max_W + 63) // 64
    return np.array(rows, np.int64).reshape(len(counts), 4), first, max(list(counts) + [0]), max_W, (0 if not nms or not S else 1 if S <= 1 else 2 if S <= 2 else 4), words


@pytest.mark.parametrize("nms", [False, True])
@pytest.mark.parametrize("counts", [
    [0, 1, 3, 64, 65, 130], [130, 65, 64, 3, 1, 0],            # zeros first and last, a one-box scene, the 64 / 65 edges
    [0, 0, 0], [0], [1], [64], [65], [63, 0, 64, 0, 65, 0, 129],
    [4096, 17], [4097, 17, 200], [8192, 8193], [16384], [1, 16384, 1],
])
def test_segments_lie_back_to_back(drv, counts, nms):
    head, segs = plan(drv, counts, nms)
    rows, total, max_count, max_W, S, words = expected(counts, nms)
    assert head == [FITS, 0, total, max_count, max_W, S, words]
    assert np.array_equal(segs, rows)
    # no two scenes share a row or a mask word, and nothing lies beyond the totals
    ends = segs[:, 0] + segs[:, 1]
    assert np.all(ends[:-1] == segs[1:, 0]) and (len(counts) == 0 or ends[-1] == total)
    if nms:
        mends = segs[:, 3] + segs[:, 1] * segs[:, 2]
        assert np.all(mends[:-1] == segs[1:, 3]) and mends[-1] == words


@pytest.mark.parametrize("n,S", [(1, 1), (64, 1), (65, 1), (4096, 1), (4097, 2), (8192, 2), (8193, 4), (16384, 4)])
def test_the_plan_of_one_scene(drv, n, S):
    """What sa_nms / sa_own_areas run: one segment that is the whole block, its mask at word 0."""
    W = -(-n // 64)
    head, segs = plan(drv, [n], True)
    assert head == [FITS, 0, n, n, W, S, n * W]       # total, max_count = n; mask_words = n * W
    assert segs.tolist() == [[0, n, W, 0]]            # first, count, W, mask_off
    head, segs = plan(drv, [n], False)
    assert head == [FITS, 0, n, n, 0, 0, 0] and segs.tolist() == [[0, n, 0, 0]]


def test_one_scene_past_the_pair_stage_is_refused(drv):
    assert plan(drv, [16385], True)[0][:2] == [SCENE_TOO_LARGE, 0]
    assert plan(drv, [16385], False)[0][0] == FITS


def test_the_sweep_class_follows_the_largest_scene(drv):
    # k_nms_sweep<S> keeps 64 * 64 * S bits of removed-bitmap: 4096 boxes per word of S
    for n, S in [(1, 1), (4096, 1), (4097, 2), (8192, 2), (8193, 4), (12288, 4), (12289, 4), (16384, 4)]:
        assert plan(drv, [17, n, 200], True)[0][5] == S, n
        assert plan(drv, [n], False)[0][5] == 0
    assert plan(drv, [0, 0], True)[0][5] == 0   # nothing reaches the device: nothing is launched


def test_scene_size_limit_of_the_pair_stage(drv):
    assert plan(drv, [5, 16384, 7], True)[0][0] == FITS
    head, _ = plan(drv, [5, 7, 16385, 9], True)
    assert head[:2] == [SCENE_TOO_LARGE, 2]
    head, segs = plan(drv, [5, 7, 16385, 9], False)   # own areas have no such limit
    assert head[0] == FITS and segs[3, 0] == 5 + 7 + 16385


def test_scene_count_limit(drv):
    ok, bad, ok1, bad1 = drv(["R 0 65535 0", "R 0 65536 0", "R 1 65535 1", "R 1 65536 1"])
    assert ok[:3] == [FITS, 0, 0] and bad[0] == TOO_MANY_SCENES
    assert ok1[:7] == [FITS, 0, 65535, 1, 1, 1, 65535] and bad1[0] == TOO_MANY_SCENES


def test_row_total_must_fit_32_bits(drv):
    (fits, over) = drv(["R 0 4 1073741823", "R 0 5 1073741824"])
    assert fits[:3] == [FITS, 0, 4 * 1073741823]
    assert over[:2] == [TOO_MANY_ROWS, 3]   # the scene that crosses 2^32 - 1


def test_spill_lists_of_64(drv):
    assert [r[0] for r in drv(["S %d" % n for n in (0, 1, 63, 64, 65, 128, 129, 200)])] == [0, 1, 1, 1, 2, 2, 3, 4]
