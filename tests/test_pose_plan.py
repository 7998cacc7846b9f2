"""The plan of a keypoint vote (similari_amd/csrc/sa_pose_plan.h: the scenes of sa_points_associate_batch, the one scene of a single
call) on the host: the header is compiled with the host compiler behind a small driver, and its segment table, totals and refusals are compared with the same arithmetic written out here."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "similari_amd" / "csrc"
FITS, TOO_MANY_SCENES, SCENE_TOO_LARGE, TOO_MANY_POSES, TOO_MANY_TRACKS, TOO_MANY_CELLS = range(6)
SIDE, SCENES, CELLS = 2048, 65535, 1 << 27
DRIVER = r"""
#include <cstdio>
#include <iostream>
#include <string>
#include "sa_pose_plan.h"
// stdin, one case per line:
//   P side S (n m){S}   ->  refusal bad_scene poses tracks tiles cells S (pose0 m track0 n cell0 tile0 tiles_x){S}
//   R side S n m        ->  the same for S scenes of m poses x n tracks each, without the table (S may be large)
int main() {
  static_assert(sizeof(SaPoseSeg) == 32, "the device reads this layout");
  static_assert(SA_POSE_PLAN_SIDE == 2048u && SA_POSE_PLAN_SCENES == 65535u && SA_POSE_PLAN_CELLS == (1ull << 27), "the limits of the public headers");
  std::string tag;
  while (std::cin >> tag) {
    if (tag != "P" && tag != "R") return 2;
    uint32_t side, S;
    std::cin >> side >> S;
    std::vector<uint32_t> n(S), m(S);
    if (tag == "P") for (uint32_t s = 0; s < S; ++s) std::cin >> n[s] >> m[s];
    else { uint32_t nv, mv; std::cin >> nv >> mv; for (uint32_t s = 0; s < S; ++s) { n[s] = nv; m[s] = mv; } }
    SaPosePlan p;
    uint32_t bad = 77;
    const int r = (int)sa_pose_plan(S, n.data(), m.data(), side, &p, &bad);
    std::printf("%d %u %u %u %u %llu", r, bad, p.poses, p.tracks, p.tiles, (unsigned long long)p.cells);
    if (tag == "P" && r == 0) {
      std::printf(" %zu", p.segs.size());
      for (const auto& g : p.segs) std::printf(" %u %u %u %u %llu %u %u", g.pose0, g.m, g.track0, g.n, (unsigned long long)g.cell0, g.tile0, g.tiles_x);
    } else std::printf(" 0");
    std::printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("pose_plan")
    (d / "drv.cpp").write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", str(CSRC), str(d / "drv.cpp"), "-o", str(d / "drv")], check=True)

    def run(lines):
        out = subprocess.run([str(d / "drv")], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        res = [[int(x) for x in line.split()] for line in out.splitlines()]
        assert len(res) == len(lines)
        return res

    return run


def plan(drv, scenes, side=SIDE):
    """scenes: (m, n) = (poses, tracks) per scene -> (head [refusal, bad, poses, tracks, tiles, cells], segs [S, 7])"""
    (out,) = drv([" ".join(["P", str(side), str(len(scenes))] + ["%d %d" % (n, m) for m, n in scenes])])
    return out[:6], np.array(out[7:], np.int64).reshape(out[6], 7)


def expected(scenes):
    """The table written out: poses, tracks, cells and tiles back to back; a scene without poses or without tracks has no tile."""
    pose0 = track0 = cell0 = tile0 = 0
    rows = []
    for m, n in scenes:
        tx = (n + 63) // 64 if m else 0
        rows.append((pose0, m, track0, n, cell0, tile0, tx))
        pose0, track0, cell0, tile0 = pose0 + m, track0 + n, cell0 + m * n, tile0 + (m + 15) // 16 * tx
    return np.array(rows, np.int64).reshape(len(scenes), 7), [pose0, track0, tile0, cell0]


SIX = [(1, 1), (3, 5), (0, 4), (17, 70), (4, 0), (70, 17)]


@pytest.mark.parametrize("scenes", [
    SIX, SIX + [(17, 65)], SIX[::-1],
    [(0, 0)], [(0, 0), (0, 7), (7, 0)], [(7, 0), (1, 1), (0, 0)],          # nothing but empty scenes; empty ones first and last
    [(16, 64)], [(17, 64)], [(16, 65)], [(17, 65)], [(1, 2048), (2048, 1)],   # at and one across the tile edges
    [(2048, 2048), (1, 1)], [(100, 100)] * 64,
])
def test_segments_lie_back_to_back(drv, scenes):
    head, segs = plan(drv, scenes)
    rows, totals = expected(scenes)
    assert head == [FITS, 0] + totals
    assert np.array_equal(segs, rows)
    # the block of the tile launch -> its scene, as k_pose_tile finds it: the last scene whose first tile is not beyond the block
    tile0 = segs[:, 5]
    for b in range(totals[2]):
        s = int(np.flatnonzero(tile0 <= b)[-1])
        m, n, tx = segs[s, 1], segs[s, 3], segs[s, 6]
        t = b - tile0[s]
        assert m > 0 and n > 0 and tx > 0 and (t // tx) * 16 < m and (t % tx) * 64 < n, (b, s)
    # every tile of every scene is some block's: the counts add up
    assert sum((m + 15) // 16 * ((n + 63) // 64) for m, n in scenes if m and n) == totals[2]


@pytest.mark.parametrize("m,n", [(1, 1), (17, 70), (70, 17), (33, 130), (2048, 2048)])
def test_the_single_call_is_the_plan_of_one_scene(drv, m, n):
    """sa_points_associate and sa_points_track plan their call as one scene and launch the plan's 1-D tile grid: everything starts at 0,
    and block b is the tile (b // tiles_x, b % tiles_x) of the ceil(m / 16) x ceil(n / 64) tiles of the matrix, each exactly once."""
    head, segs = plan(drv, [(m, n)])
    ty, tx = (m + 15) // 16, (n + 63) // 64
    assert head == [FITS, 0, m, n, ty * tx, m * n]
    pose0, sm, track0, sn, cell0, tile0, tiles_x = segs[0]
    assert pose0 == track0 == cell0 == tile0 == 0 and (sm, sn) == (m, n)
    assert tiles_x == tx and head[4] == ty * tx
    assert [(b // tiles_x, b % tiles_x) for b in range(head[4])] == [(y, x) for y in range(ty) for x in range(tx)]


def test_a_scene_beyond_the_side_is_refused_with_its_number(drv):
    assert plan(drv, [(5, 5), (2048, 2048), (7, 7)])[0][0] == FITS
    assert plan(drv, [(5, 5), (7, 7), (2049, 1), (9, 9)])[0][:2] == [SCENE_TOO_LARGE, 2]
    assert plan(drv, [(5, 5), (1, 2049), (2049, 1)])[0][:2] == [SCENE_TOO_LARGE, 1]   # the first such scene
    assert plan(drv, [(0, 2049)])[0][:2] == [SCENE_TOO_LARGE, 0]                        # also one that would have no pair
    assert plan(drv, [(2049, 0)])[0][:2] == [SCENE_TOO_LARGE, 0]


def test_scene_count_limit(drv):
    ok, bad, ok1 = drv(["R %d 65535 0 0" % SIDE, "R %d 65536 0 0" % SIDE, "R %d 65535 1 1" % SIDE])
    assert ok[:6] == [FITS, 0, 0, 0, 0, 0] and bad[0] == TOO_MANY_SCENES
    assert ok1[:6] == [FITS, 0, 65535, 65535, 65535, 65535]


def test_the_cell_cap_at_exactly_2_27_and_one_above(drv):
    full = [(2048, 2048)] * 32
    head, segs = plan(drv, full)
    assert head == [FITS, 0, 32 * 2048, 32 * 2048, 32 * 128 * 32, CELLS] and segs[31, 4] == 31 * 2048 * 2048
    assert plan(drv, full + [(0, 5), (5, 0)])[0][:2] == [FITS, 0]            # scenes without a pair add nothing
    assert plan(drv, full + [(0, 5), (1, 1)])[0][:2] == [TOO_MANY_CELLS, 33]   # one pair above, named by the scene that crosses
    assert plan(drv, [(1, 1)] + full)[0][:2] == [TOO_MANY_CELLS, 32]
    assert plan(drv, full[:31] + [(2048, 2047), (1, 2048)])[0][:2] == [FITS, 0]
    assert plan(drv, full[:31] + [(2048, 2047), (1, 2048), (1, 1)])[0][:2] == [TOO_MANY_CELLS, 33]


def test_sums_must_fit_32_bits(drv):
    # within the call's side of 2048 and 65535 scenes the sums stay below 2^27; the two refusals guard a larger side
    big = 0xFFFFFFFF
    fits, poses, tracks = drv(["R %d 4 0 1073741823" % big, "R %d 5 0 1073741824" % big, "R %d 5 1073741824 0" % big])
    assert fits[:6] == [FITS, 0, 4 * 1073741823, 0, 0, 0]
    assert poses[:2] == [TOO_MANY_POSES, 3]     # the scene that crosses 2^32 - 1
    assert tracks[:2] == [TOO_MANY_TRACKS, 3]
    assert plan(drv, [(3, 0), (big, 0)], side=big)[0][:2] == [TOO_MANY_POSES, 1]
    assert plan(drv, [(big, 0), (0, big)], side=big)[0][:4] == [FITS, 0, big, big]
