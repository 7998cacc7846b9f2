"""The host arithmetic behind sa_points_track / sa_points_track_batch (similari_amd/csrc/sa_pose_track_plan.h): from the columns the vote
gave the poses of a call, the slot every pose steps, the created count, each created track's place in call order and the listed tracks
that coast.  The header is compiled with the host compiler behind a small driver and compared with the same rule written in numpy.  Also:
the two structs of include/similari_pose_track.h are as large as their ctypes mirrors."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "similari_amd" / "csrc"
NONE = 0xFFFFFFFF
DRIVER = r"""
#include <cstdio>
#include <iostream>
#include "sa_pose_track_plan.h"
#include "../../include/similari_pose_track.h"
// stdin, one case per line:  T_old identity S (n m){S} (col){sum m} (slot){sum n}
//   ->  sizeof(options) sizeof(stats) matched created | (slot){sum m} | (rank){sum m} | (unmatched){S} | k (coasted){k}
int main() {
  uint32_t T_old, identity, S;
  while (std::cin >> T_old >> identity >> S) {
    std::vector<uint32_t> n(S), m(S);
    size_t M = 0, N = 0;
    for (uint32_t s = 0; s < S; ++s) { std::cin >> n[s] >> m[s]; M += m[s]; N += n[s]; }
    std::vector<int32_t> cols(M);
    std::vector<uint32_t> slots(N);
    for (auto& c : cols) std::cin >> c;
    for (auto& v : slots) std::cin >> v;
    SaPoseTrackPlan p;
    sa_pose_track_plan(S, n.data(), m.data(), cols.data(), identity ? nullptr : slots.data(), T_old, &p);
    if (p.slot.size() != M || p.rank.size() != M || p.unmatched.size() != S) return 3;
    std::printf("%zu %zu %u %u |", sizeof(sa_pose_track_options), sizeof(sa_pose_track_stats), p.matched, p.created);
    for (uint32_t v : p.slot) std::printf(" %u", v);
    std::printf(" |");
    for (uint32_t v : p.rank) std::printf(" %u", v);
    std::printf(" |");
    for (uint32_t v : p.unmatched) std::printf(" %u", v);
    std::printf(" | %zu", p.coasted.size());
    for (uint32_t v : p.coasted) std::printf(" %u", v);
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
    d = tmp_path_factory.mktemp("pose_track_plan")
    (d / "drv.cpp").write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", str(CSRC), str(d / "drv.cpp"), "-o", str(d / "drv")], check=True)

    def run(T_old, scenes, cols, slots):
        """scenes: (m, n) per scene; slots None: the listed tracks are slots 0, 1, 2, ..."""
        ident = slots is None
        slots = np.arange(sum(n for _, n in scenes)) if ident else slots
        line = " ".join(str(int(v)) for v in [T_old, int(ident), len(scenes)] + [x for m, n in scenes for x in (n, m)] + list(cols) + list(slots))
        out = subprocess.run([str(d / "drv")], input=line + "\n", capture_output=True, text=True, check=True).stdout
        parts = [[int(x) for x in part.split()] for part in out.strip().split("|")]
        assert len(parts) == 5 and parts[4][0] == len(parts[4]) - 1
        return dict(sizes=parts[0][:2], matched=parts[0][2], created=parts[0][3], slot=parts[1], rank=parts[2], unmatched=parts[3], coasted=parts[4][1:])

    return run


def expected(T_old, scenes, cols, slots):
    """The rule in numpy: an unmatched pose is the k-th unmatched pose of the whole call, k counting scene after scene, then pose order."""
    cols = np.asarray(cols, np.int64)
    ns = np.repeat([n for _, n in scenes], [m for m, _ in scenes])                        # the tracks of each pose's scene
    t0 = np.repeat(np.cumsum([0] + [n for _, n in scenes])[:-1], [m for m, _ in scenes])  # and its first track
    hit = (cols >= 0) & (cols < ns)
    k = np.cumsum(~hit) - 1
    slots = np.arange(sum(n for _, n in scenes)) if slots is None else np.asarray(slots)
    slot = np.where(hit, slots[np.where(hit, t0 + cols, 0)] if len(slots) else 0, T_old + k)
    rank = np.where(hit, NONE, k)
    taken = np.zeros(len(slots), bool)
    taken[(t0 + cols)[hit]] = True
    ends = np.cumsum([m for m, _ in scenes])
    unmatched = [int((~hit)[e - m: e].sum()) for e, (m, _) in zip(ends, scenes)]
    return dict(matched=int(hit.sum()), created=int((~hit).sum()), slot=slot.tolist(), rank=rank.tolist(), unmatched=unmatched,
                coasted=np.flatnonzero(~taken).tolist())


def check(drv, T_old, scenes, cols, slots=None):
    got, want = drv(T_old, scenes, cols, slots), expected(T_old, scenes, cols, slots)
    for key, v in want.items():
        assert got[key] == v, key
    return got


def random_cols(rng, scenes, p_match):
    """Per scene a partial injective map pose -> column, -1 = none."""
    cols = []
    for m, n in scenes:
        c = np.full(m, -1, np.int64)
        rows = np.flatnonzero(rng.random(m) < p_match)[:n]
        c[rows] = rng.permutation(n)[: len(rows)]
        cols += c.tolist()
    return cols


SEVEN = [(1, 1), (3, 5), (0, 4), (17, 70), (4, 0), (70, 17), (17, 65)]   # (poses, tracks): a scene without poses, one without tracks


@pytest.mark.parametrize("p_match", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("scenes", [SEVEN, SEVEN[::-1], [(0, 3), (0, 0), (5, 0)], [(6, 6)], [(0, 9)]])
def test_mixed_scenes(drv, scenes, p_match):
    rng = np.random.default_rng(len(scenes) * 10 + int(p_match * 2))
    cols = random_cols(rng, scenes, p_match)
    n = sum(t for _, t in scenes)
    T_old = n + 13
    slots = rng.permutation(T_old)[:n]   # the listed tracks lie anywhere in the bank
    got = check(drv, T_old, scenes, cols, slots)
    check(drv, T_old, scenes, cols)
    # what the call relies on: the created tracks take the slots behind the bank's, one after the other in call order
    made = [s for s, r in zip(got["slot"], got["rank"]) if r != NONE]
    assert made == list(range(T_old, T_old + got["created"]))
    assert got["matched"] + got["created"] == len(cols) and sum(got["unmatched"]) == got["created"]
    assert len(got["coasted"]) == n - got["matched"]


def test_all_matched_and_none_matched(drv):
    scenes = [(3, 3), (2, 4)]
    got = check(drv, 20, scenes, [2, 0, 1, 3, 1], slots=[7, 8, 9, 1, 2, 3, 4])
    assert got["created"] == 0 and got["slot"] == [9, 7, 8, 4, 2] and got["coasted"] == [3, 5] and got["unmatched"] == [0, 0]
    got = check(drv, 20, scenes, [-1] * 5, slots=[7, 8, 9, 1, 2, 3, 4])
    assert got["created"] == 5 and got["slot"] == [20, 21, 22, 23, 24] and got["rank"] == [0, 1, 2, 3, 4] and got["coasted"] == list(range(7))
    assert got["unmatched"] == [3, 2]


def test_a_column_beyond_the_scene_counts_as_none(drv):
    got = check(drv, 5, [(2, 2), (1, 3)], [2, 1, 3])   # column 2 of a two-track scene, column 3 of a three-track one
    assert got["rank"] == [0, NONE, 1] and got["slot"] == [5, 1, 6] and got["coasted"] == [0, 2, 3, 4]


def test_the_structs_are_as_large_as_their_mirrors(drv):
    from similari_amd import pose_track as PT

    got = drv(0, [(0, 0)], [], None)
    assert got["sizes"] == [C.sizeof(PT.sa_pose_track_options), C.sizeof(PT.sa_pose_track_stats)] == [16, 112]
