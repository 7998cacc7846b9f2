"""The host's half of the keypoint tracker (similari_amd/csrc/sa_pose_sort_plan.h): epochs, expiry, the compaction of the bank, the
per-track limits, the lists and the id counter.  The header is compiled with the host compiler behind a small driver that holds a
tracker state and answers commands; tests/pose_sort_ref.RefSort gets the same commands and the same vote columns, and after every one
the two states are compared.  Also: the structs of include/similari_pose_sort.h are as large as their ctypes mirrors, the binding
declares what the header declares, and the library exports it."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pose_sort_ref as SR

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "similari_amd" / "csrc"
HEADER = ROOT / "include" / "similari_pose_sort.h"
f32, u32 = np.float32, np.uint32
DRIVER = r"""
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include "sa_pose_sort_plan.h"
#include "../../include/similari_pose_sort.h"
static SaPoseSortState t;
static void dump() {
  std::printf("next %llu | order", (unsigned long long)t.next_id);
  for (const auto& s : t.slot) std::printf(" %llu:%llu:%u:%u:%u", (unsigned long long)s.id, (unsigned long long)t.scene_id[s.scene], s.first, s.last, s.length);
  std::printf(" | scenes");
  for (size_t k = 0; k < t.scene_id.size(); ++k) {
    std::printf(" %llu:%u:", (unsigned long long)t.scene_id[k], t.epoch[k]);
    for (uint32_t s : t.list[k]) std::printf("%llu,", (unsigned long long)t.slot[s].id);
  }
  std::printf("\n");
}
// commands, one per line:
//   init max_idle n (delta dist){n}
//   frame max_tracks S (scene){S} (poses){S} (col){sum poses}   -> fit bad | epochs | leaving ids | track counts | slot ids | limit bits, then the state
//   skip scene n
//   sizes
int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "init") {
      uint32_t n;
      t = SaPoseSortState();
      std::cin >> t.max_idle >> n;
      std::vector<uint32_t> d(n);
      std::vector<float> x(n);
      for (uint32_t i = 0; i < n; ++i) std::cin >> d[i] >> x[i];
      sa_pose_sort_constraints(n, d.data(), x.data(), &t.cons);
      std::printf("cons");
      for (auto& c : t.cons) { uint32_t b; std::memcpy(&b, &c.second, 4); std::printf(" %u:%08x", c.first, b); }
      std::printf("\n");
    } else if (cmd == "frame") {
      uint32_t max_tracks, S;
      std::cin >> max_tracks >> S;
      std::vector<uint64_t> ids(S);
      std::vector<uint32_t> pc(S);
      size_t m = 0;
      for (auto& v : ids) std::cin >> v;
      for (auto& v : pc) { std::cin >> v; m += v; }
      std::vector<int32_t> cols(m);
      for (auto& v : cols) std::cin >> v;
      SaPoseSortFrame f;
      uint32_t bad = 0;
      const int fit = sa_pose_sort_frame(t, S, ids.data(), max_tracks, &f, &bad);
      std::printf("fit %d %u |", fit, bad);
      if (fit == SA_POSE_SORT_FITS) {
        for (uint32_t e : f.epoch) std::printf(" %u", e);
        std::printf(" |");
        for (uint32_t s : f.leaving) std::printf(" %llu", (unsigned long long)t.slot[s].id);
        std::printf(" |");
        for (uint32_t n : f.track_counts) std::printf(" %u", n);
        std::printf(" |");
        for (uint32_t s : f.old_slots) std::printf(" %llu", (unsigned long long)t.slot[s].id);
        std::printf(" |");
        for (float x : f.limits) { uint32_t b; std::memcpy(&b, &x, 4); std::printf(" %08x", b); }
        std::printf(" | %d", f.gated ? 1 : 0);
        std::vector<SaPoseSortSlot> left;
        sa_pose_sort_expire(&t, S, ids.data(), f, &left);
        for (size_t k = 0; k < f.slots.size(); ++k)   // the slots after the compaction hold the same tracks
          if (f.slots[k] >= t.slot.size() || f.new_of[f.old_slots[k]] != f.slots[k]) return 4;
        SaPoseTrackPlan p;
        sa_pose_track_plan(S, f.track_counts.data(), pc.data(), cols.data(), f.slots.data(), (uint32_t)t.slot.size(), &p);
        sa_pose_sort_absorb(&t, f, pc.data(), p);
      }
      std::printf("\n");
      dump();
    } else if (cmd == "skip") {
      uint64_t scene; uint32_t n;
      std::cin >> scene >> n;
      sa_pose_sort_skip(&t, scene, n);
      dump();
    } else if (cmd == "sizes") {
      std::printf("%zu %zu %zu\n", sizeof(sa_pose_sort_options), sizeof(sa_pose_sort_track), sizeof(sa_pose_sort_stats));
    } else return 2;
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("pose_sort_plan")
    (d / "drv.cpp").write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", str(CSRC), str(d / "drv.cpp"), "-o", str(d / "drv")], check=True)

    def run(lines):
        out = subprocess.run([str(d / "drv")], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        return out.strip().split("\n")

    return run


def state_line(m):
    """RefSort's state as the driver prints it"""
    order = " ".join("%d:%d:%d:%d:%d" % (t, m.rec[t]["scene"], m.rec[t]["first"], m.rec[t]["last"], m.rec[t]["length"]) for t in m.order)
    scenes = " ".join("%d:%d:%s" % (s, m.epochs[s], "".join("%d," % t for t in m.lists[s])) for s in m.lists)
    return ("next %d | order %s | scenes %s" % (m.next_id, order, scenes)).replace("order  |", "order |").rstrip()


def fbits(x):
    return "%08x" % np.array(x, f32).view(u32)


class Both:
    """the driver's command lines and the model's answers to them, in step"""

    def __init__(self, max_idle, cons):
        self.m = SR.RefSort(1, max_idle, cons)
        self.lines = ["init %d %d %s" % (max_idle, len(cons), " ".join("%d %r" % (d, float(x)) for d, x in cons))]
        self.want = ["cons" + "".join(" %d:%s" % (d, fbits(x)) for d, x in self.m.cons)]

    def frame(self, rng, scenes, counts, p_match=0.6, max_tracks=2048, cols=None):
        if len(set(scenes)) != len(scenes):
            k = next(k for k, s in enumerate(scenes) if s in scenes[:k])
            self.lines.append("frame %d %d %s %s" % (max_tracks, len(scenes), " ".join(map(str, scenes)), " ".join(map(str, counts))) + " -1" * sum(counts))
            self.want += ["fit 1 %d |" % k, state_line(self.m)]
            return None
        pl = self.m.plan(scenes)
        big = [k for k, t in enumerate(pl["tracks"]) if len(t) > max_tracks]
        if cols is None:
            cols = []
            for m, tracks in zip(counts, pl["tracks"]):
                c = np.full(m, -1, np.int64)
                rows = np.flatnonzero(rng.random(m) < p_match)[: len(tracks)]
                c[rows] = rng.permutation(len(tracks))[: len(rows)]
                cols.append(c.tolist())
        self.lines.append("frame %d %d %s %s %s" % (max_tracks, len(scenes), " ".join(map(str, scenes)), " ".join(map(str, counts)),
                                                    " ".join(str(c) for cs in cols for c in cs)))
        if big:
            self.want += ["fit 2 %d |" % big[0], state_line(self.m)]
            return None
        lim = [x for ls in pl["limits"] for x in ls]
        head = "fit 0 0 | %s | %s | %s | %s | %s | %d" % (" ".join(map(str, pl["epoch"])), " ".join(map(str, pl["expired"])),
                                                       " ".join(str(len(t)) for t in pl["tracks"]), " ".join(str(t) for ts in pl["tracks"] for t in ts),
                                                       " ".join(fbits(x) for x in lim), int(any(np.isfinite(x) for x in lim)))
        out = self.m.apply(scenes, pl, cols)
        self.want += [re.sub(r"\s+", " ", head), state_line(self.m)]
        return pl, out

    def skip(self, scene, n):
        self.m.skip_epochs(scene, n)
        self.lines.append("skip %d %d" % (scene, n))
        self.want.append(state_line(self.m))

    def check(self, drv):
        got = [re.sub(r"\s+", " ", g).strip() for g in drv(self.lines)]
        assert len(got) == len(self.want)
        for k, (g, w) in enumerate(zip(got, self.want)):
            assert g == w.strip(), (k, self.lines)


def test_twelve_frames_of_four_scenes(drv):
    """Scenes 7, 8, 9 and 2^40: named and unnamed in turn, tracks matched, missed and born, idle ones expiring at exactly max_idle + 1,
    a limit per track, a skip — and the driver's state equals the model's after every command."""
    rng = np.random.default_rng(12)
    b = Both(4, [(3, 2.0), (1, 0.5), (3, 9.0)])   # (an idle delta of 4 has no constraint: +inf)
    scenes = [7, 8, 9, 1 << 40]
    expired, limits_seen, order_changed = 0, set(), 0
    for k in range(12):
        named = [s for s in scenes if rng.random() < 0.7] or [scenes[k % 4]]
        if k % 5 == 4:
            named = named[::-1]
        if k == 6:
            b.skip(8, 2)
            b.skip(555, 3)   # a scene never seen starts at n
        counts = [int(rng.integers(0, 6)) for _ in named]
        before = list(b.m.order)
        pl, _ = b.frame(rng, named, counts, p_match=0.5)
        expired += len(pl["expired"])
        limits_seen |= {float(x) for ls in pl["limits"] for x in ls}
        kept = [t for t in before if t not in pl["expired"]]
        order_changed += kept != b.m.order[: len(kept)]
    b.check(drv)
    assert expired >= 5 and limits_seen >= {0.5, 2.0, float("inf")} and order_changed >= 1   # removals from the middle moved tracks
    assert b.m.epochs[555] == 3 and b.m.next_id > 20


def test_expiry_at_exactly_max_idle_and_one_beyond(drv):
    rng = np.random.default_rng(1)
    b = Both(3, [])
    b.frame(rng, [1], [2], cols=[[-1, -1]])          # epoch 1: tracks 1 and 2 are born
    b.frame(rng, [1], [1], cols=[[0]])               # epoch 2: track 1 is seen, track 2 is not
    for e in (3, 4):
        pl, _ = b.frame(rng, [1], [1], cols=[[0]])
        assert pl["expired"] == []
    pl, _ = b.frame(rng, [1], [1], cols=[[0]])       # epoch 5: 5 - 1 = 4 > 3
    assert pl["expired"] == [2] and pl["epoch"] == [5] and b.m.lists[1] == [1]
    b.frame(rng, [2], [0])                           # another scene's frame changes nothing for scene 1
    assert b.m.epochs == {1: 5, 2: 1}
    b.skip(1, 3)                                     # epoch 8; the next predict is epoch 9: 9 - 5 = 4 > 3
    pl, _ = b.frame(rng, [1], [0])
    assert pl["expired"] == [1] and b.m.order == [] and b.m.next_id == 3
    b.check(drv)


def test_list_order_after_removals_and_the_banks_order(drv):
    rng = np.random.default_rng(2)
    b = Both(1, [(1, 1.0)])
    b.frame(rng, [1, 2], [3, 3], cols=[[-1] * 3, [-1] * 3])     # tracks 1..3 in scene 1, 4..6 in scene 2
    pl, _ = b.frame(rng, [1, 2], [2, 1], cols=[[2, 0], [1]])    # everybody listed: an idle delta of 1 expires nobody
    assert pl["expired"] == [] and pl["tracks"] == [[1, 2, 3], [4, 5, 6]]
    pl, _ = b.frame(rng, [2, 1], [1, 1], cols=[[0], [0]])       # delta 2 for 4 and 6, then for 2: scenes in call order, then list order
    assert pl["expired"] == [4, 6, 2] and pl["tracks"] == [[5], [1, 3]]
    assert b.m.order == [1, 5, 3] and b.m.lists == {1: [1, 3], 2: [5]}   # 6 into the hole of 4, 5 into the hole of 6, 5 again into the hole of 2
    b.check(drv)


def test_every_refusal_leaves_the_state_as_it_was(drv):
    rng = np.random.default_rng(3)
    b = Both(5, [(2, 1.5)])
    b.frame(rng, [1, 2], [4, 2], cols=[[-1] * 4, [-1] * 2])
    assert b.frame(rng, [1, 2, 1], [1, 1, 1]) is None           # a scene named twice
    assert b.frame(rng, [2, 1], [1, 1], max_tracks=3) is None   # scene 1 has 4 tracks
    pl, _ = b.frame(rng, [1, 2], [1, 1], cols=[[3], [0]])       # the next good call works
    assert pl["epoch"] == [2, 2]
    b.check(drv)


def test_the_structs_are_as_large_as_their_mirrors(drv):
    from similari_amd import pose_sort as S

    assert [int(x) for x in drv(["sizes"])[0].split()] == [C.sizeof(S.sa_pose_sort_options), C.sizeof(S.sa_pose_sort_track), C.sizeof(S.sa_pose_sort_stats)] == [104, 32, 144]
    for struct in (S.sa_pose_sort_options, S.sa_pose_sort_track, S.sa_pose_sort_stats):
        fields = re.search(r"typedef struct %s \{(.*?)\}" % struct.__name__, HEADER.read_text(), flags=re.S).group(1)
        fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
        names = [re.sub(r"\[.*", "", n).strip() for decl in fields.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert names == [f for f, _ in struct._fields_], struct.__name__


def test_every_declared_symbol_is_bound_and_exported():
    from similari_amd import build
    from similari_amd import pose_sort as S

    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:int|void|uint64_t|sa_points\s*\*)\s*(sa_[a-z0-9_]+)\s*\(", text, flags=re.M)))
    assert len(declared) == 13 and set(S.PROTOTYPES) == set(declared)
    lib = C.CDLL(str(build.build_lib()))
    assert not [n for n in declared if not hasattr(lib, n)]
    S.bind(lib)
    assert lib.sa_pose_sort_predict.restype is C.c_int
