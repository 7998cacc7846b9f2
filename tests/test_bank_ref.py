"""The feature-bank policy on the host: similari_amd/csrc/sa_kalman.h is compiled with the host compiler behind a small driver, and its
sa_bank_policy / sa_feature_can_be_used — the code the device step runs as thread 0 of every bank block — are compared with
tests/bank_ref.py for every bank depth, over random presence patterns, tied qualities and the gates' edges; then the model is held
against cases worked by hand from the reference text (visual_sort/metric.rs:129-154, 227-249, 297-374)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bank_ref as B

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "similari_amd" / "csrc"
DRIVER = r"""
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include "sa_kalman.h"
// stdin, one case per line; floats travel as their 32-bit patterns
//   P K  present[K]  quality[K]                              ->  m  src[K]
//   F minimal_area aspect height q min_q has_own own min_own  ->  0 | 1
static float f(uint32_t u) { float v; memcpy(&v, &u, 4); return v; }
int main() {
  std::string what;
  while (std::cin >> what) {
    if (what == "P") {
      uint32_t K;
      std::cin >> K;
      uint8_t present[SA_MAX_BANK], src[SA_MAX_BANK];
      float quality[SA_MAX_BANK];
      for (uint32_t k = 0; k < K; ++k) { uint32_t p; std::cin >> p; present[k] = (uint8_t)p; }
      for (uint32_t k = 0; k < K; ++k) { uint32_t u; std::cin >> u; quality[k] = f(u); }
      const uint32_t m = sa_bank_policy(K, K, present, quality, src);
      std::printf("%u", m);
      for (uint32_t k = 0; k < K; ++k) std::printf(" %u", (unsigned)src[k]);
      std::printf("\n");
    } else {
      uint32_t u[8];
      for (int i = 0; i < 8; ++i) std::cin >> u[i];
      sa_box b{};
      b.aspect = f(u[1]); b.height = f(u[2]);
      std::printf("%d\n", sa_feature_can_be_used(f(u[0]), b, f(u[3]), f(u[4]), u[5] != 0, f(u[6]), f(u[7])) ? 1 : 0);
    }
  }
  return 0;
}
"""
SA_BANK_NEW, SA_BANK_NONE = 0xFE, 0xFF


def bits(x):
    return int(np.float32(x).view(np.uint32))


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("bank")
    (d / "drv.cpp").write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", str(CSRC), str(d / "drv.cpp"), "-o", str(d / "drv")],
                   check=True)

    def run(lines):
        out = subprocess.run([str(d / "drv")], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        res = [[int(x) for x in line.split()] for line in out.splitlines()]
        assert len(res) == len(lines)
        return res

    return run


def header_src(out, K):
    """the driver's (m, src[K]) in the model's terms"""
    return [B.NEW if s == SA_BANK_NEW else B.EMPTY if s == SA_BANK_NONE else s for s in out[1 : 1 + K]], out[0]


LEVELS = np.array([0.1, 0.5, 0.5000001, 0.9], np.float32)   # few levels: most banks hold ties, two levels one ulp-ish apart


def test_the_header_is_the_model(drv):
    """Every K in 1..16: the all-present and the none-present bank, and 60 random presence patterns each, qualities drawn from four
    levels.  The m >= K drop is taken (a full bank) and not taken (any other) at every K."""
    rng = np.random.default_rng(11)
    cases = []
    for K in range(1, 17):
        pats = [np.ones(K, np.uint8), np.zeros(K, np.uint8)]
        pats += [(rng.uniform(size=K) < rng.choice([0.3, 0.7, 0.95])).astype(np.uint8) for _ in range(60)]
        for p in pats:
            cases.append((K, p, LEVELS[rng.integers(0, len(LEVELS), K)]))
        cases.append((K, np.ones(K, np.uint8), np.full(K, 0.5, np.float32)))   # a full bank of one quality: the last slot goes
    outs = drv(["P %d %s %s" % (K, " ".join(map(str, p)), " ".join(str(bits(q)) for q in qs)) for K, p, qs in cases])
    dropped = {}
    for (K, p, qs), out in zip(cases, outs):
        want, m = B.policy(K, p, qs)
        got, gm = header_src(out, K)
        assert (got, gm) == (want, m), (K, p.tolist(), qs.tolist())
        # what the policy is, whatever the order: NEW in front, every kept slot once, only present slots, at most one of them gone
        assert got[0] == B.NEW and m == min(int(p.sum()) + 1, K)
        old = [s for s in got if s not in (B.NEW, B.EMPTY)]
        assert len(set(old)) == len(old) == m - 1 and all(p[s] for s in old)
        assert got[m:] == [B.EMPTY] * (K - m)
        dropped.setdefault(K, set()).add(int(p.sum()) >= K)
    assert all(dropped[K] == {False, True} for K in range(1, 17)), dropped


def test_ties_keep_their_order_and_the_drop_takes_the_last_of_the_lowest(drv):
    """By hand.  K = 4, full, qualities .5 .9 .5 .5: sorted 1 0 2 3 (ties in slot order), the last (slot 3) goes, NEW is pushed and
    swapped with the front: NEW 0 2 1."""
    assert B.policy(4, [1, 1, 1, 1], [0.5, 0.9, 0.5, 0.5]) == ([B.NEW, 0, 2, 1], 4)
    assert header_src(drv(["P 4 1 1 1 1 %d %d %d %d" % tuple(bits(q) for q in (0.5, 0.9, 0.5, 0.5))])[0], 4) == ([B.NEW, 0, 2, 1], 4)
    # the lowest quality sits in FRONT (the newest observation was a poor one): it is the one that goes
    assert B.policy(4, [1, 1, 1, 1], [0.1, 0.9, 0.5, 0.5]) == ([B.NEW, 2, 3, 1], 4)
    # K = 1: the bank is full with one row, which goes; an empty K = 1 bank just takes the new one
    assert B.policy(1, [1], [0.9]) == ([B.NEW], 1) and B.policy(1, [0], [0.0]) == ([B.NEW], 1)
    # one present row, K = 3: [s, NEW] swapped -> NEW s
    assert B.policy(3, [0, 0, 1], [0.0, 0.0, 0.7]) == ([B.NEW, 2, B.EMPTY], 2)


def test_the_issue_example(drv):
    """K = 8, slot 2 absent, qualities .5 .5 - .9 .1 .5 .7 .2: retained 0 1 3 4 5 6 7, sorted 3 6 0 1 5 7 4, seven < eight so nothing
    goes, push NEW, swap the ends: NEW 6 0 1 5 7 4 3."""
    p = [1, 1, 0, 1, 1, 1, 1, 1]
    q = [0.5, 0.5, 0.33, 0.9, 0.1, 0.5, 0.7, 0.2]    # (the absent slot's quality is not looked at)
    want = ([B.NEW, 6, 0, 1, 5, 7, 4, 3], 8)
    assert B.policy(8, p, q) == want
    out = drv(["P 8 %s %s" % (" ".join(map(str, p)), " ".join(str(bits(x)) for x in q))])[0]
    assert header_src(out, 8) == want


def test_feature_can_be_used_at_the_gate_edges(drv):
    """q == min_q, area == minimal_area, own share absent, own share == min_own: all pass (>=); one ulp below each gate fails.  The area
    is formed in f32 as (height * aspect) * height."""
    h, a = np.float32(37.3), np.float32(0.73)
    area = np.float32(np.float32(h * a) * h)
    below = lambda x: np.nextafter(np.float32(x), np.float32(-np.inf))
    above = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))
    cases = []
    for min_area in (np.float32(0.0), below(area), area, above(area)):
        for q, min_q in ((0.4, 0.4), (below(0.4), 0.4), (0.9, 0.4), (0.0, 0.0)):
            for own, min_own in ((None, 0.5), (0.5, 0.5), (below(0.5), 0.5), (1.0, 0.5), (0.0, 0.0)):
                cases.append((min_area, a, h, q, min_q, own, min_own))
    outs = drv(["F %d %d %d %d %d %d %d %d" % (bits(ma), bits(a_), bits(h_), bits(q), bits(mq), own is not None, bits(0.0 if own is None else own), bits(mo))
                for ma, a_, h_, q, mq, own, mo in cases])
    seen = set()
    for c, out in zip(cases, outs):
        want = B.feature_can_be_used(*c)
        assert bool(out[0]) == want, c
        seen.add(want)
    assert seen == {False, True}
    f = B.feature_can_be_used
    assert f(area, a, h, 0.4, 0.4, None, 0.5) and f(area, a, h, 0.4, 0.4, 0.5, 0.5)
    assert not f(above(area), a, h, 0.4, 0.4, None, 0.5)
    assert not f(area, a, h, below(0.4), 0.4, None, 0.5)
    assert not f(area, a, h, 0.4, 0.4, below(0.5), 0.5)


def test_step_by_hand():
    """metric.rs:297-374 on a K = 3 bank.  A new track keeps a poor observation as it came; a merge below the collect gate re-sorts the
    bank and puts a featureless observation (quality kept) in front; the next merge drops that one (no feature) and collects."""
    D = 4
    row = lambda v: np.full(D, v, np.float32)
    gates = dict(minimal_area=100.0, q_collect=0.5, own_collect=0.3)
    b = B.step(B.Bank(3, D), False, row(1), 0.1, 0.5, 40.0, None, **gates)            # new, quality below the gate: kept
    assert b.src == [B.NEW, None, None] and b.present.tolist() == [1, 0, 0] and b.quality.tolist() == [np.float32(0.1), 0, 0] and b.count == 1
    b = B.step(b, True, row(2), 0.9, 0.5, 40.0, None, **gates)                         # collected: NEW in front
    assert b.src == [B.NEW, 0, None] and b.rows[:, 0].tolist() == [2, 1, 0] and b.count == 2
    b = B.step(b, True, row(3), 0.4, 0.5, 40.0, None, **gates)                         # below q_collect: sorted (.9 .1), nothing added
    assert b.src == [B.NEW, 1, 0] and b.present.tolist() == [0, 1, 1] and b.rows[:, 0].tolist() == [0, 1, 2]
    assert b.quality.tolist() == [np.float32(0.4), np.float32(0.1), np.float32(0.9)] and b.count == 2
    b = B.step(b, True, row(4), 0.6, 0.5, 40.0, 0.3, **gates)                          # own share == the gate: collected; slot 0 (no feature) is gone
    assert b.src == [B.NEW, 1, 2] and b.rows[:, 0].tolist() == [4, 1, 2] and b.count == 3
    b = B.step(b, True, row(5), 0.6, 0.5, 40.0, None, **gates)                         # full: .9 .6 .1 -> .1 goes
    assert b.src == [B.NEW, 0, 2] and b.rows[:, 0].tolist() == [5, 4, 2] and b.quality.tolist() == [np.float32(0.6)] * 2 + [np.float32(0.9)]
    b2 = B.step(b, True, None, 0.9, 0.5, 40.0, None, **gates)                          # no feature at all: full bank still loses its last
    assert b2.src == [B.NEW, 0, 2] and b2.present.tolist() == [0, 1, 1] and b2.rows[:, 0].tolist() == [0, 5, 2]
    b3 = B.step(b, True, row(6), 0.9, 0.5, 4.0, None, **gates)                         # 0.5 * 4 * 4 = 8 < 100: the box is too small
    assert b3.present.tolist() == [0, 1, 1] and b3.quality[0] == np.float32(0.9)
    b4 = B.step(b, False, None, 0.7, 0.5, 40.0, None, **gates)                         # a new track without a feature
    assert b4.src == [B.NEW, None, None] and b4.count == 0 and b4.quality.tolist() == [np.float32(0.7), 0, 0] and not b4.rows.any()
