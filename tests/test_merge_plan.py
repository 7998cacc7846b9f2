"""The merge plan (similari_amd/csrc/sa_merge_plan.h) on the host: the header is compiled with the host compiler behind a small
driver, its rows are applied to a numpy stand-in for the device arrays — every row gathered first, then every row scattered, as the
two launches do — and the result is compared with tests/merge_ref.py; its compaction moves are compared with a sequential
simulation of sa_store_remove."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import merge_ref as R

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "similari_amd" / "csrc"
STAGED, ZERO = 0x80000000, 0xFFFFFFFF
DRIVER = r"""
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include "sa_merge_plan.h"
// stdin, one case per line:
//   B keep C Kp slot old_n fresh n (src quality_bits){n}   ->  new_n quality_bits{Kp} nrows (dst src){nrows}
//   M T n removed{n}                                       ->  nperm perm{nperm} nmoves (from to){nmoves}
int main() {
  std::string tag;
  while (std::cin >> tag) {
    if (tag == "B") {
      uint32_t keep, C, Kp, slot, old_n, fresh, n;
      std::cin >> keep >> C >> Kp >> slot >> old_n >> fresh >> n;
      std::vector<SaMergeObs> bank(n);
      for (auto& o : bank) {
        uint32_t bits;
        std::cin >> o.src >> bits;
        std::memcpy(&o.quality, &bits, 4);
      }
      std::vector<SaMergeRow> rows;
      std::vector<float> q(Kp, -1.f);
      const uint32_t m = sa_merge_plan_bank(keep, C, Kp, slot, old_n, fresh != 0, bank, rows, q.data());
      std::printf("%u", m);
      for (float x : q) {
        uint32_t bits;
        std::memcpy(&bits, &x, 4);
        std::printf(" %u", bits);
      }
      std::printf(" %zu", rows.size());
      for (const auto& r : rows) std::printf(" %u %u", r.dst, r.src);
      std::printf("\n");
    } else if (tag == "M") {
      uint32_t T, n;
      std::cin >> T >> n;
      std::vector<uint32_t> removed(n), perm;
      for (auto& r : removed) std::cin >> r;
      std::vector<SaMergeMove> moves;
      sa_merge_compaction(T, removed, perm, moves);
      std::printf("%zu", perm.size());
      for (uint32_t p : perm) std::printf(" %u", p);
      std::printf(" %zu", moves.size());
      for (const auto& m : moves) std::printf(" %u %u", m.from, m.to);
      std::printf("\n");
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
    d = tmp_path_factory.mktemp("merge_plan")
    (d / "drv.cpp").write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", str(CSRC), str(d / "drv.cpp"), "-o", str(d / "drv")], check=True)

    def run(lines):
        out = subprocess.run([str(d / "drv")], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        res = [[int(x) for x in line.split()] for line in out.splitlines()]
        assert len(res) == len(lines)
        return res

    return run


def bits(q):
    return int(np.float32(q).view(np.uint32))


QUALITIES = np.array([0.0, -0.0, 1.0, 1.0, 2.5, -3.0, np.inf, -np.inf, 0.25], np.float32)   # tied, +-0, infinite


def bank_cases(K, seed, count):
    """Random stores of a few tracks whose rows are numbered (0 = a zero row), one append or merge into one destination each.
    -> per case: (driver line, device array before, what the bank must hold afterwards, the destination's slot, the staged rows)"""
    rng = np.random.default_rng(seed)
    Kp = 1
    while Kp < K:
        Kp *= 2
    cases = []
    for c in range(count):
        T = int(rng.integers(1, 6))
        dev = np.zeros(T * Kp, np.int64)
        qual = np.zeros(T * Kp, np.float32)
        nobs = rng.integers(0, K + 1, T)
        if c % 7 == 0:
            nobs[:] = K   # full banks: everything competes
        for t in range(T):
            for k in range(nobs[t]):
                dev[t * Kp + k] = 1000 * (t + 1) + k
                qual[t * Kp + k] = rng.choice(QUALITIES)
        keep = int(rng.integers(2))
        C = int(rng.integers(1, K + 1))
        slot = int(rng.integers(T))
        own = [(slot * Kp + k, qual[slot * Kp + k]) for k in range(nobs[slot])]
        staged = []
        fresh = 0
        if rng.integers(2):   # merge: some other tracks as sources, in a random order
            others = [t for t in rng.permutation(T) if t != slot][: int(rng.integers(0, T))]
            extra = [(t * Kp + k, qual[t * Kp + k]) for t in others for k in range(nobs[t])]
        else:                 # append: 1..K staged rows, now and then into a slot that is new and holds anything
            n_new = int(rng.integers(1, K + 1))
            base = int(rng.integers(0, 50))
            staged = {base + k: 500000 + k for k in range(n_new)}
            extra = [(STAGED | (base + k), rng.choice(QUALITIES)) for k in range(n_new)]
            if rng.integers(4) == 0:
                fresh, own = 1, []
                dev[slot * Kp: (slot + 1) * Kp] = -7   # garbage: every row of a fresh slot must be written
                nobs[slot] = 0
        entries = own + extra
        name = lambda s: staged[s & ~STAGED] if s & STAGED else int(dev[s])
        want = R.optimize([(name(s), np.float32(q)) for s, q in entries], (R.LATEST, R.BEST)[keep], C)
        line = " ".join(["B", str(keep), str(C), str(Kp), str(slot), str(int(nobs[slot])), str(fresh), str(len(entries))] +
                        [f"{s} {bits(q)}" for s, q in entries])
        cases.append((line, dev, want, slot, staged, Kp))
    return cases


@pytest.mark.parametrize("K", [1, 3, 5, 32])
def test_planned_banks_equal_the_restatement(drv, K):
    cases = bank_cases(K, 1000 + K, 400)
    permuted = zeroed = skipped = 0
    for (line, dev, want, slot, staged, Kp), out in zip(cases, drv([c[0] for c in cases])):
        m, q, nrows = out[0], out[1: 1 + Kp], out[1 + Kp]
        rows = np.array(out[2 + Kp:], np.int64).reshape(nrows, 2)
        assert m == len(want)
        assert q[:m] == [bits(x) for _, x in want] and all(x == 0 for x in q[m:])
        dsts = rows[:, 0]
        assert len(set(dsts.tolist())) == nrows and np.all(dsts // Kp == slot)   # one writer per slot, all inside the bank
        stage = [0 if s == ZERO else staged[s & ~STAGED] if s & STAGED else int(dev[s]) for s in rows[:, 1].tolist()]   # gather ...
        after = dev.copy()
        after[dsts] = stage                                                                                                # ... then scatter
        assert after[slot * Kp: slot * Kp + m].tolist() == [n for n, _ in want]
        assert np.all(after[slot * Kp + m: (slot + 1) * Kp] == 0)
        untouched = np.ones(len(dev), bool)
        untouched[slot * Kp: (slot + 1) * Kp] = False
        assert np.array_equal(after[untouched], dev[untouched])
        own_src = [(d, s) for d, s in rows.tolist() if s != ZERO and not s & STAGED and s // Kp == slot]
        permuted += any(d != s for d, s in own_src)
        zeroed += bool((rows[:, 1] == ZERO).any())
        skipped += nrows < Kp
    # the cases reach what they are for (one slot per bank can neither permute nor lose a row: something always fills it)
    assert skipped and (K == 1 or (zeroed and permuted))


def test_a_reversal_and_an_interleave_by_hand(drv):
    """K = 4 at slot 2, ascending qualities under BEST: the bank reverses through rows that read each other; with one better foreign
    row the own rows shift by one and the worst one goes."""
    asc = [(8 + k, float(k)) for k in range(4)]
    line = lambda entries, C: " ".join(["B 1", str(C), "4 2 4 0", str(len(entries))] + [f"{s} {bits(q)}" for s, q in entries])
    (rev, mix) = drv([line(asc, 4), line(asc + [(0, 2.5)], 4)])
    assert rev[0] == 4 and rev[5] == 4 and rev[6:] == [8, 11, 9, 10, 10, 9, 11, 8]
    assert mix[0] == 4 and [bits(x) for x in (3.0, 2.5, 2.0, 1.0)] == mix[1:5]
    assert mix[5] == 3 and mix[6:] == [8, 11, 9, 0, 11, 9]   # slot 10 keeps its row: three rows move


def sequential_remove(T, removed):
    """sa_store_remove one id at a time: the last track moves into the hole.  -> final slot -> original slot"""
    at = list(range(T))
    for o in removed:
        p = at.index(o)
        at[p] = at[-1]
        at.pop()
    return at


def test_compaction_moves_equal_sequential_removal(drv):
    rng = np.random.default_rng(77)
    cases = [(1, [0]), (2, [1]), (2, [0]), (2, [0, 1]), (2, [1, 0]), (5, []), (6, [5, 0]), (6, [0, 5]), (6, [3, 4, 5]), (6, [5, 4, 3]),
             (6, [0, 1, 2, 3]), (6, [1, 2, 3, 4, 5]), (6, [5, 4, 3, 2, 1, 0])]
    for _ in range(600):
        T = int(rng.integers(1, 70))
        cases.append((T, rng.permutation(T)[: int(rng.integers(0, T + 1))].tolist()))
    outs = drv([" ".join(["M", str(T), str(len(rem))] + [str(r) for r in rem]) for T, rem in cases])
    chained = 0
    for (T, rem), out in zip(cases, outs):
        n = out[0]
        perm, nm = out[1: 1 + n], out[1 + n]
        moves = np.array(out[2 + n:], np.int64).reshape(nm, 2)
        assert n == T - len(rem) and perm == sequential_remove(T, rem)
        assert sorted(moves[:, 1].tolist()) == [p for p in range(n) if perm[p] != p]
        assert all(perm[to] == frm for frm, to in moves.tolist())
        # the range property: sources at or beyond the final count, targets below it, no source twice — one launch can run them all
        assert np.all(moves[:, 0] >= n) and np.all(moves[:, 1] < n) and len(set(moves[:, 0].tolist())) == nm
        # a sequential removal may move a track twice (into a hole that is removed later); the net move is one
        steps, at = 0, list(range(T))
        for o in rem:
            p = at.index(o)
            steps += p != len(at) - 1
            at[p] = at[-1]
            at.pop()
        chained += steps > nm
    assert chained
