"""The compatibility rule on the host: similari_amd/csrc/sa_compat.h is compiled with the host compiler behind a small driver and
compared with tests/compat_ref.py over every flag combination and the int64 extremes; then the model is held against the
reference's own assertions (src/track/store/store_tests.rs), with fixed timestamps in place of clocks."""
import itertools
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import compat_ref as X
import topn_ref as R

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "similari_amd" / "csrc"
DRIVER = r"""
#include <cstdio>
#include <iostream>
#include "sa_compat.h"
// stdin, one case per line: flags ready_at q.key q.start q.end t.key t.start t.end  ->  live, then the union (key start end) of q <- t
int main() {
  uint32_t flags;
  long long ready_at;
  unsigned long long qk, tk;
  long long qs, qe, ts, te;
  while (std::cin >> flags >> ready_at >> qk >> qs >> qe >> tk >> ts >> te) {
    const sa_track_attrs q{qk, qs, qe}, t{tk, ts, te};
    const sa_track_attrs u = sa_compat_union(q, t);
    std::printf("%d %llu %lld %lld\n", sa_compat_live(flags, ready_at, q, t) ? 1 : 0, (unsigned long long)u.key, (long long)u.start,
                (long long)u.end);
  }
  return 0;
}
"""
TIMES = [X.INT64_MIN, -1, 0, 1, 5, 6, X.INT64_MAX]


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("compat")
    (d / "drv.cpp").write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", str(CSRC), str(d / "drv.cpp"), "-o", str(d / "drv")], check=True)

    def run(lines):
        out = subprocess.run([str(d / "drv")], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        res = [[int(x) for x in line.split()] for line in out.splitlines()]
        assert len(res) == len(lines)
        return res

    return run


def test_the_header_is_the_model(drv):
    """All 16 flag words (the predicate itself knows no refusals), spans start <= end over the seven times, two keys, three values of
    ready_at; the union is checked along."""
    spans = [(s, e) for s in TIMES for e in TIMES if s <= e]
    cases = []
    for flags in range(16):
        for ready_at in (X.INT64_MIN, 5, X.INT64_MAX) if flags & X.ONLY_READY else (X.INT64_MAX,):
            for (qs, qe), (ts, te) in itertools.product(spans, spans):
                for tk in (7, 2**64 - 1):
                    cases.append((flags, ready_at, (7, qs, qe), (tk, ts, te)))
    outs = drv([f"{f} {r} {q[0]} {q[1]} {q[2]} {t[0]} {t[1]} {t[2]}" for f, r, q, t in cases])
    seen = set()
    for (f, r, q, t), out in zip(cases, outs):
        want = X.live(f, r, q, t)
        assert bool(out[0]) == want, (f, r, q, t)
        assert tuple(out[1:]) == X.merged_attrs(X.NO_RULE, q, [t])
        seen.add((f, want))
    assert seen == {(f, w) for f in range(16) for w in (False, True)} - {(0, False)}   # every flag word both ways (0 gates nothing)


def euclid_cells(q_feats, s_feats, K):
    """[Q][K][T][K] euclidean distances of ragged banks, NaN where an observation is absent"""
    cells = np.full((len(q_feats), K, len(s_feats), K), np.nan, np.float32)
    for i, a in enumerate(q_feats):
        for j, b in enumerate(s_feats):
            for x, u in enumerate(a):
                for y, v in enumerate(b):
                    cells[i, x, j, y] = np.sqrt(np.sum((np.float32(u) - np.float32(v)) ** 2, dtype=np.float32))
    return cells


RULE = (X.QUERY_FIRST, X.INT64_MAX)   # TimeAttrs::compatible, store_tests.rs:44-46


def test_general_ops():
    """store_tests.rs:241-292.  The stored track began at 100; the query ended at 50, then at 150 (incompatible: no distances, no
    errors), then — after the stored track got a second observation at 200 — at start - 1."""
    q_feats, s_feats = [[(1.0, 0.0)]], [[(0.0, 1.0)]]
    stored = [(0, 100, 100)]
    d = X.pairs([2], [1], euclid_cells(q_feats, s_feats, 2), RULE, [(0, 50, 50)], stored)
    assert len(d) == 1 and d[0][:2] == (2, 1) and abs(d[0][2] - math.sqrt(2.0)) < 1e-6
    assert X.pairs([2], [1], euclid_cells(q_feats, s_feats, 2), RULE, [(0, 50, 150)], stored) == []
    s_feats = [[(0.0, 1.0), (1.0, 1.0)]]
    stored = [(0, 100, 200)]
    assert X.pairs([2], [1], euclid_cells(q_feats, s_feats, 2), RULE, [(0, 50, 150)], stored) == []
    d = X.pairs([2], [1], euclid_cells(q_feats, s_feats, 2), RULE, [(0, 50, stored[0][1] - 1)], stored)
    assert len(d) == 2 and d[0][1] == 1 and abs(d[0][2] - math.sqrt(2.0)) < 1e-6 and abs(d[1][2] - 1.0) < 1e-6


def ready_at(now, baked_period):
    """TimeAttrs::baked (store_tests.rs:54-60): Ready when now >= baked_period + end_time, that is end_time <= now - baked_period"""
    return now - baked_period


def test_baked_similarity():
    """store_tests.rs:298-361, baked_period 10.  Foreign form at time 2: the stored track (ended at 1) is not baked yet.  Owned form at
    time 12 with track 1 withdrawn: track 1 is baked by now, track 0 (added at 12) is not — nothing in either."""
    cells = euclid_cells([[(0.66, 0.33)]], [[(0.0, 1.0)]], 1)
    only_baked = (X.QUERY_FIRST | X.ONLY_READY, ready_at(2, 10))
    assert X.pairs([2], [1], cells, only_baked, [(0, 1, 1)], [(0, 1, 1)]) == []
    assert len(X.pairs([2], [1], cells, RULE, [(0, 1, 1)], [(0, 1, 1)])) == 1   # the gate, not the rule, kept it out
    s_ids, s_attrs = [1, 0], [(0, 1, 1), (0, 12, 12)]
    cells = euclid_cells([[(0.0, 1.0)]], [[(0.0, 1.0)], [(0.0, 1.0)]], 1)
    only_baked = (X.QUERY_FIRST | X.ONLY_READY, ready_at(12, 10))
    res, M = X.search_stored(s_ids, cells, [1], only_baked, s_attrs, 5, math.inf, withdraw=True)
    assert res == {} and M == -1.0
    res, _ = X.search_stored(s_ids, cells, [1], RULE, s_attrs, 5, math.inf, withdraw=True)
    assert list(res) == [1] and [w for w, _ in res[1]] == [0]


def test_all_similarity():
    """store_tests.rs:364-425: the external track at 1, track 1 at 2 -> one distance; track 3 at 3, owned([1]) -> one distance."""
    cells = euclid_cells([[(0.66, 0.33)]], [[(0.0, 1.0)]], 1)
    assert len(X.pairs([2], [1], cells, RULE, [(0, 1, 1)], [(0, 2, 2)])) == 1
    s_ids, s_attrs = [1, 3], [(0, 2, 2), (0, 3, 3)]
    cells = euclid_cells([[(0.0, 1.0)]], [[(0.0, 1.0)], [(0.0, 1.0)]], 1)
    res, _ = X.search_stored(s_ids, cells, [1], RULE, s_attrs, 5, math.inf, withdraw=True)
    assert {q: [w for w, _ in lst] for q, lst in res.items()} == {1: [3]}
    res, _ = X.search_stored(s_ids, cells, [3], RULE, s_attrs, 5, math.inf, withdraw=True)   # 3 ended after 1 began: the other direction is dead
    assert res == {}


def test_a_dead_pair_with_the_largest_distance_changes_every_weight():
    """What a host-side filter of the plain call's winners gets wrong: M is taken over pairs the reference never sees."""
    rng = np.random.default_rng(5)
    Q, T, K = 4, 9, 3
    cells = rng.uniform(0.1, 1.0, (Q, K, T, K)).astype(np.float32)
    cells[2, 1, 6, 0] = 7.5   # the call's largest distance, in the pair (query 102, stored 6)
    q_ids, s_ids = np.arange(100, 100 + Q), np.arange(T) + 1
    q_attrs = [(1, 0, 10)] * Q
    s_attrs = [(1, 20, 30)] * T
    s_attrs[6] = (2, 20, 30)   # stored id 7 sits in column 6: another key, dead for every query
    rule = (X.SAME_KEY, X.INT64_MAX)
    plain, M_plain = R.restate(q_ids, s_ids, cells, T, 2.0)
    gated, M = X.restate(q_ids, s_ids, cells, rule, q_attrs, s_attrs, T, 2.0)
    assert M_plain == np.float32(7.5) and M < 1.0
    filtered = {q: [(w, x) for w, x in lst if w != 7] for q, lst in plain.items()}
    assert {q: [w for w, _ in lst] for q, lst in gated.items()} != {} and all(7 not in [w for w, _ in lst] for lst in gated.values())
    for q in gated:
        for (w, x), (w2, x2) in zip(sorted(gated[q]), sorted(filtered[q])):
            assert w == w2 and x != x2   # the same groups, every weight different
    # and the model is the reference's voting on the reference's distances
    want, M_ref = R.winners(X.pairs(q_ids, s_ids, cells, rule, q_attrs, s_attrs), T, 2.0)
    assert M_ref == M and want == gated


def test_dead_tiles_by_hand():
    """Kp = 8: a cosine tile holds 8 x 8 groups, a euclidean one 4 x 16.  20 queries x 40 stored tracks, the first 16 stored tracks
    under a key no query has: cosine column tiles 0 and 1 (tracks 0..15) die in all three row tiles; the euclidean column tile 0
    holds tracks 0..15 exactly."""
    q = [(1, 0, 1)] * 20
    s = [(9, 5, 6)] * 16 + [(1, 5, 6)] * 24
    rule = (X.SAME_KEY, X.INT64_MAX)
    assert X.dead_tiles("cosine", 8, rule, q, s) == (3 * 5, 3 * 2)
    assert X.dead_tiles("euclidean", 8, rule, q, s) == (5 * 3, 5 * 1)
    assert X.dead_tiles("cosine", 8, X.NO_RULE, q, s) == (15, 0)
    # join of the 40: 5 row tiles; cosine: 15 tiles on or above the diagonal; keys split 16 / 24, so tiles that pair only tracks
    # 0..15 with tracks 16..39 are dead: (0,2) (0,3) (0,4) (1,2) (1,3) (1,4)
    assert X.dead_tiles("cosine", 8, rule, s, s, join=True) == (15, 6)
    # Kp = 32, euclidean: tile (i = 3, j = 0) holds track 3 against tracks 0..3 — no group with q < t, nothing to do
    one = [(1, 0, 1)] * 4
    assert X.dead_tiles("euclidean", 32, X.NO_RULE, one, one, join=True) == (4, 1)


def test_merge_model():
    m = X.Model(2, 1)
    m.upsert([1, 2, 3, 4], [np.zeros((1, 1), np.float32)] * 4)
    assert m.attrs_in_order() == [X.ZERO] * 4
    m.set_attrs([1, 2, 3, 4], [(1, 0, 10), (1, 10, 20), (1, 5, 8), (2, 30, 40)])
    rule = (X.SAME_KEY | X.DISJOINT, X.INT64_MAX)
    with pytest.raises(X.Incompatible):
        m.copy().merge({1: [3]}, rule=rule)            # 5..8 lies inside 0..10
    with pytest.raises(X.Incompatible):
        m.copy().merge({1: [4]}, rule=rule)            # another key
    a = m.copy()
    a.merge({1: [2]}, rule=rule)
    assert a.attrs == {1: (1, 0, 20), 3: (1, 5, 8), 4: (2, 30, 40)} and a.order == [1, 4, 3]
    b = m.copy()
    b.set_attrs([3], [(1, 20, 25)])
    with pytest.raises(X.Incompatible):
        b.copy().merge({2: [3, 1]}, rule=(X.QUERY_FIRST, X.INT64_MAX))   # 3 is fine after 2; then 2 runs 10..25 and 1 began at 0
    b.merge({2: [3, 1]}, rule=X.NO_RULE)                                  # no bits: the union, no test
    assert b.attrs[2] == (1, 0, 25)
    c = m.copy()
    c.merge({1: [2]})                                                     # plain merge: the destination's attributes stay
    assert c.attrs[1] == (1, 0, 10) and 2 not in c.attrs
