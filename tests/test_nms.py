"""Non-maximum suppression (src/utils/nms.rs:32-72).

cpu : the oracle's or_nms on the reference's own examples — the (disabled) unit test of nms.rs:142-156 and the doc example of
      utils/nms/nms_py.rs:24-37 — and on properties that follow from the algorithm.
gpu : sa_nms through the C ABI returns exactly the oracle's indices, in the same order, for axis-aligned and oriented boxes,
      with and without scores, on dense random scenes up to the reference bench size (benches/nms.rs: 1000 boxes) — all of which the
      one-word sweep k_nms_sweep<1> takes — and on chain scenes of 4096, 4097, 8192, 8193 and 16384 boxes, which run the sweep's
      three classes <1>, <2> and <4> up to the ceiling of 16384 boxes; one box more is refused.
cpu : the chain scenes themselves: the ranks fall in the 4096-rank blocks they were planted in and the oracle keeps A and C of
      every chain and drops B."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from similari_amd import abi, synth


def xyaah(xc, yc, aspect, h, angle=None):
    return abi.make_boxes([xc], [yc], [aspect], [h], angle=None if angle is None else [angle])[0]


def test_reference_unit_example():
    # nms.rs:145-151: three concentric boxes and one apart, threshold 0.8, no scores -> rank = height
    b = np.array([xyaah(0, 0, 1.0, 5.0), xyaah(0, 0, 1.05, 5.1), xyaah(0, 0, 1.0, 4.9), xyaah(3, 4, 1.0, 4.5)], abi.BOX_DTYPE)
    keep = O.nms(b, None, 0.8, None)
    # visited by height: #1 (5.1) suppresses #0 (25 / 25 = 1.0) and #2 (24.01 / 24.01); #3 overlaps #1 by 2.85 x 1.35 / 20.25 = 0.19
    assert keep.tolist() == [1, 3]


def test_reference_doc_example():
    # nms_py.rs:24-37 — ltwh boxes (10, 11, 3, 3.8) score 1.0 and (10.3, 11.1, 2.9, 3.9) score 0.9; the second is suppressed
    b = np.concatenate([abi.ltwh([10.3], [11.1], [2.9], [3.9]), abi.ltwh([10.0], [11.0], [3.0], [3.8])])
    assert O.nms(b, [0.9, 1.0], 0.7, 0.0).tolist() == [1]
    # without scores the taller box ranks first (3.9 vs 4.0 in the doc's second call)
    b2 = np.concatenate([abi.ltwh([10.3], [11.1], [2.9], [3.9]), abi.ltwh([10.0], [11.0], [3.0], [4.0])])
    assert O.nms(b2, None, 0.7, 0.0).tolist() == [1]


def test_filters_and_order():
    rng = np.random.default_rng(0)
    b = synth.dense_boxes(rng, 40, (4000.0, 4000.0))          # far apart: nothing is suppressed
    s = rng.uniform(0, 1, 40).astype(np.float32)
    keep = O.nms(b, s, 0.5, 0.3)
    assert set(keep.tolist()) == set(np.nonzero(s > 0.3)[0].tolist())
    assert (np.diff(s[keep]) <= 0).all(), "output is in descending rank"
    # equal ranks keep their input order (stable sort)
    s2 = np.full(40, 0.5, np.float32)
    assert O.nms(b, s2, 0.5, None).tolist() == list(range(40))
    # NaN score = None: passes any threshold, ranks by height
    s3 = s.copy(); s3[::3] = np.nan
    k3 = O.nms(b, s3, 0.5, 0.99)
    assert set(k3.tolist()) >= set(range(0, 40, 3))


def scene(rng, n, oriented):
    b = synth.dense_boxes(rng, n, (1200.0, 800.0), oriented=oriented)
    # clusters of near-duplicates, as a detector emits them
    dup = synth.jitter_boxes(rng, b[: n // 2], 3.0, size_rel=0.05, angle_sigma=0.05 if oriented else 0.0)
    return np.concatenate([b, dup])[rng.permutation(n + n // 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("oriented", [False, True])
@pytest.mark.parametrize("n", [1, 17, 200, 1000])
@pytest.mark.parametrize("with_scores", [False, True])
def test_gpu_nms_matches_oracle(oriented, n, with_scores):
    from similari_amd.engine import Engine

    rng = np.random.default_rng(1000 * oriented + n + with_scores)
    b = scene(rng, n, oriented)
    s = rng.uniform(0, 1, len(b)).astype(np.float32) if with_scores else None
    if with_scores:
        s[::7] = np.nan
    eng = Engine(abi.make_config())
    try:
        for thr, sthr in ((0.5, None), (0.3, 0.2), (0.8, None), (-1.0, None)):
            got = eng.nms(b, s, thr, sthr)
            want = O.nms(b, s, thr, sthr)
            np.testing.assert_array_equal(got, want)
        if n >= 200:
            assert len(want) < len(b), "the duplicates must be suppressed at some threshold"
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_nms_edge_cases():
    from similari_amd.engine import Engine

    eng = Engine(abi.make_config())
    try:
        assert eng.nms(np.zeros(0, abi.BOX_DTYPE)).tolist() == []
        b = np.array([xyaah(0, 0, 1.0, 5.0), xyaah(0, 0, 1.0, 5.0)], abi.BOX_DTYPE)
        assert eng.nms(b, None, 0.5, None).tolist() == [0]           # identical boxes: the first one stays
        assert eng.nms(b, None, 1.0, None).tolist() == [0, 1]        # metric 1.0 is not > 1.0
        assert eng.nms(b, [0.1, 0.9], 0.5, 0.5).tolist() == [1]
        assert eng.nms(b, [0.1, 0.2], 0.5, 0.5).tolist() == []
    finally:
        eng.close()


# ---- the sweep's other classes: chain scenes of 4096 .. 16384 boxes ----------------------------------------------------------
# k_nms_sweep<S> keeps the removed-bitmap as S words per lane: the bit of rank i lives in word i >> 6, which lane (i >> 6) & 63 holds in
# its slot i >> 12.  A 4096-rank BLOCK is one slot.  A chain is three equal boxes A, B, C in a row, B shifted by 0.4 of the width from
# A and C by 0.8: the metric (w - shift) / w is 0.6 between neighbours and 0.2 between A and C, so at threshold 0.5 A removes B, and B
# — removed — must not remove C.  The sweep gets that right only if it reads B's bit from the slot B's rank lies in and finds C's
# row untouched: with A, B and C planted in chosen blocks, a lane that reads the wrong slot keeps B or loses C.
# At 4097 and 8193 boxes the last block is ONE rank.  A kept box there (the C of a chain) would show nothing: a lane that reads another
# slot for it finds a clear bit too.  That rank goes to the B of a two-box chain whose A lies one block lower: it is removed through the
# last slot and read back from it.
NMS_BLOCK = 4096
NMS_SIZES = [4096, 4097, 8192, 8193, 16384]   # last size of <1> (W = 64) | <2>, lane 0 alone holds a second word | <2> full | <4>, S = 3 | the ceiling, W = 256
NAN_RANKS = 512                               # scenes with scores: the first ranks belong to boxes without a score (rank = height > every score)


def chain_plan(n):
    """The chains to plant at n boxes, as the blocks of their members: every triple (bA <= bB <= bC) of the blocks that hold more than
    one rank, triples of more different blocks first; a last block of one rank takes the B of a pair (bA, bB) instead."""
    nb = -(-n // NMS_BLOCK)
    room = [min(NMS_BLOCK, n - b * NMS_BLOCK) for b in range(nb)]
    room[0] -= NAN_RANKS
    plan = []
    if room[-1] == 1:
        plan.append((nb - 2, nb - 1))
        room[-2] -= 1
        room[-1] -= 1
    triples = [(a, b, c) for a in range(nb) for b in range(a, nb) for c in range(b, nb)]
    triples.sort(key=lambda t: -len(set(t)))
    for t in triples:
        need = {b: t.count(b) for b in set(t)}
        if all(room[b] - need[b] >= 0 for b in need):
            for b in need:
                room[b] -= need[b]
            plan.append(t)
    return plan


@functools.lru_cache(maxsize=None)
def chain_scene(n, oriented, with_scores):
    """n boxes: a sparse base set (one box per cell of a grid: nothing overlaps), near-duplicates of a sixteenth of them at random
    ranks, and the chains of chain_plan(n).  With scores the input order is shuffled, the scores fall from 1.0 to 0.2 along the ranks
    and the first NAN_RANKS ranks have no score (NaN) and descending heights; without scores all heights are equal, so the stable sort
    leaves the input order as the rank order.  Returns (boxes, scores | None, chains [((iA, iB[, iC]), (bA, bB[, bC]))])."""
    rng = np.random.default_rng(7 * n + 2 * oriented + with_scores)
    plan = chain_plan(n)
    n_dup = n // 16
    n_base = n - sum(len(t) for t in plan) - n_dup
    # ranks: the chains' first (drawn inside their blocks), the rest to base boxes and duplicates at random
    free = np.ones(n, bool)
    chain_ranks = []
    for t in plan:
        rk = []
        for b in t:
            lo, hi = b * NMS_BLOCK + (NAN_RANKS if b == 0 else 0), min(n, (b + 1) * NMS_BLOCK)
            cand = np.nonzero(free[lo:hi])[0] + lo
            r = int(rng.choice(cand))
            free[r] = False
            rk.append(r)
        chain_ranks.append(sorted(rk))                         # bA <= bB <= bC: sorting keeps every member in its block
    rest = np.nonzero(free)[0]
    rest = np.concatenate([rest[rest < NAN_RANKS], rng.permutation(rest[rest >= NAN_RANKS])])
    base_ranks, dup_ranks = rest[:n_base], rest[n_base:]      # (the ranks without a score all go to base boxes)
    cells = n_base + len(plan)
    side = int(np.ceil(np.sqrt(cells)))
    cell = rng.permutation(side * side)[:cells]
    cx, cy = (cell % side) * 100.0 + 50.0, (cell // side) * 100.0 + 50.0
    xc, yc, asp, hgt, ang = (np.zeros(n, np.float32) for _ in range(5))
    h0 = 24.0
    # base boxes
    xc[base_ranks], yc[base_ranks] = cx[:n_base], cy[:n_base]
    asp[base_ranks] = rng.uniform(0.5, 1.5, n_base)
    hgt[base_ranks] = rng.uniform(20.0, 28.0, n_base) if with_scores else h0
    ang[base_ranks] = rng.uniform(-3.0, 3.0, n_base)
    if with_scores:
        hgt[:NAN_RANKS] = 40.0 - 10.0 * np.arange(NAN_RANKS) / NAN_RANKS
    # near-duplicates of base boxes
    src = base_ranks[rng.choice(n_base, n_dup, replace=False)]
    xc[dup_ranks], yc[dup_ranks] = xc[src] + rng.normal(0, 3.0, n_dup), yc[src] + rng.normal(0, 3.0, n_dup)
    asp[dup_ranks], ang[dup_ranks] = asp[src] * rng.uniform(0.95, 1.05, n_dup), ang[src] + (rng.normal(0, 0.05, n_dup) if oriented else 0.0)
    hgt[dup_ranks] = hgt[src] * rng.uniform(0.95, 1.05, n_dup) if with_scores else h0
    # chains: equal boxes, shifted along their own width axis
    for k, rk in enumerate(chain_ranks):
        a, h, th = rng.uniform(0.8, 1.5), (rng.uniform(20.0, 28.0) if with_scores else h0), (rng.uniform(-3.0, 3.0) if oriented else 0.0)
        for r, shift in zip(rk, (-0.4, 0.0, 0.4)):
            xc[r] = cx[n_base + k] + shift * a * h * np.cos(th)
            yc[r] = cy[n_base + k] + shift * a * h * np.sin(th)
            asp[r], hgt[r], ang[r] = a, h, th
    boxes = abi.make_boxes(xc, yc, asp, hgt, angle=ang if oriented else None)
    if not with_scores:
        return boxes, None, [(tuple(rk), t) for rk, t in zip(chain_ranks, plan)]
    scores = (1.0 - 0.8 * np.arange(n) / n).astype(np.float32)
    scores[:NAN_RANKS] = np.nan
    p = rng.permutation(n)                                     # input position p[r] holds the box of rank r
    inv = np.empty(n, np.int64)
    inv[p] = np.arange(n)
    return boxes[inv], scores[inv], [(tuple(int(p[r]) for r in rk), t) for rk, t in zip(chain_ranks, plan)]


@functools.lru_cache(maxsize=None)
def chain_oracle(n, oriented, with_scores, thr, sthr):
    b, s, _ = chain_scene(n, oriented, with_scores)
    return O.nms(b, s, thr, sthr)


def test_chain_plan():
    assert chain_plan(4096) == [(0, 0, 0)]
    assert chain_plan(4097) == [(0, 1), (0, 0, 0)]                          # block 1 is one rank: the B of a pair
    assert set(chain_plan(8192)) == {(0, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1)}
    assert chain_plan(8193)[0] == (1, 2) and set(chain_plan(8193)[1:]) == {(0, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1)}
    assert len(chain_plan(16384)) == 20 and {(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)} <= set(chain_plan(16384))


@pytest.mark.parametrize("with_scores", [False, True])
@pytest.mark.parametrize("oriented", [False, True])
@pytest.mark.parametrize("n", NMS_SIZES)
def test_chain_scenes_are_what_they_claim(n, oriented, with_scores):
    """Without a GPU: the ranks the reference's stable sort gives the chains' boxes fall in the blocks intended, A before B before C,
    and the oracle keeps A and C and drops B of every chain (A and B of a pair); the near-duplicates make it drop others too."""
    b, s, chains = chain_scene(n, oriented, with_scores)
    assert len(b) == n and len(chains) == len(chain_plan(n)) >= 1
    rank_value = b["height"] if s is None else np.where(np.isnan(s), b["height"], s)
    order = np.argsort(-rank_value.astype(np.float64), kind="stable")
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    keep = chain_oracle(n, oriented, with_scores, 0.5, None)
    kept = np.zeros(n, bool)
    kept[keep] = True
    np.testing.assert_array_equal(rank[keep], np.sort(rank[keep]))          # output in rank order
    for idx, t in chains:
        assert (np.diff(rank[list(idx)]) > 0).all()
        assert tuple(rank[list(idx)] // NMS_BLOCK) == t, (rank[list(idx)], t)
        assert kept[list(idx)].tolist() == [True, False, True][: len(idx)], (idx, t)
    if n % NMS_BLOCK == 1:
        assert rank[chains[0][0][1]] == n - 1 and not kept[chains[0][0][1]]      # the one rank of the last block: removed
    assert n - len(keep) > len(chains) + n // 64, "the duplicates must be suppressed too"
    if with_scores:
        assert np.isnan(s).sum() == NAN_RANKS and (rank[np.isnan(s)] < NAN_RANKS).all()


@pytest.mark.gpu
@pytest.mark.parametrize("with_scores", [False, True])
@pytest.mark.parametrize("oriented", [False, True])
@pytest.mark.parametrize("n", NMS_SIZES)
def test_gpu_nms_sweep_classes(n, oriented, with_scores):
    """sa_nms on the chain scenes equals the oracle, index for index: 4096 boxes run k_nms_sweep<1> at its last size (W = 64), 4097
    and 8192 run k_nms_sweep<2> (at 4097 lane 0 alone holds a second word), 8193 (S = 3: one empty word per lane) and 16384 (the
    ceiling, W = 256) run k_nms_sweep<4>.  With scores a second call drops the lower ranks at a score threshold, which moves every
    later box into another word."""
    from similari_amd.engine import Engine

    b, s, chains = chain_scene(n, oriented, with_scores)
    eng = Engine(abi.make_config())
    try:
        for thr, sthr in ((0.5, None), (0.3, 0.5)) if with_scores else ((0.5, None),):
            got = eng.nms(b, s, thr, sthr)
            want = chain_oracle(n, oriented, with_scores, thr, sthr)
            np.testing.assert_array_equal(got, want)
        kept = np.zeros(n, bool)
        kept[eng.nms(b, s, 0.5, None)] = True
        for idx, t in chains:
            assert kept[list(idx)].tolist() == [True, False, True][: len(idx)], (idx, t)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_nms_ceiling():
    """16385 boxes that all pass the filter are refused (SA_ERR_UNSUPPORTED, "at most 16384 boxes"); with one of them under the score
    threshold 16384 reach the pair stage and the result is the oracle's."""
    from similari_amd.engine import Engine, EngineError

    b, s, _ = chain_scene(16384, False, True)
    b = np.concatenate([b, abi.make_boxes([-500.0], [-500.0], [1.0], [24.0])])
    s = np.concatenate([s, np.array([0.1], np.float32)])
    eng = Engine(abi.make_config())
    try:
        with pytest.raises(EngineError) as err:
            eng.nms(b, s, 0.5, None)
        assert err.value.code == abi.SA_ERR_UNSUPPORTED and "at most 16384 boxes" in str(err.value)
        with pytest.raises(EngineError) as err:
            eng.nms(b, None, 0.5, None)
        assert err.value.code == abi.SA_ERR_UNSUPPORTED
        got = eng.nms(b, s, 0.5, 0.15)
        want = chain_oracle(16384, False, True, 0.5, None)          # the extra box is the last one and never passes: same indices
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(O.nms(b, s, 0.5, 0.15), want)
    finally:
        eng.close()
