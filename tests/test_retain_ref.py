"""tests/retain_ref.py, what the GPU tests of sa_store_absorb_keep lean on: ranks(), the rank formula k_absorb_move_best runs per lane,
held to merge_ref.optimize's stable sort; and the model under "keep the best" held to the rule of examples/track_merging.rs:279-297
(sort by quality descending, truncate to a capacity that grows with the merges) on a short drifting-identity scenario."""
import numpy as np
import pytest

import merge_ref as M
import retain_ref as R

f32 = np.float32


def order_of_optimize(q):
    """The bank order merge_ref.optimize(BEST) leaves, as indices into q (the "row" of observation i is i itself)."""
    return [row for row, _ in M.optimize([(i, f32(x)) for i, x in enumerate(q)], M.BEST, len(q))]


def holds(q):
    q = np.asarray(q, f32)
    rk = R.ranks(q)
    assert sorted(rk.tolist()) == list(range(len(q)))           # a permutation: every position has exactly one source
    order = order_of_optimize(q)
    assert [int(np.flatnonzero(rk == p)[0]) for p in range(len(q))] == order
    for C in {1, (len(q) + 1) // 2, len(q)}:                        # the cut keeps the observations of rank < C, in rank order
        assert [row for row, _ in M.optimize([(i, x) for i, x in enumerate(q)], M.BEST, C)] == order[:C]


@pytest.mark.parametrize("n", range(1, 65))
def test_ranks_is_the_stable_sort_by_quality_descending(n):
    """Every length a wave can hold, one observation per lane: random, all equal, tie-heavy (three values), signed zeros and
    infinities."""
    rng = np.random.default_rng(n)
    holds(rng.uniform(0, 1, n))
    holds(np.full(n, 0.5))
    holds(rng.choice([0.25, 0.5, 0.75], n))
    holds(rng.choice([0.0, -0.0], n))                              # all equal in the compare: the bank order stays
    holds(rng.choice([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0], n))
    holds(np.sort(rng.uniform(0, 1, n)))                           # ascending: fully reversed
    holds(-np.sort(-rng.uniform(0, 1, n)))                         # sorted already: the identity


def test_signed_zeros_tie_and_keep_their_order():
    assert R.ranks([0.0, -0.0, 0.0, -0.0]).tolist() == [0, 1, 2, 3]
    assert R.ranks([-0.0, 1.0, 0.0, -np.inf, np.inf]).tolist() == [2, 1, 3, 4, 0]


def test_two_drifting_identities_keep_their_best_observations():
    """track_merging.rs's optimize() per frame on the incremental loop: two identities drift from (0, 0) and (1, 1), every frame brings
    one observation of each under a fresh id with a random quality, the capacity is growth_capacity(frame) (4, 6, 9, 12, 12, ..).
    After every frame each track holds its identity's best min(seen, capacity) observations so far, best first, the earlier of
    equals first — and a dropped observation never returns."""
    rng = np.random.default_rng(11)
    K = 12
    m = R.Model(K, 2, "euclidean")
    pos = [np.array([0.0, 0.0], f32), np.array([1.0, 1.0], f32)]
    kept = [[], []]   # per identity: the (quality, -arrival, row) still held, as the reference's sort-then-truncate leaves them
    next_id = 100
    for frame in range(9):
        cap = M.growth_capacity(frame)
        ids, feats, qual = [], [], []
        for k in range(2):
            pos[k] = (pos[k] + rng.uniform(-0.01, 0.01, 2).astype(f32)).astype(f32)
            x = f32(rng.choice([0.2, 0.5, 0.8])) if frame % 2 else f32(rng.uniform(0, 1))   # ties every other frame
            ids.append(next_id)
            next_id += 1
            feats.append(pos[k].reshape(1, 2))
            qual.append([x])
            kept[k] = sorted(kept[k] + [(x, -frame, pos[k].copy())], key=lambda o: (-o[0], -o[1]))[:cap]
        res, dest = m.absorb(ids, feats, 1, 0.1, keep_below=0.1, quality=qual, capacity=cap, keep=M.BEST)
        assert dest == ({100: 100, 101: 101} if frame == 0 else {ids[0]: 100, ids[1]: 101})
        for k, t in enumerate((100, 101)):
            assert m.quality(t).tolist() == [o[0] for o in kept[k]]
            assert np.array_equal(m.feats(t), np.stack([o[2] for o in kept[k]]))
    assert m.order == [100, 101] and [len(m.banks[t]) for t in m.order] == [9, 9]


def test_keep_latest_through_the_model_is_absorb_ref():
    import absorb_ref as A

    rng = np.random.default_rng(3)
    a, b = R.Model(3, 4, "euclidean"), A.Model(3, 4, "euclidean")
    rows = [rng.uniform(-1, 1, (2, 4)).astype(f32) for _ in range(3)]
    for m in (a, b):
        m.upsert([1, 2, 3], rows)
    q = [rows[0][:1] + f32(0.01), rng.uniform(5, 6, (3, 4)).astype(f32)]
    qual = [[0.9], [0.1, 0.5, 0.3]]
    assert a.absorb([7, 8], q, 1, 0.5, quality=qual, capacity=2, keep=M.LATEST) == b.absorb([7, 8], q, 1, 0.5, quality=qual, capacity=2)
    assert a.order == b.order and all(np.array_equal(a.feats(t), b.feats(t)) and np.array_equal(a.quality(t), b.quality(t)) for t in a.order)
