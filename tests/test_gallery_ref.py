"""The gallery yardstick (tests/gallery_ref.py) on hand-made cases: withdrawal, joins of nothing, unknown ids."""
import numpy as np

import gallery_ref as G

NAN = float("nan")


def matrix(T, pairs, K=1):
    """[T][K][T][K] with the given symmetric distances at observation (0, 0), zeros on the diagonal, NaN elsewhere."""
    c = np.full((T, K, T, K), NAN, np.float32)
    for t in range(T):
        c[t, 0, t, 0] = 0.0
    for (a, b), d in pairs.items():
        c[a, 0, b, 0] = c[b, 0, a, 0] = d
    return c


def test_a_withdrawn_pair_does_not_raise_m():
    s_ids = [1, 2, 3]
    full = matrix(3, {(0, 1): 9.0, (0, 2): 0.2, (1, 2): 0.3})
    cells = G.rows_of(s_ids, full, [1, 2])
    left, M = G.search_stored(s_ids, cells, [1, 2], 5, 1.0)
    assert M == np.float32(9.0)
    assert left == {1: [(3, float(np.float32(9.0) - np.float32(0.2)))], 2: [(3, float(np.float32(9.0) - np.float32(0.3)))]}
    out, M = G.search_stored(s_ids, cells, [1, 2], 5, 1.0, withdraw=True)
    assert M == np.float32(0.3)
    assert out == {1: [(3, float(np.float32(0.3) - np.float32(0.2)))], 2: [(3, 0.0)]}
    # with the threshold open the withdrawn pair still forms no group
    out, _ = G.search_stored(s_ids, cells, [1, 2], 5, 100.0, withdraw=True)
    assert all(w not in (1, 2) for lst in out.values() for w, _ in lst)
    both, _ = G.search_stored(s_ids, cells, [1, 2], 5, 100.0)
    assert [w for w, _ in both[1]] == [3, 2] and both[1][1][1] == 0.0


def test_withdrawing_every_track_leaves_nothing():
    s_ids = [4, 5]
    full = matrix(2, {(0, 1): 0.1})
    res, M = G.search_stored(s_ids, full, s_ids, 5, 1.0, withdraw=True)
    assert res == {} and M == np.float32(-1.0)


def test_a_join_of_one_track_or_of_none_has_no_winners():
    assert G.join([7], matrix(1, {}), 5, 1.0) == ({}, np.float32(-1.0))
    assert G.join([], np.zeros((0, 1, 0, 1), np.float32), 5, 1.0) == ({}, np.float32(-1.0))
    assert G.surviving_pairs([7], matrix(1, {}), 1.0) == set()


def test_an_unknown_id_gives_an_empty_row():
    s_ids = [1, 2, 3]
    full = matrix(3, {(0, 1): 0.5, (0, 2): 0.2, (1, 2): 0.3})
    cells = G.rows_of(s_ids, full, [2, 99])
    assert np.isnan(cells[1]).all() and np.array_equal(cells[0], full[1], equal_nan=True)
    res, M = G.search_stored(s_ids, cells, [2, 99], 5, 1.0)
    assert 99 not in res and M == np.float32(0.5)
    assert [w for w, _ in res[2]] == [3, 1]


def test_the_join_is_the_stored_search_over_the_order():
    rng = np.random.default_rng(3)
    T, K = 9, 2
    d = rng.uniform(0, 1, (T, K, T, K)).astype(np.float32)
    full = ((d + d.transpose(2, 3, 0, 1)) / 2).astype(np.float32)
    s_ids = np.arange(11, 11 + T)
    a = G.join(s_ids, full, 3, 0.4, 2)
    b = G.search_stored(s_ids, G.rows_of(s_ids, full, s_ids), s_ids, 3, 0.4, 2)
    assert a == b and a[0]
    pairs = G.surviving_pairs(s_ids, full, 0.4, 2)
    full_res, _ = G.join(s_ids, full, G.ALL, 0.4, 2)
    assert 2 * len(pairs) == sum(len(v) for v in full_res.values())
