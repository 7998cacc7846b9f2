"""The track-search yardstick (tests/topn_ref.py) pinned on the reference's own literals: TopNVoting's unit tests
(src/track/voting/topn.rs:146-279), the two calls of examples/simple.rs, and the edge cases of M and of self-exclusion."""
import math

import numpy as np

import oracle_lib as O
import topn_ref as R

NAN = float("nan")


def by_winner(res):
    return {q: sorted(v) for q, v in res.items()}


def test_default_voting_literals():
    v = dict(topn=5, max_distance=0.32, min_votes=1)
    assert R.winners([(0, 1, 0.2)], **v)[0] == {0: [(1, 0.0)]}
    assert R.winners([(0, 1, 0.2), (0, 1, 0.3)], **v)[0] == {0: [(1, 0.10000000894069672)]}
    assert R.winners([(0, 1, 0.2), (0, 1, 0.4)], **v)[0] == {0: [(1, 0.20000000298023224)]}
    assert by_winner(R.winners([(0, 1, 0.2), (0, 2, 0.2)], **v)[0]) == {0: [(1, 0.0), (2, 0.0)]}
    m = [(0, 1, 0.2), (0, 1, 0.22), (0, 2, 0.21), (0, 2, 0.2), (0, 3, 0.22), (0, 3, 0.2),
         (0, 4, 0.23), (0, 4, 0.3), (0, 5, 0.24), (0, 5, 0.3), (0, 6, 0.25), (0, 6, 0.5)]
    res, M = R.winners(m, **v)
    assert M == np.float32(0.5)
    assert by_winner(res) == {0: [(1, 0.5800000131130219), (2, 0.5900000333786011), (3, 0.5800000131130219),
                                  (4, 0.4699999690055847), (5, 0.4599999785423279)]}
    # the engine's own order: weight descending, then id ascending — 6 (0.25) is the one truncated
    assert [w for w, _ in res[0]] == [2, 1, 3, 4, 5]


def test_two_query_vecs_literals():
    """Query 0's weights come from query 7's 0.5: M is one number for the whole call."""
    m = [(0, 1, 0.2), (0, 1, 0.22), (0, 2, 0.21), (0, 2, 0.2), (0, 3, 0.22), (0, 3, 0.2),
         (7, 4, 0.23), (7, 4, 0.3), (7, 5, 0.24), (7, 5, 0.3), (7, 6, 0.25), (7, 6, 0.5)]
    res, _ = R.winners(m, topn=5, max_distance=0.32, min_votes=1)
    assert by_winner(res) == {0: [(1, 0.5800000131130219), (2, 0.5900000333786011), (3, 0.5800000131130219)],
                              7: [(4, 0.4699999690055847), (5, 0.4599999785423279), (6, 0.25)]}


def test_weights_need_the_f32_subtraction():
    """c * M - sum(d) in f64 does not give the reference's literals."""
    ds = [0.2, 0.22]
    naive = 2 * float(np.float32(0.5)) - sum(float(np.float32(d)) for d in ds)
    assert naive != 0.5800000131130219
    assert R.winners([(0, 1, d) for d in ds] + [(0, 9, 0.5)], 5, 0.32)[0][0][0] == (1, 0.5800000131130219)


def cells_of(q_feats, s_feats, metric):
    """[Q][K][T][K] oracle distances (NaN where absent) of lists of per-track observation arrays."""
    L = O.lib()
    K = max([len(f) for f in q_feats + s_feats] + [1])
    out = np.full((len(q_feats), K, len(s_feats), K), np.nan, np.float32)
    fn = L.or_cosine if metric == "cosine" else L.or_euclidean
    for qi, qf in enumerate(q_feats):
        for ti, sf in enumerate(s_feats):
            for a, x in enumerate(qf):
                for b, y in enumerate(sf):
                    xa = np.zeros(8 * L.or_feature_blocks(len(x)), np.float32)
                    ya = np.zeros(8 * L.or_feature_blocks(len(y)), np.float32)
                    bx = L.or_feature_pad(O.fptr(np.asarray(x, np.float32)), len(x), O.fptr(xa))
                    by = L.or_feature_pad(O.fptr(np.asarray(y, np.float32)), len(y), O.fptr(ya))
                    out[qi, a, ti, b] = fn(O.fptr(xa), bx, O.fptr(ya), by)
    return out


def test_examples_simple_rs():
    """examples/simple.rs: store {0: [(1, 0)], 1: [(0.9, 0.1)]}, query 2: [(0.66, 0.33)], euclidean."""
    cells = cells_of([[(0.66, 0.33)]], [[(1.0, 0.0)], [(0.9, 0.1)]], "euclidean")
    res, M = R.restate([2], [0, 1], cells, topn=2, max_distance=1.0)
    assert [w for w, _ in res[2]] == [1, 0]
    assert M == cells[0, 0, 0, 0] and res[2][1][1] == 0.0
    res, _ = R.restate([2], [0, 1], cells, topn=2, max_distance=0.4)
    assert [w for w, _ in res[2]] == [1]


def test_self_pair_never_becomes_m():
    cells = np.array([5.0, 0.1], np.float32).reshape(1, 1, 2, 1)   # query 3 against stored 3 (5.0) and 4 (0.1)
    res, M = R.restate([3], [3, 4], cells, topn=5, max_distance=1.0)
    assert M == np.float32(0.1) and res == {3: [(4, 0.0)]}
    assert R.winners(R.pair_metrics([3], [3, 4], cells), 5, 1.0)[0] == res


def test_nan_cell_neither_raises_m_nor_is_kept():
    cells = np.array([NAN, 0.3, 0.2, NAN], np.float32).reshape(1, 2, 1, 2)
    res, M = R.restate([1], [2], cells, topn=5, max_distance=1.0, min_votes=3)
    assert M == np.float32(0.3) and res == {}
    res, _ = R.restate([1], [2], cells, topn=5, max_distance=1.0, min_votes=2)
    assert res == {1: [(2, 0.0 + float(np.float32(0.3) - np.float32(0.2)))]}


def test_min_votes_zero_is_one_and_keep_below_drops_before_m():
    cells = np.array([0.2, 0.9], np.float32).reshape(1, 1, 2, 1)
    for mv in (0, 1):
        res, M = R.restate([1], [2, 3], cells, topn=5, max_distance=0.5, min_votes=mv)
        assert M == np.float32(0.9) and res == {1: [(2, float(np.float32(0.9) - np.float32(0.2)))]}
    res, M = R.restate([1], [2, 3], cells, topn=5, max_distance=0.5, keep_below=0.9)
    assert M == np.float32(0.2) and res == {1: [(2, 0.0)]}
    res, M = R.restate([1], [2, 3], np.full_like(cells, -3.0), topn=5, max_distance=0.5)   # every distance below -1: M stays -1
    assert M == np.float32(-1.0) and res[1][0] == (2, 2.0)


def test_vectorised_restatement_equals_the_triple_form():
    rng = np.random.default_rng(3)
    Q, K, T = 4, 3, 7
    cells = rng.uniform(0, 1, (Q, K, T, K)).astype(np.float32)
    cells[rng.uniform(size=cells.shape) < 0.2] = np.nan
    q_ids, s_ids = [5, 1, 9, 2], [1, 2, 3, 4, 5, 6, 7]
    for mv, md, kb in ((1, 0.5, math.inf), (2, 0.8, 0.95), (0, 0.2, math.inf)):
        a = R.restate(q_ids, s_ids, cells, 3, md, mv, kb)
        b = R.winners(R.pair_metrics(q_ids, s_ids, cells, kb), 3, md, mv)
        assert a[0] == b[0] and a[1] == b[1]
