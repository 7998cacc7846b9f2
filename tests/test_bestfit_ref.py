"""The host restatement of the BestFit vote (tests/bestfit_ref.py) against the pinned checker of BestFitVoting::winners
(or_bestfit_voting, oracle/oracle.cpp) and against itself: the two KATs of test_oracle_kat.py, the "TopN list with replaced ids"
identity and the invariance under a permutation of the queries.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import bestfit_cases as Z
import bestfit_ref as B
import compat_ref as X
import oracle_lib as O
import topn_ref as R

L = O.lib()
BIG = 3.4e38


def _u64(v):
    a = np.array(v, np.uint64)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint64))


def oracle_rank0(rows, ids, votes=1, maxd=BIG):
    """{query: (winner, weight)} of or_bestfit_voting for the queries that have a group"""
    fr, frp = _u64([r[0] for r in rows])
    to, top = _u64([r[1] for r in rows])
    vis = np.array([r[2] for r in rows], np.float32)
    idarr, idp = _u64(ids)
    out, outp = _u64([0] * len(ids))
    w = np.zeros(len(ids))
    L.or_bestfit_voting(maxd, votes, len(rows), frp, top, O.fptr(vis), len(ids), idp, outp, O.dptr(w))
    return {int(q): (int(t), float(x)) for q, t, x in zip(ids, out, w) if t}


def rank0(res):
    return {q: (lst[0][0], lst[0][1]) for q, lst in res.items()}


def all_weights(res):
    return [w for lst in res.values() for _, w, _ in lst]


def cells_of(rng, Q, K, T, absent=0.2, levels=None):
    """[Q][K][T][K] with absent observations on both sides; levels: distances drawn from that many values, so that weights tie"""
    d = rng.uniform(0.05, 1.0, (Q, K, T, K)).astype(np.float32)
    if levels:
        d = (np.floor(d * levels) / levels).astype(np.float32)
    d[rng.uniform(size=(Q, K)) < absent] = np.nan
    d[:, :, rng.uniform(size=(T, K)) < absent] = np.nan
    return d


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("votes", [1, 2])
def test_rank_0_is_the_oracles_on_random_lists_with_distinct_weights(seed, votes):
    rng = np.random.default_rng(seed)
    queries = [int(q) for q in rng.permutation(np.arange(1, 9))]
    n = 150
    rows = [(int(rng.choice(queries)), int(rng.integers(100, 106)), float(np.float32(rng.uniform(0.1, 1.0)))) for _ in range(n)]
    maxd = 0.8
    res, groups, claimed = B.from_triples(rows, maxd, votes)
    ws = all_weights(res)
    assert groups == len(ws) >= 8 and len(set(ws)) == len(ws)   # no ties: the oracle's first-appearance rule is not exercised
    assert groups - claimed >= 2                                # and some group does lose its track
    assert rank0(res) == oracle_rank0(rows, queries, votes, maxd)


@pytest.mark.parametrize("seed", range(4))
def test_rank_0_is_the_oracles_on_ordered_lists_with_ties(seed):
    """Query ids ascending in call order, stored ids ascending in column order: the oracle's stable sort over first appearance is
    then (weight desc, query id asc, stored id asc), rule 8b — ties included."""
    rng = np.random.default_rng(100 + seed)
    Q, K, T = 7, 2, 5
    q_ids = np.arange(1, Q + 1) * 2
    s_ids = np.arange(1, T + 1) * 2 + 101
    cells = cells_of(rng, Q, K, T, levels=3)
    cells[3] = cells[1]   # two queries with the same distances: their weights tie in every column
    rows = R.pair_metrics(q_ids, s_ids, cells)
    maxd = 0.7
    res, groups, claimed = B.restate(q_ids, s_ids, cells, maxd)
    ws = all_weights(res)
    assert len(set(ws)) < len(ws)
    assert rank0(res) == oracle_rank0(rows, [int(q) for q in q_ids], 1, maxd)
    assert (res, groups, claimed) == B.from_triples(rows, maxd)


def test_the_weight_formula_kat_through_the_restatement():
    """tests/test_oracle_kat.py::test_bestfit_weight_formula_kat"""
    assert B.from_triples([(7, 1, 0.2)], BIG)[0] == {7: [(1, 0.0, 1)]}
    assert B.from_triples([(7, 1, 0.2), (7, 1, 0.3)], BIG)[0] == {7: [(1, 0.10000000894069672, 1)]}
    assert B.from_triples([(7, 1, 0.2), (7, 1, 0.4)], 0.32)[0] == {7: [(1, 0.20000000298023224, 1)]}


def test_the_greedy_kat_through_the_restatement():
    """tests/test_oracle_kat.py::test_bestfit_greedy_marks_every_group: every group of a query marks its track taken, not only its best"""
    rows = [(1, 10, 0.1), (1, 20, 0.2), (2, 20, 0.3), (2, 30, 0.4), (3, 99, 0.9)]
    res, groups, claimed = B.from_triples(rows, BIG)
    assert [res[q][0][0] for q in (1, 2, 3)] == [10, 2, 99]
    assert [(w, t) for w, _, t in res[1]] == [(10, 10), (20, 20)]
    assert [(w, t) for w, _, t in res[2]] == [(2, 20), (30, 30)]   # the second entry of a query can win where its first lost
    assert (groups, claimed) == (5, 4)
    assert rank0(res) == oracle_rank0(rows, [1, 2, 3])


@pytest.mark.parametrize("seed", range(3))
def test_a_bestfit_list_is_the_topn_list_with_replaced_ids(seed):
    rng = np.random.default_rng(200 + seed)
    Q, K, T = 9, 3, 6
    q_ids = np.arange(1, Q + 1) + 50
    s_ids = np.arange(1, T + 1)
    q_ids[2] = s_ids[4]   # one query carries a stored id: its self pair forms no group
    cells = cells_of(rng, Q, K, T)
    for maxd, votes in ((2.0, 1), (0.6, 2)):
        res, groups, claimed = B.restate(q_ids, s_ids, cells, maxd, votes)
        for topn in (1, 2, 64):
            assert B.topn_view(res, topn) == R.restate(q_ids, s_ids, cells, topn, maxd, votes)[0]
        entries = [(q, w, t) for q, lst in res.items() for w, _, t in lst]
        assert groups == len(entries)
        assert all(w in (q, t) and q != t for q, w, t in entries)
        won = [w for q, w, t in entries if w == t]
        assert len(won) == len(set(won)) == claimed == len({t for _, _, t in entries})
        assert groups - claimed == sum(w == q for q, w, _ in entries) > 0


@pytest.mark.parametrize("seed", range(3))
def test_the_result_does_not_depend_on_the_order_of_the_queries(seed):
    rng = np.random.default_rng(300 + seed)
    Q, K, T = 8, 2, 5
    q_ids = np.arange(1, Q + 1) * 3 + 40
    s_ids = np.arange(1, T + 1)
    cells = cells_of(rng, Q, K, T, levels=4)
    cells[5] = cells[0]   # ties across queries: the lower id must hold them wherever it stands in the call
    want = B.restate(q_ids, s_ids, cells, 0.8)
    for _ in range(3):
        p = rng.permutation(Q)
        assert B.restate(q_ids[p], s_ids, cells[p], 0.8) == want
    shared = [t for w, _, t in want[0][int(q_ids[0])] if w == t]
    assert all(w == int(q_ids[5]) for w, _, t in want[0][int(q_ids[5])] if t in shared)


def test_the_gallery_and_compat_forms_claim_over_their_own_groups():
    rng = np.random.default_rng(7)
    T, K = 7, 2
    s_ids = np.arange(1, T + 1) * 5
    cells = cells_of(rng, T, K, T, absent=0.0)
    cells = np.minimum(cells, cells.transpose(2, 3, 0, 1))   # a store against itself: the block of (t, q) is the transpose of (q, t)
    res, groups, claimed = B.join(s_ids, cells, 2.0)
    assert groups == T * (T - 1) and claimed == T
    some = s_ids[[1, 4, 6]]
    out, g2, c2 = B.search_stored(s_ids, cells[[1, 4, 6]], some, 2.0, withdraw=True)
    assert (g2, c2) == (3 * (T - 3), T - 3)
    assert not {t for lst in out.values() for _, _, t in lst} & {int(i) for i in some}   # a withdrawn column has no claimant
    attrs = [(1 + i % 2, 0, 1) for i in range(T)]
    ruled, g3, c3 = B.join(s_ids, cells, 2.0, rule=(X.SAME_KEY, X.INT64_MAX), s_attrs=attrs)
    assert g3 == sum(a[0] == b[0] for i, a in enumerate(attrs) for j, b in enumerate(attrs) if i != j) and c3 == T
    assert all(attrs[list(s_ids).index(q)][0] == attrs[list(s_ids).index(t)][0] for q, lst in ruled.items() for _, _, t in lst)


@pytest.mark.parametrize("kind", ["cosine", "euclidean"])
def test_the_contention_seeds_were_chosen_for_what_the_gpu_test_asserts(kind):
    """tests/test_gpu_bestfit.py::test_contention asserts these on the engine's cells; here the same on numpy's, so the choice of
    Z.CONTENTION_SEED can be made again from this file: in the thresholded variant some query's rank-0 entry loses while a later
    entry of the same query wins, and some query with observations has no group; unthresholded, four tracks are claimed and at
    least a third of the groups lose."""
    K, ids, s_feats, q_ids, q_feats = Z.contention_case(kind, Z.CONTENTION_SEED[kind])
    assert (len(ids), len(q_ids), K) == (5, 8, 3) and s_feats[4] is None and sum(f is None for f in q_feats) == 1
    cells = Z.host_cells(kind, q_feats, s_feats, K)
    res, groups, claimed = B.restate(q_ids, ids, cells, np.inf)
    assert claimed == 4 and 3 * (groups - claimed) >= groups
    md, mv = Z.contention_thresholded(kind, cells)
    res, groups, claimed = B.restate(q_ids, ids, cells, md, mv)
    assert Z.loses_first_wins_later(res)
    assert Z.queries_without_a_group(res, q_ids, q_feats)
