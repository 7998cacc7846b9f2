"""The BestFit vote on the MI355X (similari_amd.bestfit.BestFitStore over include/similari_bestfit.h).

No tolerance anywhere.  Every call with the tap is held to the host restatement (tests/bestfit_ref.py) on that call's own cells:
counts, winner ids, track ids and f64 weight bits; the call without the tap must return the same bits; (out_n, out_track,
out_weight) must be (out_n, out_winner, out_weight) of the TopN call with the same arguments; sa_store_bestfit_last must count the
restatement's groups and claimed tracks.  The shapes are the smallest that reach each path of the three launches."""
import ctypes as C
import math

import numpy as np
import pytest

import bestfit_ref as B
from bestfit_cases import (CONTENTION_SEED, D33, banks, contention_case, contention_thresholded, loses_first_wins_later, packed,
                           quantile, queries_without_a_group, rows, spans)
import compat_ref as X
from similari_amd import abi, attrs as A
from similari_amd.bestfit import BestFitStore
from similari_amd.engine import Engine, EngineError
from similari_amd.search import _p, sa_topn_params

pytestmark = pytest.mark.gpu
INF = math.inf
KINDS = ["cosine", "euclidean"]
u64 = np.uint64


@pytest.fixture(scope="module")
def engine():
    eng = Engine(abi.make_config(device=0))
    yield eng
    eng.close()


# ---- what every case asserts ----
def same_fit(a, b):
    """two raw BestFit results (out_n, winners, tracks, weights, ..): every bit"""
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[3].view(u64), b[3].view(u64))


def is_topn(fit, top):
    """(out_n, out_track, out_weight) of the BestFit call are (out_n, out_winner, out_weight) of the TopN call"""
    assert np.array_equal(fit[0], top[0]) and np.array_equal(fit[2], top[1])
    assert np.array_equal(fit[3].view(u64), top[2].view(u64))


def equals_model(raw, q_ids, want, topn):
    out_n, win, trk, wt = raw[:4]
    res = B.cut(want[0], topn)
    for i, q in enumerate(q_ids):
        lst = res.get(int(q), [])
        n = len(lst)
        assert out_n[i] == n, (q, out_n[i], n)
        assert [int(x) for x in trk[i, :n]] == [t for _, _, t in lst], q
        assert [int(x) for x in win[i, :n]] == [w for w, _, _ in lst], q
        assert np.array_equal(wt[i, :n].view(u64), np.array([w for _, w, _ in lst], np.float64).view(u64)), q
        assert not win[i, n:].any() and not trk[i, n:].any() and not wt[i, n:].view(u64).any()
    held = [int(w) for i, q in enumerate(q_ids) for w in win[i, : out_n[i]] if int(w) != int(q)]
    assert len(held) == len(set(held))   # a stored id is a winner at most once in the whole call


def checked(store, topn, call_fit, call_top, model, q_ids):
    """-> (the raw result of the call with the tap, the restatement (res, groups, claimed) on its cells)"""
    raw = call_fit(True)
    stats = store.bestfit_stats()
    want = model(raw[4])
    equals_model(raw, q_ids, want, topn)
    assert (stats["groups"], stats["claimed"]) == (want[1], want[2])
    same_fit(raw, call_fit(False))
    is_topn(raw, call_top())
    return raw, want


def fed(store, q_ids, q_feats, topn, md, mv=1, kb=INF, rule=None, q_attrs=None, s_attrs=None):
    order = store.order()
    qa = None if rule is None else packed(q_attrs)
    if rule is None:
        model = lambda c: B.restate(q_ids, order, c, md, mv, kb)
    else:
        model = lambda c: B.restate_compat(q_ids, order, c, rule, q_attrs, s_attrs, md, mv, kb)
    return checked(store, topn,
                   lambda tap: store.search_bestfit_raw(q_ids, q_feats, topn, md, mv, kb, tap=tap, compat=rule, q_attrs=qa),
                   lambda: store.search_raw(q_ids, q_feats, topn, md, mv, kb, compat=rule, q_attrs=qa),
                   model, q_ids)


def stored(store, ids, topn, md, mv=1, kb=INF, withdraw=False, rule=None, s_attrs=None):
    order = store.order()
    return checked(store, topn,
                   lambda tap: store.search_stored_bestfit_raw(ids, topn, md, mv, kb, withdraw, tap=tap, compat=rule),
                   lambda: store.search_stored_raw(ids, topn, md, mv, kb, withdraw, compat=rule),
                   lambda c: B.search_stored(order, c, ids, md, mv, kb, withdraw, rule, s_attrs), ids)


def joined(store, topn, md, mv=1, kb=INF, rule=None, s_attrs=None):
    order = store.order()
    return checked(store, topn,
                   lambda tap: store.join_bestfit_raw(topn, md, mv, kb, tap=tap, compat=rule),
                   lambda: store.join_raw(topn, md, mv, kb, compat=rule),
                   lambda c: B.join(order, c, md, mv, kb, rule, s_attrs), order)


def holders(res):
    """{stored id: the query that holds it}"""
    return {t: q for q, lst in res.items() for w, _, t in lst if w == t}


# ---- 1. contention (the case and its seeds: tests/bestfit_cases.py) ----
@pytest.mark.parametrize("kind", KINDS)
def test_contention(engine, kind):
    K, ids, s_feats, q_ids, q_feats = contention_case(kind, CONTENTION_SEED[kind])
    store = BestFitStore(engine, kind, D33, K)
    try:
        store.upsert(ids, s_feats)
        raw, (res, groups, claimed) = fed(store, q_ids, q_feats, 5, INF)
        assert claimed == 4 and 15 not in holders(res)   # the empty track has no claimant
        assert 3 * (groups - claimed) >= groups
        assert 106 not in res and raw[0][5] == 0
        fed(store, q_ids, q_feats, 2, INF)               # the claim runs over all groups, whatever topn is
        # thresholded: the state of the calls above must be gone, a rank-0 entry loses while a later one of the same query wins,
        # and a query that has observations is left without a group
        md, mv = contention_thresholded(kind, raw[4])
        _, (res, groups, claimed) = fed(store, q_ids, q_feats, 5, md, mv)
        assert loses_first_wins_later(res)
        assert queries_without_a_group(res, q_ids, q_feats)
    finally:
        store.close()


# ---- 2. exact ties ----
@pytest.mark.parametrize("kind", KINDS)
def test_exact_ties_go_to_the_lower_query_id(engine, kind):
    rng = np.random.default_rng(12)
    K, T = 3, 5
    store = BestFitStore(engine, kind, D33, K)
    try:
        store.upsert(np.arange(1, T + 1), banks(rng, T, K, D33, kind))
        twin = rows(rng, K, D33, kind)
        for q_ids in ([205, 203], [203, 205]):   # the call order of the two does not matter
            raw, (res, groups, claimed) = fed(store, q_ids, [twin, twin], 64, INF)
            out_n, win, trk, wt = raw[:4]
            assert out_n[0] == out_n[1] == T and np.array_equal(trk[0], trk[1])
            assert np.array_equal(wt[0].view(u64), wt[1].view(u64))   # first: the weight rows are bit-equal
            lo, hi = (0, 1) if q_ids[0] < q_ids[1] else (1, 0)
            assert np.array_equal(win[lo, :T], trk[lo, :T]) and np.all(win[hi, :T] == q_ids[hi])
            assert (groups, claimed) == (2 * T, T)
    finally:
        store.close()


# ---- 3. Kp = 32 ----
@pytest.mark.parametrize("kind", KINDS)
def test_32_observations_per_track(engine, kind):
    rng = np.random.default_rng(32)
    K, Q, T, D = 32, 3, 4, 64
    store = BestFitStore(engine, kind, D, K)
    try:
        store.upsert(np.arange(1, T + 1) * 7, banks(rng, T, K, D, kind))
        q_ids, q_feats = np.arange(1, Q + 1) + 500, banks(rng, Q, K, D, kind)
        raw, _ = fed(store, q_ids, q_feats, 4, INF)
        fed(store, q_ids, q_feats, 2, quantile(raw[4], 0.6), 3)
        joined(store, 3, quantile(raw[4], 0.6), 3)
    finally:
        store.close()


# ---- 4. across tiles and workgroups ----
@pytest.mark.parametrize("kind", KINDS)
def test_across_tiles(engine, kind):
    rng = np.random.default_rng(70)
    K, Q, T = 1, 70, 150
    store = BestFitStore(engine, kind, D33, K)
    try:
        store.upsert(np.arange(1, T + 1), banks(rng, T, K, D33, kind))
        q_ids, q_feats = np.arange(1, Q + 1) + 1000, banks(rng, Q, K, D33, kind)
        raw, _ = fed(store, q_ids, q_feats, 5, INF)
        _, (res, groups, claimed) = fed(store, q_ids, q_feats, 5, quantile(raw[4], 0.3))
        assert 0 < claimed < groups < Q * T
    finally:
        store.close()


@pytest.mark.parametrize("kind", KINDS)
def test_the_pool_overflow_rerun(engine, kind):
    """800 groups against a fresh store's 256 pool blocks: both stages run twice, the second time over a reset per-column state"""
    rng = np.random.default_rng(20)
    K, Q, T = 4, 20, 40
    store = BestFitStore(engine, kind, D33, K)
    try:
        order = np.arange(1, T + 1)
        store.upsert(order, banks(rng, T, K, D33, kind))
        q_ids, q_feats = np.arange(1, Q + 1) + 1000, banks(rng, Q, K, D33, kind)
        raw = store.search_bestfit_raw(q_ids, q_feats, 5, INF, tap=True)
        assert store.last_stats()["reruns"] == 1 and store.last_stats()["groups"] == Q * T
        want = B.restate(q_ids, order, raw[4], INF)
        equals_model(raw, q_ids, want, 5)
        st = store.bestfit_stats()
        assert (st["groups"], st["claimed"]) == (want[1], want[2]) == (Q * T, T)
        again, _ = fed(store, q_ids, q_feats, 5, INF)
        assert store.last_stats()["reruns"] == 0
        same_fit(raw, again)
    finally:
        store.close()


# ---- 5. more than 2048 groups in one query ----
def lists_k1(q_ids, s_ids, cells, md):
    """steps 1-7 for K = 1, vectorised: every group is one cell, its weight one term -> {query: [(track, weight), ...]} in TopN order"""
    d = np.asarray(cells, np.float32)[:, 0, :, 0]
    valid = ~np.isnan(d) & (np.asarray(q_ids, u64)[:, None] != np.asarray(s_ids, u64)[None, :])
    M = np.float32(max(np.float32(-1.0), d[valid].max()))
    with np.errstate(invalid="ignore"):
        kept = valid & (d <= np.float32(md))
    w = (M - d).astype(np.float32).astype(np.float64)
    out = {}
    for i, q in enumerate(q_ids):
        t = np.nonzero(kept[i])[0]
        t = t[np.lexsort((np.asarray(s_ids, u64)[t], -w[i, t]))]
        if len(t):
            out[int(q)] = [(int(s_ids[k]), float(w[i, k])) for k in t]
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_more_groups_than_a_workgroup_keeps_in_lds(engine, kind):
    rng = np.random.default_rng(2100)
    K, Q, T, D = 1, 3, 2100, 32
    store = BestFitStore(engine, kind, D, K)
    try:
        order = np.arange(1, T + 1)
        store.upsert(order, list(rows(rng, T, D, kind)[:, None, :]))
        q_ids, q_feats = [9001, 9002, 9003], list(rows(rng, Q, D, kind)[:, None, :])
        for topn in (64, 3):
            _, (res, groups, claimed) = checked(store, topn,
                                                lambda tap: store.search_bestfit_raw(q_ids, q_feats, topn, INF, tap=tap),
                                                lambda: store.search_raw(q_ids, q_feats, topn, INF),
                                                lambda c: B.claim(lists_k1(q_ids, order, c, INF)), q_ids)
            assert (groups, claimed) == (Q * T, T)
    finally:
        store.close()


# ---- 6. gallery forms ----
@pytest.mark.parametrize("kind", KINDS)
def test_gallery_forms(engine, kind):
    rng = np.random.default_rng(40)
    K, T = 4, 40
    store = BestFitStore(engine, kind, D33, K)
    try:
        ids = np.arange(1, T + 1) * 2
        store.upsert(ids, banks(rng, T, K, D33, kind))
        order = store.order()
        full = store.join_bestfit_raw(5, INF, tap=True)
        md = quantile(full[4], 0.4)
        n_obs, feats, _ = store.fetch_raw(order)
        fetched = [feats[i, : n_obs[i]] for i in range(T)]
        for topn, mv in ((5, 2), (64, 1)):
            j, (res, groups, claimed) = joined(store, topn, md, mv)
            assert 0 < claimed < groups
            s, _ = stored(store, order, topn, md, mv)
            f, _ = fed(store, order, fetched, topn, md, mv)
            same_fit(j, s)
            same_fit(j, f)
        some = ids[[3, 4, 17, 30, 31, 39]]
        raw, (res, groups, claimed) = stored(store, some, 5, md, withdraw=True)
        assert groups and not set(holders(res)) & {int(i) for i in some}   # a withdrawn column has no claimant
        assert not np.isin(raw[2], some).any()
        unknown = np.concatenate([some[:2], [9999]])                       # an id the store does not hold: a query without a group
        stored(store, unknown, 5, md)
    finally:
        store.close()


@pytest.mark.parametrize("kind", KINDS)
def test_a_join_of_2100_tracks_is_the_stored_form(engine, kind):
    """4.4 M groups, every row beyond what a workgroup keeps in LDS: held to sa_store_search_stored_bestfit over order() only"""
    rng = np.random.default_rng(2101)
    K, T, D = 1, 2100, 32
    store = BestFitStore(engine, kind, D, K)
    try:
        store.upsert(np.arange(1, T + 1), list(rows(rng, T, D, kind)[:, None, :]))
        j = store.join_bestfit_raw(8, INF)
        st = store.bestfit_stats()
        assert (st["groups"], st["claimed"]) == (T * (T - 1), T)
        same_fit(j, store.search_stored_bestfit_raw(store.order(), 8, INF))
        is_topn(j, store.join_raw(8, INF))
        won = j[1][j[1] == j[2]]
        assert len(won) == len(set(won.tolist())) and (j[1] != j[2]).any()
    finally:
        store.close()


def order_case(seed, K=32):
    """tests/test_gpu_gallery.py::order_case: two tracks in the plane whose block mixes cosines near -1 with cosines of a few 1e-8, so
    that the sequential f64 sum of the block depends on whether it is taken row by row or column by column"""
    rng = np.random.default_rng(seed)
    a = np.zeros((K, 2), np.float32)
    b = np.zeros((K, 2), np.float32)
    small = np.arange(K) % 2 == 0
    a[small, 0] = 1
    a[small, 1] = rng.uniform(0, 1e-7, small.sum())
    a[~small, 0] = rng.uniform(-0.5, 0.5, (~small).sum())
    a[~small, 1] = -1
    b[:, 0] = -rng.uniform(0, 1e-7, K)
    b[:, 1] = 1
    return a, b


def test_each_direction_of_a_pair_claims_with_its_own_weight(engine):
    told_apart = 0
    for seed in (0, 3, 5):
        a, b = order_case(seed)
        store = BestFitStore(engine, "cosine", 2, 32)
        try:
            store.upsert([10, 20], [a, b])
            (out_n, win, trk, wt, cells), _ = joined(store, 5, INF)
            blk = cells[0, :, 1, :]
            terms = (blk.max() - blk).astype(np.float32).astype(np.float64)
            rows_first = float(np.cumsum(terms.reshape(-1))[-1])     # query 10: its observations are the block's rows
            cols_first = float(np.cumsum(terms.T.reshape(-1))[-1])   # query 20: its observations are the block's columns
            assert list(out_n) == [1, 1] and (win[0, 0], win[1, 0]) == (20, 10) and (trk[0, 0], trk[1, 0]) == (20, 10)
            assert wt[0, 0].hex() == rows_first.hex() and wt[1, 0].hex() == cols_first.hex()
            same_fit((out_n, win, trk, wt), store.search_stored_bestfit_raw([10, 20], 5, INF))
            told_apart += rows_first.hex() != cols_first.hex()
        finally:
            store.close()
    assert told_apart >= 1


# ---- 7. under a rule ----
def compat_case(kind, seed=7):
    rng = np.random.default_rng(seed)
    K, T, Q = 3, 12, 9
    ids = np.arange(1, T + 1) * 3
    q_ids = np.arange(1, Q + 1) * 3 + 1000
    return K, ids, banks(rng, T, K, D33, kind), spans(rng, T), q_ids, banks(rng, Q, K, D33, kind), spans(rng, Q)


@pytest.mark.parametrize("kind", KINDS)
def test_a_dead_best_group_leaves_its_column_to_the_next(engine, kind):
    K, ids, feats, s_attrs, q_ids, q_feats, q_attrs = compat_case(kind)
    rule = A.Compat(X.SAME_KEY | X.DISJOINT)
    store = BestFitStore(engine, kind, D33, K)
    try:
        store.upsert(ids, feats)
        store.set_attrs_raw(ids, packed(s_attrs))
        _, (plain, _, _) = fed(store, q_ids, q_feats, 64, INF)
        _, (ruled, groups, claimed) = fed(store, q_ids, q_feats, 64, INF, rule=rule, q_attrs=q_attrs, s_attrs=s_attrs)
        lv = X.live_matrix(rule, q_attrs, s_attrs)
        live = lambda q, t: lv[list(q_ids).index(q), list(ids).index(t)]
        was, now = holders(plain), holders(ruled)
        moved = [t for t, q in was.items() if not live(q, t) and t in now]
        assert moved                                             # the best-ranked group of some column is dead ..
        assert all(live(now[t], t) and now[t] != was[t] for t in moved)   # .. and the next one claims it
        filtered = {q: [e for e in lst if live(q, e[2])] for q, lst in plain.items()}
        assert not set(moved) & set(holders(filtered))           # a host-side filter of the plain call leaves such a column unclaimed
        assert {q: lst for q, lst in filtered.items() if lst} != ruled
        assert groups == int(lv.sum()) and claimed == int(lv.any(axis=0).sum())
        fed(store, q_ids, q_feats, 2, INF, rule=rule, q_attrs=q_attrs, s_attrs=s_attrs)
    finally:
        store.close()


@pytest.mark.parametrize("kind", KINDS)
def test_an_asymmetric_rule_in_a_join_and_a_rule_without_bits(engine, kind):
    K, ids, feats, s_attrs, q_ids, q_feats, q_attrs = compat_case(kind, 8)
    store = BestFitStore(engine, kind, D33, K)
    try:
        store.upsert(ids, feats)
        store.set_attrs_raw(ids, packed(s_attrs))
        first = A.Compat(X.QUERY_FIRST)
        lv = X.live_matrix(first, s_attrs, s_attrs)
        assert (lv != lv.T).any()
        j, (res, groups, claimed) = joined(store, 5, INF, rule=first, s_attrs=s_attrs)   # directions claim independently
        assert 0 < claimed <= groups < len(ids) * (len(ids) - 1)
        s, _ = stored(store, store.order(), 5, INF, rule=first, s_attrs=s_attrs)
        same_fit(j, s)
        none = A.compat()
        for a, b in ((store.search_bestfit_raw(q_ids, q_feats, 5, INF), store.search_bestfit_raw(q_ids, q_feats, 5, INF, compat=none, q_attrs=packed(q_attrs))),
                     (store.search_stored_bestfit_raw(ids[:5], 5, INF, withdraw=True), store.search_stored_bestfit_raw(ids[:5], 5, INF, withdraw=True, compat=none)),
                     (store.join_bestfit_raw(5, INF), store.join_bestfit_raw(5, INF, compat=none))):
            assert a[0].any()
            same_fit(a, b)
    finally:
        store.close()


# ---- 8. refusals and neighbours ----
def test_refusals_leave_the_store_unchanged(engine):
    rng = np.random.default_rng(41)
    K, D, T = 3, 20, 20
    store = BestFitStore(engine, "cosine", D, K)
    try:
        ids = np.arange(1, T + 1)
        store.upsert(ids, banks(rng, T, K, D, "cosine"))
        q_ids, q_feats = [100, 101], banks(rng, 2, K, D, "cosine", ragged=False)
        q_attrs = packed([(1, 0, 5), (1, 6, 9)])
        long = np.zeros((K + 1, D), np.float32)
        rule = A.compat(same_key=True)
        fit = store.search_bestfit_raw
        before = (store.order(), fit(q_ids, q_feats, 5, 0.3, tap=True))
        BAD, UNS = abi.SA_ERR_BAD_ARG, abi.SA_ERR_UNSUPPORTED
        lib, h = store.lib, store.h
        prm = sa_topn_params(5, 1, 0.3, INF)
        n, w, t, x = np.zeros(T, np.uint32), np.zeros((T, 5), u64), np.zeros((T, 5), u64), np.zeros((T, 5))
        outs = (_p(n, C.c_uint32), _p(w, C.c_uint64), _p(t, C.c_uint64), _p(x, C.c_double), None)
        qi, qn = np.array(q_ids, u64), np.array([K, K], np.uint32)

        def raw_rc(rc):
            store._chk(rc)

        bad = [
            (BAD, lambda: fit(q_ids, q_feats, 0, 0.3)),                                   # topn 0
            (UNS, lambda: fit(q_ids, q_feats, 65, 0.3)),                                  # topn > 64
            (BAD, lambda: fit(q_ids, q_feats, 5, float("nan"))),
            (BAD, lambda: fit(q_ids, q_feats, 5, 0.3, keep_below=float("nan"))),
            (BAD, lambda: fit([100, 100], q_feats, 5, 0.3)),                              # an id twice
            (BAD, lambda: fit([0, 101], q_feats, 5, 0.3)),                                # id 0
            (BAD, lambda: fit(q_ids, [q_feats[0], long], 5, 0.3)),                        # more than K observations
            (BAD, lambda: fit(q_ids, q_feats, 5, 0.3, compat=rule)),                      # a rule without q_attrs
            (BAD, lambda: fit(q_ids, q_feats, 5, 0.3, q_attrs=q_attrs)),                  # q_attrs without a rule
            (BAD, lambda: fit(q_ids, q_feats, 5, 0.3, compat=A.sa_compat(8, 1, 0), q_attrs=q_attrs)),      # struct_size
            (BAD, lambda: fit(q_ids, q_feats, 5, 0.3, compat=A.Compat(16), q_attrs=q_attrs)),              # unknown rule bits
            (BAD, lambda: fit(q_ids, q_feats, 5, 0.3, compat=A.Compat(X.DISJOINT | X.QUERY_FIRST), q_attrs=q_attrs)),
            (BAD, lambda: fit(q_ids, q_feats, 5, 0.3, compat=rule, q_attrs=packed([(1, 5, 0), (1, 6, 9)]))),   # start > end
            (BAD, lambda: store.search_stored_bestfit_raw(ids[:3], 5, 0.3, flags=2)),     # unknown flag bits
            (BAD, lambda: store.search_stored_bestfit_raw([3, 3], 5, 0.3)),
            (BAD, lambda: store.search_stored_bestfit_raw([3, 0], 5, 0.3, compat=rule)),
            (UNS, lambda: store.join_bestfit_raw(65, 0.3)),
            (BAD, lambda: store.join_bestfit_raw(5, float("nan"), compat=rule)),
            (BAD, lambda: raw_rc(lib.sa_store_join_bestfit(h, None, None, *outs))),       # null params
            (BAD, lambda: raw_rc(lib.sa_store_join_bestfit(h, C.byref(prm), None, None, *outs[1:]))),            # null out_n
            (BAD, lambda: raw_rc(lib.sa_store_join_bestfit(h, C.byref(prm), None, outs[0], None, *outs[2:]))),   # null out_winner
            (BAD, lambda: raw_rc(lib.sa_store_join_bestfit(h, C.byref(prm), None, *outs[:3], None, None))),      # null out_weight
            (BAD, lambda: raw_rc(lib.sa_store_search_stored_bestfit(h, C.byref(prm), None, 0, 2, None, *outs))),   # null ids
            (BAD, lambda: raw_rc(lib.sa_store_search_bestfit(h, C.byref(prm), None, 2, None, _p(qn, C.c_uint32), None, None, *outs))),   # null q_ids
            (BAD, lambda: raw_rc(lib.sa_store_search_bestfit(h, C.byref(prm), None, 2, _p(qi, C.c_uint64), _p(qn, C.c_uint32), None, None, *outs))),   # null q_feats
            (BAD, lambda: raw_rc(lib.sa_store_search_bestfit(h, C.byref(prm), None, 2, _p(qi, C.c_uint64), None, None, None, *outs))),   # null q_n_obs
        ]
        for k, (code, call) in enumerate(bad):
            with pytest.raises(EngineError) as ei:
                call()
            assert ei.value.code == code, k
        after = (store.order(), fit(q_ids, q_feats, 5, 0.3, tap=True))
        assert np.array_equal(before[0], after[0])
        same_fit(before[1], after[1])
        assert np.array_equal(before[1][4], after[1][4], equal_nan=True)
        raw_rc(lib.sa_store_join_bestfit(h, C.byref(prm), None, outs[0], outs[1], None, outs[3], None))   # out_track and out_cells may be null
        same = store.join_bestfit_raw(5, 0.3)
        assert np.array_equal(n, same[0]) and np.array_equal(w, same[1]) and np.array_equal(x.view(u64), same[3].view(u64))
        assert store.join_bestfit_raw(5, 0.3, track=False)[2] is None
    finally:
        store.close()


def test_an_extent_beyond_the_limits_is_refused(engine):
    """65 536 queries x 32 observation slots: one query slot more than a search's grid can tile (sa_search_limits.h), as
    tests/test_gpu_search.py::test_nan_parameters_and_oversized_searches_are_refused; the edge itself runs all three launches"""
    rng = np.random.default_rng(61)
    K, D = 32, 8
    store = BestFitStore(engine, "euclidean", D, K)
    try:
        store.upsert([1, 2], banks(rng, 2, K, D, "euclidean", ragged=False))
        n = 65535 * 32 // K + 1
        for rule, qa in ((None, None), (A.compat(), packed([(0, 0, 0)] * n))):
            with pytest.raises(EngineError) as ei:
                store.search_bestfit_raw(np.arange(100, 100 + n), [None] * n, 5, 1.0, compat=rule, q_attrs=qa)
            assert ei.value.code == abi.SA_ERR_UNSUPPORTED
        n -= 1
        out_n, win, trk, wt, _ = store.search_bestfit_raw(np.arange(100, 100 + n), [None] * n, 5, 1.0)   # no observations, no groups
        assert not out_n.any() and not win.any() and not trk.any()
        st = store.bestfit_stats()
        assert (st["groups"], st["claimed"]) == (0, 0) and len(store) == 2
        one = store.search_bestfit_raw([100], banks(rng, 1, K, D, "euclidean", ragged=False), 5, INF)   # the store still answers
        assert one[0][0] == 2 and set(one[1][0, :2].tolist()) == {1, 2}
    finally:
        store.close()


def test_an_empty_store_and_an_empty_call(engine):
    store = BestFitStore(engine, "euclidean", 8, 2)
    try:
        rng = np.random.default_rng(1)
        out_n, win, trk, wt, _ = store.search_bestfit_raw([5, 6], banks(rng, 2, 2, 8, "euclidean"), 3, INF)
        assert not out_n.any() and not win.any() and not trk.any() and not wt.any()
        assert store.join_bestfit(3, INF) == {} and store.search_bestfit([], [], 3, INF) == {}
        assert store.bestfit_stats()["groups"] == 0
    finally:
        store.close()


@pytest.mark.parametrize("kind", KINDS)
def test_topn_is_untouched_by_a_bestfit_call_between(engine, kind):
    rng = np.random.default_rng(88)
    K, T, Q = 3, 30, 11
    store = BestFitStore(engine, kind, D33, K)
    try:
        store.upsert(np.arange(1, T + 1), banks(rng, T, K, D33, kind))
        q_ids, q_feats = np.arange(1, Q + 1) + 100, banks(rng, Q, K, D33, kind)
        md = quantile(store.search_raw(q_ids, q_feats, 5, INF, tap=True)[3], 0.5)
        for call in (lambda: store.search_raw(q_ids, q_feats, 5, md, 2), lambda: store.join_raw(5, md, 2)):
            a = call()
            store.search_bestfit_raw(q_ids, q_feats, 5, md, 2)
            store.join_bestfit_raw(7, INF)
            b = call()
            assert a[0].any() and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(u64), b[2].view(u64))
        st = store.last_stats()
        assert st["launch1_ms"] > 0 and st["launch2_ms"] > 0
        store.join_bestfit_raw(7, INF)
        st, fs = store.last_stats(), store.bestfit_stats()
        assert st["groups"] == store.join_stats()["blocks"] == T * (T - 1) // 2 and fs["groups"] == T * (T - 1)
        assert abs(st["launch2_ms"] - (fs["weigh_ms"] + fs["claim_ms"] + fs["rank_ms"])) < 1e-6 and min(fs["weigh_ms"], fs["claim_ms"], fs["rank_ms"]) > 0
    finally:
        store.close()


def test_mutual_pairs_of_a_bestfit_join_merge_as_they_come(engine):
    """Tracklet pairs: tracks 2i and 2i + 1 observe one identity.  With topn = 1 a track's entry is its best group; where that group
    holds its claim in both directions the two tracks name each other and nobody else does — no host-side filter before the merge."""
    rng = np.random.default_rng(64)
    K, T, D = 2, 40, 24
    ident = rng.uniform(0, 1, (T // 2, D)).astype(np.float32)
    feats = [(ident[i // 2] + rng.normal(0, 0.02, (K, D))).astype(np.float32) for i in range(T)]
    store = BestFitStore(engine, "euclidean", D, 2 * K)
    try:
        ids = np.arange(1, T + 1)
        store.upsert(ids, feats)
        top = {q: lst[0][0] for q, lst in store.join_bestfit(1, INF).items()}
        pairs = {q: [w] for q, w in top.items() if q < w and top.get(w) == q}
        assert len(pairs) == T // 2 and all(w == q + 1 and q % 2 for q, (w,) in pairs.items())
        store.merge(pairs)
        assert len(store) == T // 2 and set(store.order().tolist()) == set(pairs)
        assert all(n == 2 * K for n in store.fetch_raw(store.order())[0])
    finally:
        store.close()
