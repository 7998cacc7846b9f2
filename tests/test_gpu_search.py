"""Track search on the MI355X (similari_amd.search.FeatureStore over include/similari_search.h).

Self-consistency is exact: out_n, winners and f64 weights equal the host restatement (tests/topn_ref.py) applied to the engine's own
cell matrix, bit for bit.  The cells themselves are held to the oracle's or_cosine / or_euclidean within the suite's tolerances, and the
winners to the restatement on oracle distances apart from counted borderline decisions."""
import math

import numpy as np
import pytest

import oracle_lib as O
import topn_ref as R
from similari_amd import abi
from similari_amd.engine import Engine, EngineError
from similari_amd.search import FeatureStore

pytestmark = pytest.mark.gpu
INF = math.inf


@pytest.fixture(scope="module")
def engine():
    eng = Engine(abi.make_config(device=0))
    yield eng
    eng.close()


def bank(rng, n, K, D, ragged=True, zero_frac=0.0, scale=1.0):
    out = []
    for _ in range(n):
        k = int(rng.integers(0, K + 1)) if ragged else K
        f = (rng.uniform(0, 1, (k, D)) * scale).astype(np.float32)
        f[rng.uniform(size=k) < zero_frac] = 0.0
        out.append(f)
    return out


def engine_result(out_n, win, wt, q_ids):
    return {int(q): [(int(win[i, r]), float(wt[i, r])) for r in range(int(out_n[i]))] for i, q in enumerate(q_ids) if out_n[i]}


def check_exact(store, q_ids, q_feats, topn, md, mv=1, kb=INF):
    """The engine's winners == the restatement on the engine's own cells (every bit of every weight)."""
    out_n, win, wt, cells = store.search_raw(q_ids, q_feats, topn, md, mv, kb, tap=True)
    want, M = R.restate(q_ids, store.order(), cells, topn, md, mv, kb)
    got = engine_result(out_n, win, wt, q_ids)
    assert got == want
    assert np.all(win[np.arange(win.shape[1])[None, :] >= out_n[:, None]] == 0)
    return got, cells, M


def distance_quantile(cells, q):
    v = cells[~np.isnan(cells)]
    return float(np.quantile(v, q)) if v.size else 0.5


@pytest.mark.parametrize("kind", ["cosine", "euclidean"])
@pytest.mark.parametrize("K", [1, 3, 5, 30, 32])
@pytest.mark.parametrize("D", [2, 100, 256, 1024])
def test_winners_equal_the_restatement_on_the_engines_cells(engine, kind, K, D):
    rng = np.random.default_rng(1000 * K + D + (kind == "cosine"))
    T, Q = 37, 6
    s_ids = rng.choice(np.arange(1, 500), T, replace=False)
    q_ids = np.concatenate([s_ids[:3], rng.choice(np.arange(500, 900), Q - 3, replace=False)])   # three queries are stored too
    zero = 0.15 if kind == "cosine" else 0.0
    store = FeatureStore(engine, kind, D, K)
    try:
        store.upsert(s_ids, bank(rng, T, K, D, zero_frac=zero))
        q_feats = bank(rng, Q, K, D, zero_frac=zero)
        q_feats[1] = np.zeros((0, D), np.float32)   # a query without observations: no pairs
        _, cells, _ = check_exact(store, q_ids, q_feats, 5, INF)
        lo, mid = distance_quantile(cells, 0.05), distance_quantile(cells, 0.5)
        for topn, md, mv, kb in ((1, mid, 1, INF), (5, lo, 0, INF), (64, mid, 3, distance_quantile(cells, 0.9)), (64, INF, 1, INF),
                                 (5, mid, 1, distance_quantile(cells, 0.3))):
            check_exact(store, q_ids, q_feats, topn, md, mv, kb)
    finally:
        store.close()


def test_m_comes_from_another_query(engine):
    """As two_query_vecs: query 2's weights are taken against the maximum that query 20 sets; query 2's own pair with stored track 2
    (a larger distance) is a self pair and never becomes M."""
    D, K = 16, 2
    store = FeatureStore(engine, "euclidean", D, K)
    try:
        near = np.zeros((K, D), np.float32)
        far = np.full((K, D), 10.0, np.float32)
        store.upsert([1, 2], [near + 0.01, far])
        got, cells, M = check_exact(store, [2], [near], 5, 1.0)
        assert M == np.float32(np.nanmax(cells[0, :, 0, :])) < np.nanmin(cells[0, :, 1, :])
        assert got == {2: [(1, 0.0)]}
        got, cells, M = check_exact(store, [2, 20], [near, far + 5.0], 5, 1.0)
        assert M == np.float32(np.nanmax(cells[1])) and M > np.nanmax(cells[0])
        assert got[2][0][0] == 1 and got[2][0][1] > 0.0 and 20 not in got
    finally:
        store.close()


def oracle_cells(q_feats, s_feats, kind, K, sample=None, rng=None):
    """or_cosine / or_euclidean of the present cells (all, or `sample` of them at random): (index tuples, distances)."""
    L = O.lib()
    fn = L.or_cosine if kind == "cosine" else L.or_euclidean

    def padded(x):
        out = np.zeros(8 * L.or_feature_blocks(len(x)), np.float32)
        return out, L.or_feature_pad(O.fptr(np.ascontiguousarray(x, np.float32)), len(x), O.fptr(out))

    idx = [(qi, a, ti, b) for qi, qf in enumerate(q_feats) for ti, sf in enumerate(s_feats) for a in range(len(qf)) for b in range(len(sf))]
    if sample is not None and len(idx) > sample:
        idx = [idx[i] for i in rng.choice(len(idx), sample, replace=False)]
    vals = []
    for qi, a, ti, b in idx:
        xa, bx = padded(q_feats[qi][a])
        ya, by = padded(s_feats[ti][b])
        vals.append(fn(O.fptr(xa), bx, O.fptr(ya), by))
    return idx, np.array(vals, np.float32)


def assert_close(kind, got, want):
    both = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    if kind == "cosine":
        assert np.abs(got[both] - want[both]).max() <= 1e-5
    else:
        assert (np.abs(got[both] - want[both]) / np.maximum(np.abs(want[both]), 1e-30)).max() <= 1e-5


@pytest.mark.parametrize("kind", ["cosine", "euclidean"])
@pytest.mark.parametrize("K,D", [(1, 2), (3, 100), (5, 256), (4, 1024)])
def test_cells_against_the_oracle_small(engine, kind, K, D):
    rng = np.random.default_rng(K * 7 + D)
    s_feats = bank(rng, 9, K, D, zero_frac=0.1 if kind == "cosine" else 0.0)
    q_feats = bank(rng, 3, K, D, zero_frac=0.1 if kind == "cosine" else 0.0)
    store = FeatureStore(engine, kind, D, K)
    try:
        store.upsert(np.arange(1, 10), s_feats)
        _, _, _, cells = store.search_raw([100, 101, 102], q_feats, 5, 0.5, tap=True)
    finally:
        store.close()
    idx, want = oracle_cells(q_feats, s_feats, kind, K)
    got = np.array([cells[i] for i in idx], np.float32)
    assert_close(kind, got, want)
    present = np.zeros(cells.shape, bool)
    for i in idx:
        present[i] = True
    assert np.isnan(cells[~present]).all()


@pytest.mark.parametrize("kind", ["cosine", "euclidean"])
def test_cells_against_the_oracle_at_bench_size_sampled(engine, kind):
    rng = np.random.default_rng(5)
    K, D, T, Q = 30, 512, 300, 4
    s_feats = bank(rng, T, K, D, ragged=False)
    q_feats = bank(rng, Q, K, D, ragged=False)
    store = FeatureStore(engine, kind, D, K)
    try:
        store.upsert(np.arange(1, T + 1), s_feats)
        _, _, _, cells = store.search_raw(np.arange(1000, 1000 + Q), q_feats, 5, 0.5, tap=True)
    finally:
        store.close()
    idx, want = oracle_cells(q_feats, s_feats, kind, K, sample=3000, rng=rng)
    assert_close(kind, np.array([cells[i] for i in idx], np.float32), want)


@pytest.mark.parametrize("kind", ["cosine", "euclidean"])
def test_end_to_end_against_oracle_distances(engine, kind):
    """Winners from the engine against the restatement on oracle distances: identical apart from decisions within the distance
    tolerance of max_distance or of a rank boundary, which are counted and bounded."""
    rng = np.random.default_rng(11)
    K, D, T, Q = 3, 64, 60, 12
    s_feats = bank(rng, T, K, D)
    base = [s_feats[i] for i in rng.choice(T, Q)]
    q_feats = [(b + rng.normal(0, 0.05, b.shape)).astype(np.float32) for b in base]   # drifted copies of stored tracks
    store = FeatureStore(engine, kind, D, K)
    try:
        store.upsert(np.arange(1, T + 1), s_feats)
        q_ids = np.arange(1000, 1000 + Q)
        _, _, _, cells = store.search_raw(q_ids, q_feats, 3, 0.5, tap=True)
        exact = np.full(cells.shape, np.nan, np.float32)
        idx, vals = oracle_cells(q_feats, s_feats, kind, K)
        for i, v in zip(idx, vals):
            exact[i] = v
        tol = 1e-5 if kind == "cosine" else 1e-5 * float(np.nanmax(np.abs(exact)))
        for topn, q in ((1, 0.1), (3, 0.3), (10, 0.6)):
            md = distance_quantile(exact, q)
            got = engine_result(*store.search_raw(q_ids, q_feats, topn, md)[:3], q_ids)
            want_eng, _ = R.restate(q_ids, store.order(), cells, topn, md)
            assert got == want_eng
            differ, unexplained, decisions = R.compare_winners(q_ids, store.order(), exact, cells, topn, md, tol)
            assert not unexplained, (unexplained, decisions)
            assert len(differ) <= max(1, decisions), (differ, decisions)
    finally:
        store.close()


def build_store(engine, kind, D, K, mirror, order):
    s = FeatureStore(engine, kind, D, K)
    s.upsert(order, [mirror[int(i)] for i in order])
    return s


def check_mirror(engine, store, mirror, kind, D, K, q_ids, q_feats):
    order = store.order()
    assert sorted(int(i) for i in order) == sorted(mirror) and len(store) == len(mirror)
    fresh = build_store(engine, kind, D, K, mirror, order)
    try:
        a = store.search_raw(q_ids, q_feats, 7, 0.4, tap=True)
        b = fresh.search_raw(q_ids, q_feats, 7, 0.4, tap=True)
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f")
        check_exact(store, q_ids, q_feats, 7, 0.4)
    finally:
        fresh.close()


@pytest.mark.parametrize("kind", ["cosine", "euclidean"])
def test_store_lifecycle_matches_a_host_mirror(engine, kind):
    rng = np.random.default_rng(21)
    K, D = 5, 48
    store = FeatureStore(engine, kind, D, K)
    mirror = {}
    q_ids = np.array([3, 1001, 1002, 1003])
    q_feats = bank(rng, 4, K, D, ragged=False)
    try:
        ids = np.arange(1, 41)
        feats = bank(rng, 40, K, D)
        store.upsert(ids, feats)
        mirror.update({int(i): f for i, f in zip(ids, feats)})
        check_mirror(engine, store, mirror, kind, D, K, q_ids, q_feats)
        rep = np.array([2, 7, 11, 40, 3])
        feats = bank(rng, 5, K, D)
        store.upsert(rep, feats)                                      # replace whole banks
        mirror.update({int(i): f for i, f in zip(rep, feats)})
        check_mirror(engine, store, mirror, kind, D, K, q_ids, q_feats)
        gone = np.array([1, 40, 17, 9999, 5, 39])                      # 9999 is unknown: ignored
        store.remove(gone)
        for i in gone:
            mirror.pop(int(i), None)
        check_mirror(engine, store, mirror, kind, D, K, q_ids, q_feats)
        back = np.array([40, 1])
        feats = bank(rng, 2, K, D)
        store.upsert(back, feats)                                     # re-add
        mirror.update({int(i): f for i, f in zip(back, feats)})
        check_mirror(engine, store, mirror, kind, D, K, q_ids, q_feats)
        more = np.arange(2000, 2150)
        feats = bank(rng, 150, K, D)
        store.upsert(more, feats)                                     # growth past the initial capacity (64) twice
        mirror.update({int(i): f for i, f in zip(more, feats)})
        check_mirror(engine, store, mirror, kind, D, K, q_ids, q_feats)
    finally:
        store.close()


@pytest.mark.parametrize("kind", ["cosine", "euclidean"])
def test_pool_overflow_reruns_the_search(engine, kind):
    """Every group survives: far more groups than the initial pool holds.  The call grows the pool and runs again, with the same
    winners as the restatement and as the next call (which fits)."""
    rng = np.random.default_rng(31)
    K, D, T, Q = 4, 32, 300, 8
    s_ids, s_feats = np.arange(1, T + 1), bank(rng, T, K, D, ragged=False)
    q_ids, q_feats = np.arange(5000, 5000 + Q), bank(rng, Q, K, D, ragged=False)
    store = FeatureStore(engine, kind, D, K)
    try:
        store.upsert(s_ids, s_feats)
        first, _, _ = check_exact(store, q_ids, q_feats, 10, INF)
        st = store.last_stats()
        assert st["reruns"] == 1 and st["groups"] == Q * T and st["pool_bytes"] >= Q * T * K * K * 4
        again, _, _ = check_exact(store, q_ids, q_feats, 10, INF)
        assert store.last_stats()["reruns"] == 0 and again == first
    finally:
        store.close()
    fresh = FeatureStore(engine, kind, D, K)
    try:
        fresh.upsert(s_ids, s_feats)
        assert fresh.search_topn(q_ids, q_feats, 10, INF) == first
    finally:
        fresh.close()


@pytest.mark.parametrize("kind", ["cosine", "euclidean"])
def test_more_candidates_than_the_top_n_workgroup_keeps_in_lds(engine, kind):
    """A query with more surviving groups than launch 2 holds in LDS (2048) ranks them from global memory instead: same winners."""
    rng = np.random.default_rng(51)
    K, D, T = 1, 8, 2600
    store = FeatureStore(engine, kind, D, K)
    try:
        store.upsert(np.arange(1, T + 1), bank(rng, T, K, D, ragged=False))
        q_ids, q_feats = [T + 1, 7], bank(rng, 2, K, D, ragged=False)
        for topn in (1, 64):
            check_exact(store, q_ids, q_feats, topn, INF)
        assert store.last_stats()["groups"] == 2 * T - 1   # query 7 is not paired with stored track 7
    finally:
        store.close()


def test_refusals_leave_the_store_unchanged(engine):
    rng = np.random.default_rng(41)
    K, D = 3, 20
    store = FeatureStore(engine, "cosine", D, K)
    try:
        store.upsert(np.arange(1, 21), bank(rng, 20, K, D))
        q_ids, q_feats = [100, 101], bank(rng, 2, K, D, ragged=False)
        before = (store.order(), store.search_raw(q_ids, q_feats, 5, 0.3, tap=True))
        bad = [
            (abi.SA_ERR_BAD_ARG, lambda: store.search_raw([100, 100], q_feats, 5, 0.3)),
            (abi.SA_ERR_UNSUPPORTED, lambda: store.search_raw(q_ids, q_feats, 65, 0.3)),
            (abi.SA_ERR_BAD_ARG, lambda: store.search_raw(q_ids, [q_feats[0], np.zeros((K + 1, D), np.float32)], 5, 0.3)),
            (abi.SA_ERR_BAD_ARG, lambda: store.search_raw([0, 101], q_feats, 5, 0.3)),
            (abi.SA_ERR_BAD_ARG, lambda: store.upsert([5, 6], [q_feats[0], np.zeros((K + 1, D), np.float32)])),
            (abi.SA_ERR_BAD_ARG, lambda: store.upsert([7, 7], [q_feats[0], q_feats[1]])),
        ]
        for code, call in bad:
            with pytest.raises(EngineError) as ei:
                call()
            assert ei.value.code == code
            after = (store.order(), store.search_raw(q_ids, q_feats, 5, 0.3, tap=True))
            assert np.array_equal(before[0], after[0])
            for x, y in zip(before[1], after[1]):
                assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f")
        # which check speaks: the params before the queries, and of several bad elements the first, whatever its fault
        long = np.zeros((K + 1, D), np.float32)
        for text, call in [
            ("must not be NaN", lambda: store.search_raw([100, 100], q_feats, 5, float("nan"))),
            ("4 observations for id 100", lambda: store.search_raw([100, 0], [long, q_feats[1]], 5, 0.3)),
            ("id 0 at 0", lambda: store.search_raw([0, 101], [q_feats[0], long], 5, 0.3)),
            ("id 100 twice", lambda: store.search_raw([100, 100], [q_feats[0], long], 5, 0.3)),
            ("4 observations for id 5", lambda: store.upsert([5, 0], [long, q_feats[1]])),
            ("id 0 at 1", lambda: store.upsert([5, 0, 5], [q_feats[0], q_feats[1], long])),
        ]:
            with pytest.raises(EngineError, match=text):
                call()
    finally:
        store.close()
    with pytest.raises(EngineError):
        FeatureStore(engine, "cosine", 8, 33)


def test_nan_parameters_and_oversized_searches_are_refused(engine):
    rng = np.random.default_rng(61)
    K, D = 32, 8
    store = FeatureStore(engine, "euclidean", D, K)
    try:
        store.upsert([1, 2], bank(rng, 2, K, D, ragged=False))
        q = bank(rng, 1, K, D, ragged=False)
        for md, kb in ((float("nan"), INF), (1.0, float("nan"))):
            with pytest.raises(EngineError) as ei:
                store.search_raw([9], q, 5, md, keep_below=kb)
            assert ei.value.code == abi.SA_ERR_BAD_ARG
        # 65 536 queries x 32 observation slots: one query slot more than a search's grid can tile (sa_search_limits.h)
        n = 65535 * 32 // K + 1
        with pytest.raises(EngineError) as ei:
            store.search_raw(np.arange(100, 100 + n), [None] * n, 5, 1.0)
        assert ei.value.code == abi.SA_ERR_UNSUPPORTED
        n -= 1
        out_n, _, _, _ = store.search_raw(np.arange(100, 100 + n), [None] * n, 5, 1.0)   # the edge itself: no observations, no winners
        assert not out_n.any()
        assert len(store) == 2
    finally:
        store.close()


def test_an_engine_destroyed_first_orphans_its_store(engine):
    rng = np.random.default_rng(71)
    other = Engine(abi.make_config(device=0))
    store = FeatureStore(other, "cosine", 16, 2)
    store.upsert([1, 2, 3], bank(rng, 3, 2, 16, ragged=False))
    other.close()
    for call in (lambda: store.upsert([4], bank(rng, 1, 2, 16)), lambda: store.remove([1]), lambda: len(store),
                 lambda: store.search_raw([9], bank(rng, 1, 2, 16), 5, 1.0)):
        with pytest.raises(EngineError) as ei:
            call()
        assert ei.value.code == abi.SA_ERR_STATE
    store.close()
    # the module's engine and a store on it are untouched
    s2 = FeatureStore(engine, "cosine", 16, 2)
    try:
        s2.upsert([1, 2, 3], bank(rng, 3, 2, 16, ragged=False))
        check_exact(s2, [9], bank(rng, 1, 2, 16, ragged=False), 5, INF)
    finally:
        s2.close()
