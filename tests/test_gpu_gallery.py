"""The gallery calls on the MI355X (similari_amd.gallery.Gallery over include/similari_gallery.h).

No tolerance anywhere: a join, a search with the stored ids and a search with the same banks uploaded from the host under their own
ids must return the same bits — out_n, winners, weights (compared as uint64) and every cell (NaN positions as a mask) — and all of
them the bits of the host restatement (tests/topn_ref.py, tests/gallery_ref.py) on the join's own cells."""
import ctypes as C
import math

import numpy as np
import pytest

import gallery_ref as G
from similari_amd import abi
from similari_amd.engine import Engine, EngineError
from similari_amd.gallery import Gallery
from similari_amd.search import _p, sa_topn_params

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


def distance_quantile(cells, q):
    v = cells[~np.isnan(cells)]
    return float(np.quantile(v, q)) if v.size else 0.5


def same_bits(a, b):
    """Two raw results (out_n, winners, weights, cells): every bit, NaN positions of the cells as a mask."""
    for x, y in zip(a[:2], b[:2]):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))
    if a[3] is not None or b[3] is not None:
        assert a[3].shape == b[3].shape
        assert np.array_equal(np.isnan(a[3]), np.isnan(b[3]))
        m = ~np.isnan(a[3])
        assert np.array_equal(a[3][m].view(np.uint32), b[3][m].view(np.uint32))


def as_dict(raw, ids):
    out_n, win, wt, _ = raw
    assert np.all(win[np.arange(win.shape[1])[None, :] >= out_n[:, None]] == 0)
    return {int(q): [(int(win[i, r]), float(wt[i, r])) for r in range(int(out_n[i]))] for i, q in enumerate(ids) if out_n[i]}


def three_ways(store, feats_of, topn, md, mv=1, kb=INF):
    """join == stored == foreign == the restatement on the join's cells.  -> (the join's raw result, the restatement)"""
    order = store.order()
    j = store.join_raw(topn, md, mv, kb, tap=True)
    s = store.search_stored_raw(order, topn, md, mv, kb, tap=True)
    f = store.search_raw(order, [feats_of[int(i)] for i in order], topn, md, mv, kb, tap=True)
    same_bits(j, s)
    same_bits(j, f)
    want, _ = G.join(order, j[3], topn, md, mv, kb)
    assert as_dict(j, order) == want
    for q, lst in want.items():   # f64 bits, not float equality
        got = j[2][list(order).index(q)][: len(lst)]
        assert np.array_equal(got.view(np.uint64), np.array([w for _, w in lst], np.float64).view(np.uint64))
    return j, want


def tile_shape(kind):
    return (64, 1) if kind == "cosine" else (32, 4)   # row tile, row tiles per column tile (sa_join_tiles.h)


def tile_count(kind, T, K):
    kp = 1
    while kp < K:
        kp *= 2
    bm, r = tile_shape(kind)
    rows = -(-T * kp // bm)
    cols = -(-rows // r)
    return r * cols * (cols - 1) // 2 + rows, rows * cols, rows


def check_join_stats(store, kind, K, want_pairs):
    st = store.join_stats()
    tiles, rect, rows = tile_count(kind, len(store), K)
    assert st["tiles"] == tiles and st["tiles_rect"] == rect
    # More than one tile row saves a tile in the 64 x 64 triangle.  In the 32 x 128 staircase the first column tile reaches the diagonal
    # of its first four row tiles (n0 + 128 > m0 for m0 = 0, 32, 64, 96), so up to four tile rows every tile of the single column runs
    # and tiles == tiles_rect is the right answer; from the fifth tile row on the count must be smaller.
    if rows > tile_shape(kind)[1]:
        assert st["tiles"] < st["tiles_rect"]
    assert st["blocks"] == want_pairs


def join_case(kind, K, D, T):
    """Ragged banks (15 % zero rows for cosine); from two tracks on, track 1 has no observation and tracks 0 and 2 have all K."""
    rng = np.random.default_rng(100000 * T + 1000 * K + D + (kind == "cosine"))
    ids = rng.choice(np.arange(1, 5000), T, replace=False)
    feats = bank(rng, T, K, D, zero_frac=0.15 if kind == "cosine" else 0.0)
    if T > 1:
        feats[1] = np.zeros((0, D), np.float32)
        feats[0] = rng.uniform(0.1, 1, (K, D)).astype(np.float32)
        feats[2] = rng.uniform(0.1, 1, (K, D)).astype(np.float32)
    return ids, feats


@pytest.mark.parametrize("kind", ["cosine", "euclidean"])
@pytest.mark.parametrize("K", [1, 3, 5, 32])
@pytest.mark.parametrize("D", [2, 100, 1024])
@pytest.mark.parametrize("T", [1, 37, 150])
def test_join_equals_stored_equals_foreign(engine, kind, K, D, T):
    """Items 1, 2 and 7 of the issue.  Not vacuous by construction, asserted for every case of 37 tracks (so in each (kind, K)
    family): stored track 1 has no observation (a query with none); topn = 1 at the median distance fills a row (out_n == topn);
    topn = 64 exceeds the 36 other tracks (0 < out_n < topn); and every surviving pair is seen from its lower and its higher slot."""
    ids, feats = join_case(kind, K, D, T)
    feats_of = {int(i): f for i, f in zip(ids, feats)}
    store = Gallery(engine, kind, D, K)
    try:
        store.upsert(ids, feats)
        order = [int(i) for i in store.order()]
        slot = {i: k for k, i in enumerate(order)}
        j, _ = three_ways(store, feats_of, 5, INF)
        cells = j[3]
        assert cells.shape == (T, K, T, K)
        lo, mid = distance_quantile(cells, 0.05), distance_quantile(cells, 0.5)
        full = empty = partial = lower = higher = False
        for topn, md, mv, kb in ((1, mid, 1, INF), (5, lo, 0, INF), (64, mid, 3, distance_quantile(cells, 0.9)), (64, INF, 1, INF),
                                 (5, mid, 1, distance_quantile(cells, 0.3))):
            j, want = three_ways(store, feats_of, topn, md, mv, kb)
            check_join_stats(store, kind, K, len(G.surviving_pairs(order, cells, md, mv, kb)))
            out_n = j[0]
            full |= bool((out_n == topn).any())
            partial |= bool(((out_n > 0) & (out_n < topn)).any())
            empty |= bool((out_n == 0).any())
            lower |= any(slot[q] < slot[w] for q, lst in want.items() for w, _ in lst)
            higher |= any(slot[q] > slot[w] for q, lst in want.items() for w, _ in lst)
        if T == 1:
            assert empty and not (full or partial or lower or higher)
        if T == 37:
            assert full and partial and empty and lower and higher
    finally:
        store.close()


def order_case(seed, K=32):
    """Two tracks in the plane whose block mixes cosines near -1 with cosines of a few 1e-8: M is tiny, the terms M - d span more
    than 53 bits, and the sequential f64 sum depends on the order it is taken in."""
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


def test_each_direction_of_a_pair_sums_in_its_own_order(engine):
    """Item 3.  The search the issue describes — K = 32, max_distance = inf, one far track to set a large M, row-major against
    column-major sequential f64 sums of a block — finds nothing, and cannot: with d >= 0 every term f32(M - d) is a multiple of
    ulp(M) / 2 and at most M, so 1024 of them sum exactly in 53 bits in any order (300 random blocks with M in [5, 1000]: 0 differ).
    The order shows when M is tiny and the terms are not: cosine of two tracks whose observations are either opposite (d ~ -1,
    terms ~ 1) or orthogonal to 1e-8 (terms ~ 1e-8).  On such blocks the two orders part in the last bits (38 of 40 seeds in
    numpy).  Three seeds are committed; the sums are taken from the engine's own cells, every direction must carry its own, and at
    least one seed must tell the two apart."""
    told_apart = 0
    for seed in (0, 3, 5):
        a, b = order_case(seed)
        store = Gallery(engine, "cosine", 2, 32)
        try:
            store.upsert([10, 20], [a, b])
            assert list(store.order()) == [10, 20]
            out_n, win, wt, cells = store.join_raw(5, INF, tap=True)
            blk = cells[0, :, 1, :]
            assert np.array_equal(blk.view(np.uint32), cells[1, :, 0, :].T.view(np.uint32)) and not np.isnan(blk).any()
            M = blk.max()
            terms = (M - blk).astype(np.float32).astype(np.float64)
            rows_first = float(np.cumsum(terms.reshape(-1))[-1])       # query 10: its observations are the block's rows
            cols_first = float(np.cumsum(terms.T.reshape(-1))[-1])     # query 20: its observations are the block's columns
            assert list(out_n) == [1, 1] and win[0, 0] == 20 and win[1, 0] == 10
            assert wt[0, 0].hex() == rows_first.hex() and wt[1, 0].hex() == cols_first.hex()
            for raw in (store.search_stored_raw([10, 20], 5, INF, tap=True), store.search_raw([10, 20], [a, b], 5, INF, tap=True)):
                same_bits((out_n, win, wt, cells), raw)
            told_apart += rows_first.hex() != cols_first.hex()
        finally:
            store.close()
    assert told_apart >= 1


@pytest.mark.parametrize("kind", ["cosine", "euclidean"])
def test_withdrawal_is_owned_track_distances(engine, kind):
    """Item 4: 6 of 40 stored tracks queried with SA_STORED_WITHDRAW, two more ids the store does not hold."""
    rng = np.random.default_rng(404)
    K, D, T = 4, 24, 40
    ids = np.arange(1, T + 1)
    feats = bank(rng, T, K, D, ragged=False)
    if kind == "euclidean":
        feats[4] = feats[4] + 50.0       # queried tracks 5 and 9 lie far from everything, and farther from each other than any
        feats[8] = feats[8] - 50.0       # other pair: their pair would set M if it counted
    else:
        feats = [f - 0.5 for f in feats]
        feats[4] = np.abs(feats[4]) + 1.0   # tracks 5 and 9: the only two banks in the positive orthant, the largest similarities
        feats[8] = np.abs(feats[8]) + 1.0
    q = np.array([5, 9, 17, 23, 31, 40])
    with_unknown = np.array([5, 777, 9, 17, 23, 31, 888, 40])
    store = Gallery(engine, kind, D, K)
    try:
        store.upsert(ids, feats)
        order = store.order()
        _, _, _, full = store.join_raw(5, INF, tap=True)
        top = np.nanmax(np.where((order[:, None] == order[None, :])[:, None, :, None], np.nan, full))
        s5, s9 = list(order).index(5), list(order).index(9)
        assert np.nanmax(full[s5, :, s9, :]) == top          # the planted pair holds the call's largest distance ...
        masked = full.copy()
        masked[s5, :, s9, :] = masked[s9, :, s5, :] = np.nan
        rest = np.nanmax(np.where((order[:, None] == order[None, :])[:, None, :, None], np.nan, masked))
        assert rest < top                                     # ... and nothing else reaches it
        for who in (q, with_unknown):
            md = distance_quantile(full, 0.4)
            for topn, mv in ((3, 1), (64, 2)):
                raw = store.search_stored_raw(who, topn, md, mv, withdraw=True, tap=True)
                assert np.array_equal(np.isnan(raw[3]), np.isnan(G.rows_of(order, full, who)))
                m = ~np.isnan(raw[3])
                assert np.array_equal(raw[3][m], G.rows_of(order, full, who)[m])   # the cells keep self and withdrawn pairs
                want, M = G.search_stored(order, raw[3], who, topn, md, mv, withdraw=True)
                got = as_dict(raw, who)
                assert got == want and got
                assert not {w for lst in got.values() for w, _ in lst} & set(int(i) for i in who)
                assert M < top and M <= rest
                left_in, M_in = G.search_stored(order, raw[3], who, topn, md, mv)
                assert M_in == top and as_dict(store.search_stored_raw(who, topn, md, mv), who) == left_in != want
                for u in (777, 888):
                    if u in who:
                        k = list(who).index(u)
                        assert raw[0][k] == 0 and np.isnan(raw[3][k]).all() and u not in got
        before = (store.order(), store.join_raw(5, 0.4, tap=True), store.search_stored_raw(q, 5, 0.4, withdraw=True, tap=True))
        bad = [
            lambda: store.search_stored_raw([5, 9, 5], 5, 0.4),
            lambda: store.search_stored_raw([5, 0], 5, 0.4),
            lambda: store.search_stored_raw([5, 9], 5, 0.4, flags=2),
            lambda: store.search_stored_raw([5, 9], 5, 0.4, flags=0x80000001),
            lambda: store.search_stored_raw([5, 9], 5, float("nan")),
            lambda: store.join_raw(5, 0.4, keep_below=float("nan")),
        ]
        for call in bad:
            with pytest.raises(EngineError) as ei:
                call()
            assert ei.value.code == abi.SA_ERR_BAD_ARG
            after = (store.order(), store.join_raw(5, 0.4, tap=True), store.search_stored_raw(q, 5, 0.4, withdraw=True, tap=True))
            assert np.array_equal(before[0], after[0])
            same_bits(before[1], after[1])
            same_bits(before[2], after[2])
        with pytest.raises(EngineError) as ei:
            store.join_raw(65, 0.4)
        assert ei.value.code == abi.SA_ERR_UNSUPPORTED
        # which check speaks: the params, then the flag word — even of a call without queries —, then the ids in their order
        for text, call in [
            ("must not be NaN", lambda: store.search_stored_raw([5, 9], 5, float("nan"), flags=2)),
            ("unknown flag bits 0x2", lambda: store.search_stored_raw([], 5, 0.4, flags=2)),
            ("unknown flag bits 0x2", lambda: store.search_stored_raw([5, 0], 5, 0.4, flags=2)),
            ("id 5 twice", lambda: store.search_stored_raw([5, 5, 0], 5, 0.4)),
            ("id 0 at 1", lambda: store.search_stored_raw([5, 0, 5], 5, 0.4)),
        ]:
            with pytest.raises(EngineError, match=text):
                call()
        assert store.search_stored_raw([], 5, 0.4)[0].size == 0   # no queries: nothing to do, no refusal
        # an empty store: a stored search zeroes the outputs of its queries, a join has none and leaves its outputs as they are
        empty = Gallery(engine, "cosine", D, K)
        try:
            prm = sa_topn_params(2, 1, 0.4, float("inf"))
            for join in (False, True):
                n_, w_, x_ = np.full(2, 7, np.uint32), np.full((2, 2), 7, np.uint64), np.full((2, 2), 7.0)
                outs = (_p(n_, C.c_uint32), _p(w_, C.c_uint64), _p(x_, C.c_double), None)
                two = np.array([5, 9], np.uint64)
                rc = (empty.lib.sa_store_join_topn(empty.h, C.byref(prm), *outs) if join else
                      empty.lib.sa_store_search_stored(empty.h, C.byref(prm), 0, 2, _p(two, C.c_uint64), *outs))
                assert rc == abi.SA_OK
                want = 7 if join else 0
                assert (n_ == want).all() and (w_ == want).all() and (x_ == want).all()
        finally:
            empty.close()
    finally:
        store.close()


@pytest.mark.parametrize("kind", ["cosine", "euclidean"])
def test_lifecycle_join_still_equals_foreign(engine, kind):
    """Item 5, after the pattern of test_store_lifecycle_matches_a_host_mirror: replaced banks, compacting removals, re-adds, growth."""
    rng = np.random.default_rng(21)
    K, D = 5, 48
    store = Gallery(engine, kind, D, K)
    mirror = {}

    def check():
        assert sorted(int(i) for i in store.order()) == sorted(mirror) and len(store) == len(mirror)
        j, _ = three_ways(store, mirror, 7, INF)
        three_ways(store, mirror, 7, distance_quantile(j[3], 0.2), 2)

    try:
        ids = np.arange(1, 41)
        feats = bank(rng, 40, K, D)
        store.upsert(ids, feats)
        mirror.update({int(i): f for i, f in zip(ids, feats)})
        check()
        rep = np.array([2, 7, 11, 40, 3])
        feats = bank(rng, 5, K, D)
        store.upsert(rep, feats)
        mirror.update({int(i): f for i, f in zip(rep, feats)})
        check()
        gone = np.array([1, 40, 17, 9999, 5, 39])
        store.remove(gone)
        for i in gone:
            mirror.pop(int(i), None)
        check()
        back = np.array([40, 1])
        feats = bank(rng, 2, K, D)
        store.upsert(back, feats)
        mirror.update({int(i): f for i, f in zip(back, feats)})
        check()
        more = np.arange(2000, 2150)
        feats = bank(rng, 150, K, D)
        store.upsert(more, feats)
        mirror.update({int(i): f for i, f in zip(more, feats)})
        check()
    finally:
        store.close()


@pytest.mark.parametrize("kind", ["cosine", "euclidean"])
def test_pool_overflow_reruns_the_join(engine, kind):
    """Item 6a: a fresh store, 60 tracks that all pair: 1770 blocks against a first pool of 256."""
    rng = np.random.default_rng(31)
    K, D, T = 4, 32, 60
    ids, feats = np.arange(1, T + 1), bank(rng, T, K, D, ragged=False)
    feats_of = {int(i): f for i, f in zip(ids, feats)}
    store = Gallery(engine, kind, D, K)
    try:
        store.upsert(ids, feats)
        first = store.join_raw(10, INF, tap=True)
        st = store.last_stats()
        assert st["reruns"] == 1 and st["groups"] == T * (T - 1) // 2 > 256 and store.join_stats()["blocks"] == st["groups"]
        assert st["pool_bytes"] >= st["groups"] * K * K * 4
        same_bits(first, store.search_raw(ids, feats, 10, INF, tap=True))
        again, _ = three_ways(store, feats_of, 10, INF)
        assert store.last_stats()["reruns"] == 0
        same_bits(first, again)
    finally:
        store.close()


@pytest.mark.parametrize("kind", ["cosine", "euclidean"])
def test_more_groups_per_query_than_lds_holds(engine, kind):
    """Item 6b: 2100 tracks of one observation, everything kept: 2099 groups per query, beyond the 2048 that launch 2 keeps in LDS,
    so weights go through global memory — two per block, one per direction."""
    rng = np.random.default_rng(51)
    K, D, T = 1, 8, 2100
    ids, feats = np.arange(1, T + 1), bank(rng, T, K, D, ragged=False)
    store = Gallery(engine, kind, D, K)
    try:
        store.upsert(ids, feats)
        for topn in (1, 64):
            j = store.join_raw(topn, INF, tap=True)
            same_bits(j, store.search_raw(ids, feats, topn, INF, tap=True))
            same_bits(j, store.search_stored_raw(ids, topn, INF, tap=True))
            assert (j[0] == topn).all()
        assert store.join_stats()["blocks"] == T * (T - 1) // 2
        # the restatement for one observation per track, a row at a time: weight f64(f32(M - d)), ranked by (weight desc, id asc)
        d = j[3][:, 0, :, 0]
        assert not np.isnan(d).any()
        M = d[~np.eye(T, dtype=bool)].max()
        w = (M - d).astype(np.float32).astype(np.float64)
        for qi in range(T):
            rank = np.lexsort((ids, -w[qi]))
            rank = rank[rank != qi][:64]
            assert np.array_equal(j[1][qi], ids[rank].astype(np.uint64))
            assert np.array_equal(j[2][qi].view(np.uint64), w[qi][rank].view(np.uint64))
    finally:
        store.close()


def test_a_join_beyond_the_pair_limit_is_refused(engine):
    """Item 8: 65 536 tracks: T * T = 2^32 >= 2^32 - 1.  Refused before anything is allocated: the pool has no bytes yet.
    (The largest join the limit admits needs 4 T^2 = 17 GB for grp alone; it is not run here.)"""
    T, D = 65536, 2
    store = Gallery(engine, "euclidean", D, 1)
    try:
        store.upsert(np.arange(1, T + 1), list(np.zeros((T, 1, D), np.float32)))
        with pytest.raises(EngineError) as ei:
            store.join_raw(1, 1.0)
        assert ei.value.code == abi.SA_ERR_UNSUPPORTED
        assert store.last_stats()["pool_bytes"] == 0 and len(store) == T
    finally:
        store.close()


@pytest.mark.parametrize("kind,T", [("cosine", 11600), ("euclidean", 8200)])
def test_a_join_with_more_tiles_than_one_grid_dimension_holds(engine, kind, T):
    """32 observation slots per track and enough tracks that launch 1 has 2^24 tiles of 256 threads (cosine) or 2^23 of 512 (euclidean)
    and more: 2^32 work-items, beyond one dimension of a dispatch.  One observation per track in the plane keeps it light.  The first
    and the last stored track are planted as a surviving pair — its tile is the first of the last column, in the grid's last rows."""
    rng = np.random.default_rng(77)
    K, D = 32, 2
    ids = np.arange(1, T + 1)
    feats = list(rng.uniform(0.05, 1, (T, 1, D)).astype(np.float32))
    if kind == "cosine":
        feats[0], feats[-1], md = np.array([[1, 0]], np.float32), np.array([[0, 1]], np.float32), 0.002   # similarity 0: kept
    else:
        feats[0], md = feats[-1].copy(), 0.001
    store = Gallery(engine, kind, D, K)
    try:
        store.upsert(ids, feats)
        j = store.join_raw(5, md)
        st = store.join_stats()
        threads = 256 if kind == "cosine" else 512
        assert st["tiles"] == tile_count(kind, T, K)[0] and st["tiles"] * threads >= 2**32
        same_bits(j, store.search_raw(ids, feats, 5, md))
        same_bits(j, store.search_stored_raw(ids, 5, md))
        got = as_dict(j, ids)
        assert T in [w for w, _ in got[1]] and 1 in [w for w, _ in got[T]]
        assert 0 < st["blocks"] == sum(len(v) for v in as_dict(store.join_raw(64, md), ids).values()) // 2
    finally:
        store.close()
