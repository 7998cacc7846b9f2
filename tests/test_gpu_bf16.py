"""bf16 feature stores on the MI355X (similari_amd.bf16.Bf16Store over include/similari_bf16.h).

A bf16 store is an f32 store fed with bf16(x) for every feature value, contracted with f32 accumulation.  So every statement the
suite makes about an f32 store is made here against rounded rows (tests/bf16_ref.py), with the tolerances the suite already has:
none for winners, weights, fetched rows and the three forms of a search; 1e-5 for a cosine cell against f64, the bound of
test_gpu_search.assert_close — products of bf16 values are exact in f32, only the order of the f32 additions differs."""
import math

import numpy as np
import pytest

import bestfit_ref as BF
import bf16_ref as B
import compat_ref as X
import gallery_ref as G
import topn_ref as R
from similari_amd import abi, attrs as A
from similari_amd.bestfit import BestFitStore
from similari_amd.bf16 import SA_ELEM_BF16, SA_ELEM_F32, Bf16Store, store_info
from similari_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu
INF = math.inf
u32, u64 = np.uint32, np.uint64


@pytest.fixture(scope="module")
def engine():
    eng = Engine(abi.make_config(device=0))
    yield eng
    eng.close()


def bank(rng, n, K, D, ragged=True, zero_frac=0.0):
    out = []
    for _ in range(n):
        k = int(rng.integers(0, K + 1)) if ragged else K
        f = rng.uniform(0, 1, (k, D)).astype(np.float32)
        f[rng.uniform(size=k) < zero_frac] = 0.0
        out.append(f)
    return out


def engine_result(out_n, win, wt, q_ids):
    return {int(q): [(int(win[i, r]), float(wt[i, r])) for r in range(int(out_n[i]))] for i, q in enumerate(q_ids) if out_n[i]}


def distance_quantile(cells, q):
    v = cells[~np.isnan(cells)]
    return float(np.quantile(v, q)) if v.size else 0.5


def same_bits(a, b):
    """Two raw results (out_n, winners, weights, cells): every bit, NaN positions of the cells as a mask."""
    for x, y in zip(a[:2], b[:2]):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert np.array_equal(a[2].view(u64), b[2].view(u64))
    if a[3] is not None or b[3] is not None:
        assert a[3].shape == b[3].shape
        assert np.array_equal(np.isnan(a[3]), np.isnan(b[3]))
        m = ~np.isnan(a[3])
        assert np.array_equal(a[3][m].view(u32), b[3][m].view(u32))


def same_rows(got, want):
    assert got.shape == want.shape and np.array_equal(got.view(u32), np.ascontiguousarray(want, np.float32).view(u32))


# ---- 1. fetch returns the rounded rows ------------------------------------------------------------------------------------------
def fetched_equal(store, ids, feats):
    n_obs, got, _ = store.fetch_raw(ids)
    for k, f in enumerate(feats):
        assert n_obs[k] == len(f)
        same_rows(got[k, : len(f)], B.round_bf16(f))
        assert not got[k, len(f):].view(u32).any()   # unfilled rows: +0.0
    return n_obs, got


@pytest.mark.parametrize("D", [2, 16, 17, 100])
def test_fetch_returns_the_rounded_rows(engine, D):
    rng = np.random.default_rng(300 + D)
    K, T = 3, 21
    ids = np.arange(1, T + 1)
    feats = bank(rng, T, K, D)
    feats[0] = (rng.normal(0, 100, (K, D))).astype(np.float32)   # both signs, other binades
    store = Bf16Store(engine, "cosine", D, K)
    try:
        store.upsert(ids, feats)
        n_obs, got = fetched_equal(store, ids, feats)
        store.upsert(ids, [got[k, : n_obs[k]] for k in range(T)])   # rounding is idempotent: feeding back changes no bit
        fetched_equal(store, ids, feats)
        more = [rng.uniform(0, 1, (1, D)).astype(np.float32) if len(f) < K else np.zeros((0, D), np.float32) for f in feats]
        store.append(ids, more)                                       # the append rounds as the upsert does
        fetched_equal(store, ids, [np.concatenate([f, m]) for f, m in zip(feats, more)])
    finally:
        store.close()


# ---- 2. winners equal the restatement on the engine's own cells -----------------------------------------------------------------
# The 16-bit tile (search_tile_h16, sa_gemm.hip) walks a row of Dp / 32 chunks through a ring of four.  Fewer than 8 chunks take the guarded
# turns alone: 1-4 chunks one turn, 5-7 a second turn that reloads 1-3 slots.  From 8 chunks on the branch-free steady state runs
# while 8 chunks remain and leaves 4 + (chunks % 4) to the guarded turns: 4 (8, 16, 32 chunks), 5 (9), 6 (10), 7 (11).
# D = 32 n - 3, so that the last chunk is ragged: 3, 5, 6, 7, 10 and 11 chunks.
RING_D = [93, 157, 189, 221, 317, 349]


def check_exact(store, q_ids, q_feats, topn, md, mv=1, kb=INF):
    """The engine's winners == the restatement on the engine's own cells (every bit of every weight)."""
    out_n, win, wt, cells = store.search_raw(q_ids, q_feats, topn, md, mv, kb, tap=True)
    want, M = R.restate(q_ids, store.order(), cells, topn, md, mv, kb)
    got = engine_result(out_n, win, wt, q_ids)
    assert got == want
    for i, q in enumerate(q_ids):   # f64 bits, not float equality
        lst = want.get(int(q), [])
        assert np.array_equal(wt[i, : len(lst)].view(u64), np.array([w for _, w in lst], np.float64).view(u64))
    assert np.all(win[np.arange(win.shape[1])[None, :] >= out_n[:, None]] == 0)
    return got, cells, M


@pytest.mark.parametrize("K", [1, 3, 32])
@pytest.mark.parametrize("D", [2, 17, 100, 1024])
def test_winners_equal_the_restatement_on_the_engines_cells(engine, K, D):
    winners_case(engine, K, D)


@pytest.mark.parametrize("D", RING_D)
def test_winners_equal_the_restatement_at_every_chunk_count_of_the_ring(engine, D):
    winners_case(engine, 3, D)


def winners_case(engine, K, D):
    rng = np.random.default_rng(1000 * K + D + 1)
    T, Q = 37, 6
    s_ids = rng.choice(np.arange(1, 500), T, replace=False)
    q_ids = np.concatenate([s_ids[:3], rng.choice(np.arange(500, 900), Q - 3, replace=False)])   # three queries are stored too
    store = Bf16Store(engine, "cosine", D, K)
    try:
        store.upsert(s_ids, bank(rng, T, K, D, zero_frac=0.15))
        q_feats = bank(rng, Q, K, D, zero_frac=0.15)
        q_feats[1] = np.zeros((0, D), np.float32)   # a query without observations: no pairs
        _, cells, _ = check_exact(store, q_ids, q_feats, 5, INF)
        lo, mid = distance_quantile(cells, 0.05), distance_quantile(cells, 0.5)
        for topn, md, mv, kb in ((1, mid, 1, INF), (5, lo, 0, INF), (64, mid, 3, distance_quantile(cells, 0.9)), (64, INF, 1, INF),
                                 (5, mid, 1, distance_quantile(cells, 0.3))):
            check_exact(store, q_ids, q_feats, topn, md, mv, kb)
    finally:
        store.close()


# ---- 3. cells against f64 on the rounded inputs ---------------------------------------------------------------------------------
def tap_cells(engine, K, D, s_feats, q_feats):
    store = Bf16Store(engine, "cosine", D, K)
    try:
        store.upsert(np.arange(1, len(s_feats) + 1), s_feats)
        return store.search_raw(np.arange(10**6, 10**6 + len(q_feats)), q_feats, 5, 0.5, tap=True)[3]
    finally:
        store.close()


def assert_cells(got, want, tol=1e-5):
    """got f32 cells, want f64 cells (same shape): the NaN pattern is identical and |got - want| <= tol.  -> the maximum"""
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    both = ~np.isnan(want)
    err = float(np.abs(got[both].astype(np.float64) - want[both]).max())
    print("max |cell - f64 of the rounded rows| = %.3g over %d cells" % (err, int(both.sum())))
    assert err <= tol
    return err


# 1, 4, 8 and 32 chunks, then every other count of RING_D.  (K per D so that the seeded ragged banks leave at least 30 cells: the
# draw of K = 4 at D = 189, for one, is three queries without a row)
@pytest.mark.parametrize("K,D", [(1, 2), (2, 16), (2, 17), (3, 100), (5, 256), (4, 1024)] + list(zip((3, 2, 3, 4, 3, 4), RING_D)))
def test_cells_against_f64_of_the_rounded_rows(engine, K, D):
    rng = np.random.default_rng(K * 7 + D)
    s_feats = bank(rng, 9, K, D, zero_frac=0.1)
    q_feats = bank(rng, 3, K, D, zero_frac=0.1)
    cells = tap_cells(engine, K, D, s_feats, q_feats)
    want = B.cosine_f64(B.round_banks(q_feats), B.round_banks(s_feats), K)
    assert np.isfinite(want).any() and (D not in RING_D or np.isfinite(want).sum() >= 30)
    assert_cells(cells, want)


def test_cells_at_the_reid_width_tell_rounded_from_unrounded_rows(engine):
    """K = 32, D = 512: 3000 sampled cells within 1e-5 of f64 on the ROUNDED rows, and the same cells further than 1e-5 from the
    cosine of the rows as given — rounding moves a cell by about 2e-4 here, so the gate can tell the two statements apart."""
    rng = np.random.default_rng(5)
    K, D, T, Q = 32, 512, 70, 4
    s_feats = bank(rng, T, K, D, ragged=False)
    q_feats = bank(rng, Q, K, D, ragged=False)
    cells = tap_cells(engine, K, D, s_feats, q_feats)
    assert cells.shape == (Q, K, T, K) and not np.isnan(cells).any()
    pick = rng.choice(cells.size, 3000, replace=False)
    got = cells.reshape(-1)[pick]
    assert_cells(got, B.cosine_f64(B.round_banks(q_feats), B.round_banks(s_feats), K).reshape(-1)[pick])
    moved = float(np.abs(got.astype(np.float64) - B.cosine_f64(q_feats, s_feats, K).reshape(-1)[pick]).max())
    print("max |cell - f64 of the rows as given| = %.3g" % moved)
    assert moved > 1e-5


# ---- 4. join == stored == host-fed --------------------------------------------------------------------------------------------
def as_dict(raw, ids):
    out_n, win, wt = raw[:3]
    assert np.all(win[np.arange(win.shape[1])[None, :] >= out_n[:, None]] == 0)
    return {int(q): [(int(win[i, r]), float(wt[i, r])) for r in range(int(out_n[i]))] for i, q in enumerate(ids) if out_n[i]}


def weight_bits(raw, ids, want):
    for i, q in enumerate(ids):
        lst = want.get(int(q), [])
        assert raw[0][i] == len(lst)
        assert np.array_equal(raw[2][i][: len(lst)].view(u64), np.array([w for _, w in lst], np.float64).view(u64))


def three_ways(store, topn, md, mv=1, kb=INF):
    """join == stored == host-fed with the FETCHED rows == the restatement on the join's cells"""
    order = store.order()
    fetched = store.fetch(order)
    j = store.join_raw(topn, md, mv, kb, tap=True)
    s = store.search_stored_raw(order, topn, md, mv, kb, tap=True)
    f = store.search_raw(order, [fetched[int(i)][0] for i in order], topn, md, mv, kb, tap=True)
    same_bits(j, s)
    same_bits(j, f)
    want, _ = G.join(order, j[3], topn, md, mv, kb)
    assert as_dict(j, order) == want
    weight_bits(j, order, want)
    return j


@pytest.mark.parametrize("T,K,D", [(37, 5, 100), (130, 1, 64)])
def test_join_equals_stored_equals_host_fed(engine, T, K, D):
    rng = np.random.default_rng(100000 * T + 1000 * K + D)
    ids = rng.choice(np.arange(1, 5000), T, replace=False)
    feats = bank(rng, T, K, D, zero_frac=0.15)
    feats[1] = np.zeros((0, D), np.float32)
    feats[0], feats[2] = (rng.uniform(0.1, 1, (K, D)).astype(np.float32) for _ in range(2))
    store = Bf16Store(engine, "cosine", D, K)
    try:
        store.upsert(ids, feats)
        order = store.order()
        cells = three_ways(store, 5, INF)[3]
        assert cells.shape == (T, K, T, K)
        flat = cells.reshape(T * K, T * K)
        m = ~np.isnan(flat)
        assert np.array_equal(m, m.T) and np.array_equal(flat[m].view(u32), flat.T[m].view(u32))   # symmetric to the bit
        lo, mid = distance_quantile(cells, 0.05), distance_quantile(cells, 0.5)
        for topn, md, mv, kb in ((1, mid, 1, INF), (5, lo, 0, INF), (64, mid, min(3, K), distance_quantile(cells, 0.9))):
            j = three_ways(store, topn, md, mv, kb)
            assert j[0].any()
        sub = [int(i) for i in order[::3]] + [9999]   # withdrawn: the queried tracks leave the store for the call
        for withdraw in (False, True):
            s = store.search_stored_raw(sub, 5, mid, 1, INF, withdraw, tap=True)
            want, _ = G.search_stored(order, s[3], sub, 5, mid, 1, INF, withdraw)
            assert as_dict(s, sub) == want and want
            weight_bits(s, sub, want)
            same_bits(s[:3] + (None,), store.search_stored_raw(sub, 5, mid, 1, INF, withdraw)[:3] + (None,))
            if withdraw:
                assert not {w for lst in want.values() for w, _ in lst} & set(sub)
    finally:
        store.close()


# ---- 5. a search after append + merge returns the bits of a freshly upserted store ---------------------------------------------
def check_against_fresh(engine, store, model, rng):
    assert [int(i) for i in store.order()] == model.order
    n_obs, feats, qual = store.fetch_raw(model.order)
    for k, i in enumerate(model.order):
        m = len(model.feats(i))
        assert n_obs[k] == m
        same_rows(feats[k, :m], model.feats(i))
        assert np.array_equal(qual[k, :m].view(u32), model.quality(i).view(u32))
    q_ids = [10**6 + k for k in range(4)] + model.order[:2]
    q_feats = [rng.uniform(0, 1, (int(rng.integers(0, model.K + 1)), model.D)).astype(np.float32) - np.float32(0.5) for _ in q_ids]
    ref = Bf16Store(engine, "cosine", model.D, model.K)
    try:
        ref.upsert(model.order, [model.feats(i) for i in model.order])
        a = store.search_raw(q_ids, q_feats, 5, INF, tap=True)
        same_bits(a, ref.search_raw(q_ids, q_feats, 5, INF, tap=True))
        md = distance_quantile(a[3], 0.3)
        same_bits(store.search_raw(q_ids, q_feats, 64, md, 2, tap=True), ref.search_raw(q_ids, q_feats, 64, md, 2, tap=True))
        assert a[0].any()
    finally:
        ref.close()


@pytest.mark.parametrize("keep", ["latest", "best"])
def test_append_and_merge_leave_what_a_fresh_store_holds(engine, keep):
    rng = np.random.default_rng(77 + (keep == "best"))
    K, D, T = 4, 100, 20
    store, model = Bf16Store(engine, "cosine", D, K), B.Model(K, D)
    try:
        ids = list(range(1, T + 1))
        feats = [rng.uniform(0, 1, (int(rng.integers(2, K + 1)), D)).astype(np.float32) - np.float32(0.5) for _ in ids]
        qual = [rng.integers(0, 4, len(f)).astype(np.float32) for f in feats]
        for m in (store, model):
            m.append(ids, feats, qual, keep=keep)
        check_against_fresh(engine, store, model, rng)
        more = [rng.uniform(0, 1, (int(rng.integers(0, K + 1)), D)).astype(np.float32) - np.float32(0.5) for _ in ids[:8]]
        mq = [rng.integers(0, 4, len(f)).astype(np.float32) for f in more]
        new = rng.uniform(0, 1, (1, D)).astype(np.float32)
        for m in (store, model):   # known ids (some get no row) and a new one, under a capacity below K
            m.append(ids[:8] + [100], more + [new], mq + [np.ones(1, np.float32)], keep=keep, capacity=3)
        check_against_fresh(engine, store, model, rng)
        pairs = {2: [19, 7], 11: [3], 5: []}
        merged = sum(len(model.feats(i)) for i in (2, 19, 7))
        assert merged > 3   # a capacity below the merged count: the rule drops rows
        for m in (store, model):
            m.merge(pairs, keep=keep, capacity={2: 3, 11: 2, 5: 1})
        assert store.merge_stats()["tracks_moved"] > 0
        check_against_fresh(engine, store, model, rng)
    finally:
        store.close()


# ---- 6. compat and BestFit -------------------------------------------------------------------------------------------------------
def attr_case(engine, seed):
    rng = np.random.default_rng(seed)
    T, K, D, Q = 37, 3, 100, 9
    ids = np.arange(1, T + 1) * 3
    feats = [rng.uniform(0, 1, (K if i % 3 == 0 else int(rng.integers(1, K + 1)), D)).astype(np.float32) - np.float32(0.5) for i in range(T)]
    spans = lambda n: [(int(rng.integers(1, 3)), int(s), int(s + rng.integers(0, 40))) for s in rng.integers(0, 100, n)]
    packed = lambda at: A.pack_attrs([a[0] for a in at], [a[1] for a in at], [a[2] for a in at])
    s_attrs, q_attrs = spans(T), spans(Q)
    q_ids = np.arange(1, Q + 1) * 3 + 1000
    q_ids[0] = ids[T // 2]   # one query carries a stored id
    q_feats = [rng.uniform(0, 1, (int(rng.integers(1, K + 1)), D)).astype(np.float32) - np.float32(0.5) for _ in range(Q)]
    store = Bf16Store(engine, "cosine", D, K)
    store.upsert(ids, feats)
    store.set_attrs_raw(ids, packed(s_attrs))
    return store, ids, s_attrs, q_ids, q_feats, q_attrs, packed


def test_compat_on_a_bf16_store(engine):
    store, ids, s_attrs, q_ids, q_feats, q_attrs, packed = attr_case(engine, 61)
    try:
        rule = A.compat(same_key=True, disjoint=True)
        order = store.order()
        lv = X.live_matrix(rule, q_attrs, s_attrs)
        assert 0.0 < lv.mean() < 1.0
        md = distance_quantile(store.search_raw(q_ids, q_feats, 5, INF, tap=True)[3], 0.5)
        for topn, mv in ((5, 2), (64, 1)):
            raw = store.search_raw(q_ids, q_feats, topn, md, mv, tap=True, compat=rule, q_attrs=packed(q_attrs))
            want, _ = X.restate(q_ids, order, raw[3], rule, q_attrs, s_attrs, topn, md, mv)
            assert want and as_dict(raw, q_ids) == want
            weight_bits(raw, q_ids, want)
            same_bits(raw[:3] + (None,), store.search_raw(q_ids, q_feats, topn, md, mv, compat=rule, q_attrs=packed(q_attrs))[:3] + (None,))
            sub = [int(i) for i in order[::2]]
            s = store.search_stored_raw(sub, topn, md, mv, tap=True, compat=rule)
            want, _ = X.search_stored(order, s[3], sub, rule, s_attrs, topn, md, mv)
            assert want and as_dict(s, sub) == want
            weight_bits(s, sub, want)
            j = store.join_raw(topn, md, mv, tap=True, compat=rule)
            want, _ = X.join(order, j[3], rule, s_attrs, topn, md, mv)
            assert want and as_dict(j, order) == want
            weight_bits(j, order, want)
            same_bits(j[:3] + (None,), store.join_raw(topn, md, mv, compat=rule)[:3] + (None,))
    finally:
        store.close()


def fit_equals(raw, q_ids, want, topn):
    out_n, win, trk, wt = raw[:4]
    res = BF.cut(want[0], topn)
    for i, q in enumerate(q_ids):
        lst = res.get(int(q), [])
        n = len(lst)
        assert out_n[i] == n
        assert [int(x) for x in trk[i, :n]] == [t for _, _, t in lst]
        assert [int(x) for x in win[i, :n]] == [w for w, _, _ in lst]
        assert np.array_equal(wt[i, :n].view(u64), np.array([w for _, w, _ in lst], np.float64).view(u64))
        assert not win[i, n:].any() and not trk[i, n:].any() and not wt[i, n:].view(u64).any()


def test_bestfit_on_a_bf16_store(engine):
    store, ids, s_attrs, q_ids, q_feats, q_attrs, packed = attr_case(engine, 62)
    try:
        order = store.order()
        md = distance_quantile(store.search_raw(q_ids, q_feats, 5, INF, tap=True)[3], 0.6)
        raw = store.search_bestfit_raw(q_ids, q_feats, 5, md, tap=True)
        want = BF.restate(q_ids, order, raw[4], md)
        assert want[1] > want[2] > 0   # some group lost its track to a better claimant
        fit_equals(raw, q_ids, want, 5)
        st = store.bestfit_stats()
        assert (st["groups"], st["claimed"]) == (want[1], want[2])
        j = store.join_bestfit_raw(1, md, tap=True)
        want = BF.join(order, j[4], md)
        assert want[0]
        fit_equals(j, order, want, 1)
        rule = A.compat(same_key=True, disjoint=True)
        j = store.join_bestfit_raw(1, md, tap=True, compat=rule)
        fit_equals(j, order, BF.join(order, j[4], md, rule=rule, s_attrs=s_attrs), 1)
    finally:
        store.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_come_with_a_message(engine):
    with pytest.raises(EngineError, match="cosine only") as ei:
        Bf16Store(engine, "euclidean", 16, 2)
    assert ei.value.code == abi.SA_ERR_UNSUPPORTED
    with pytest.raises(EngineError, match="unknown element type 7") as ei:
        Bf16Store(engine, "cosine", 16, 2, elem=7)
    assert ei.value.code == abi.SA_ERR_BAD_ARG
    with pytest.raises(EngineError) as ei:   # what sa_store_create refuses is refused here too
        Bf16Store(engine, "cosine", 16, 33)
    assert ei.value.code == abi.SA_ERR_UNSUPPORTED


# ---- 8. an f32 store and a bf16 store on one engine ---------------------------------------------------------------------------
def test_an_f32_and_a_bf16_store_side_by_side(engine):
    rng = np.random.default_rng(81)
    K, D, T, Q = 3, 100, 37, 6
    ids, feats = np.arange(1, T + 1), bank(rng, T, K, D)
    q_ids, q_feats = np.arange(1000, 1000 + Q), bank(rng, Q, K, D, ragged=False)
    f32, b16 = BestFitStore(engine, "cosine", D, K), Bf16Store(engine, "cosine", D, K)
    as_f32 = Bf16Store(engine, "cosine", D, K, elem=SA_ELEM_F32)   # SA_ELEM_F32 is sa_store_create itself
    try:
        for s in (f32, b16, as_f32):
            s.upsert(ids, feats)
        first = [s.search_raw(q_ids, q_feats, 5, 0.8, tap=True) for s in (f32, b16)]
        for _ in range(2):
            for s, want in zip((f32, b16), first):
                same_bits(s.search_raw(q_ids, q_feats, 5, 0.8, tap=True), want)
                same_bits(s.join_raw(3, 0.8, tap=True), s.search_stored_raw(s.order(), 3, 0.8, tap=True))
        same_bits(as_f32.search_raw(q_ids, q_feats, 5, 0.8, tap=True), first[0])
        m = ~np.isnan(first[0][3])
        assert not np.array_equal(first[0][3][m].view(u32), first[1][3][m].view(u32))   # their own results: the rows differ
        same_rows(f32.fetch_raw(ids)[1], np.stack([np.concatenate([f, np.zeros((K - len(f), D), np.float32)]) for f in feats]))
    finally:
        for s in (f32, b16, as_f32):
            s.close()


# ---- 9. info -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,D", [(3, 100), (32, 512), (1, 2)])
def test_info(engine, K, D):
    rng = np.random.default_rng(91)
    T = 70   # past the first capacity of 64
    f32, b16 = BestFitStore(engine, "cosine", D, K), Bf16Store(engine, "cosine", D, K)
    try:
        assert b16.info()["feature_bytes"] == 0
        for s in (f32, b16):
            s.upsert(np.arange(1, T + 1), bank(rng, T, K, D, ragged=False))
        a, b = store_info(f32), b16.info()
        kp = 1 << (K - 1).bit_length()
        assert (a["elem"], b["elem"]) == (SA_ELEM_F32, SA_ELEM_BF16)
        for i in (a, b):
            assert i["struct_size"] == 24 and i["Dp"] == -(-D // 32) * 32 and i["Kp"] == kp
        assert a["feature_bytes"] == 128 * kp * a["Dp"] * 4 and 2 * b["feature_bytes"] == a["feature_bytes"]
    finally:
        f32.close()
        b16.close()
