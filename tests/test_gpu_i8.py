"""int8 feature stores on the MI355X (similari_amd.i8.I8Store over include/similari_i8.h).

An i8 store is an f32 store fed with codes(x) for every row (tests/i8_ref.py), and from there everything is integers: the dot
products and the squared norms are exact, a cell is f32(dot) / sqrtf(f32(na) * f32(nb)).  So every statement here is an equality —
fetched rows against the model's codes, the tapped cells against the numpy f32 formula on int64 sums, winners and f64 weights against
the restatement on the engine's own cells, the three forms of a search, device-fed against host-fed calls, absorb against
search + append — except one: a cell against f64, within 5e-7.  That bound is derived, not measured: the conversions of dot, na and
nb, the product and the square root (half a rounding on the result) and the quotient are 4.5 roundings of 2^-24 on |cell| <= 1,
2.7e-7."""
import math

import numpy as np
import pytest

import bestfit_ref as BF
import compat_ref as X
import devrows_ref as DRef
import i8_ref as I
import test_gpu_absorb as TA
import test_gpu_bf16 as TB
import test_gpu_devrows as TD
import test_gpu_retain as TR
from similari_amd import abi, attrs as A
from similari_amd.bf16 import store_info
from similari_amd.devrows import DeviceRows
from similari_amd.engine import Engine, EngineError
from similari_amd.i8 import SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_F32, SA_ELEM_I8, I8Store
from similari_amd.retain import RetainStore

pytestmark = pytest.mark.gpu
INF = math.inf
u16, u32, u64, f32 = np.uint16, np.uint32, np.uint64, np.float32
CELL_TOL = 5e-7


@pytest.fixture(scope="module")
def engine():
    eng = Engine(abi.make_config(device=0))
    yield eng
    eng.close()


def bank(rng, n, K, D, ragged=True, zero_frac=0.0):
    """n observation arrays of both signs; a zero_frac of the rows is all zeros (a ZERO ROW: NaN cells)"""
    out = []
    for _ in range(n):
        k = int(rng.integers(0, K + 1)) if ragged else K
        f = rng.normal(0, 1, (k, D)).astype(f32)
        f[rng.uniform(size=k) < zero_frac] = 0.0
        out.append(f)
    return out


def same_codes(got, want):
    assert got.shape == want.shape and np.array_equal(got.view(u32), np.ascontiguousarray(want, f32).view(u32))


# ---- 1. fetch returns the codes -------------------------------------------------------------------------------------------------
def fetched_equal(store, ids, feats):
    n_obs, got, _ = store.fetch_raw(ids)
    for k, f in enumerate(feats):
        assert n_obs[k] == len(f)
        same_codes(got[k, : len(f)], I.codes(f))
        assert not got[k, len(f):].view(u32).any()   # unfilled rows: +0.0
    return n_obs, got


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("D", [1, 2, 63, 64, 65, 100])
def test_fetch_returns_the_models_codes(engine, D, K):
    rng = np.random.default_rng(300 + 10 * D + K)
    T = 21
    ids = np.arange(1, T + 1)
    feats = bank(rng, T, K, D)
    feats[0] = rng.normal(0, 100, (K, D)).astype(f32)             # other binades
    feats[1] = np.zeros((K, D), f32)                              # ZERO ROWS
    feats[2] = rng.normal(0, 1, (K, D)).astype(f32)
    feats[2][0, D // 2] = np.nan                                  # a NaN anywhere: a ZERO ROW
    feats[3] = rng.normal(0, 1, (K, D)).astype(f32)
    feats[3][0, D - 1] = f32(-3e38)                               # one huge element: -127 there, zeros elsewhere
    feats[4] = rng.normal(0, 1, (K, D)).astype(f32)
    feats[4][0, 0] = np.inf
    feats[5] = np.clip(rng.normal(0, 1, (K, D)) * 2.0**-101, -(2.0**-101), 2.0**-101).astype(f32)   # all below the floor of 2^-100
    feats[6] = ((rng.integers(-126, 126, (K, D)) + 0.5) / 8).astype(f32)   # m = 127 / 8, inv = 8: every other product is a tie
    feats[6][:, 0] = f32(127 / 8)
    store = I8Store(engine, "cosine", D, K)
    try:
        store.upsert(ids, feats)
        n_obs, got = fetched_equal(store, ids, feats)
        assert not got[1].any() and not got[2][0].any() and not got[4][0].any() and not got[5].any()
        assert got[3][0, D - 1] == -127 and np.count_nonzero(got[3][0]) == 1
        store.upsert(ids, [got[k, : n_obs[k]] for k in range(T)])     # directions, not lengths: feeding back changes no bit
        n_obs2, again, _ = store.fetch_raw(ids)
        assert np.array_equal(n_obs, n_obs2) and np.array_equal(got.view(u32), again.view(u32))
        more = [rng.normal(0, 1, (1, D)).astype(f32) if len(f) < K else np.zeros((0, D), f32) for f in feats]
        store.append(ids, more)                                       # the append codes as the upsert does
        want = [np.concatenate([I.codes(f), I.codes(m)]) for f, m in zip(feats, more)]
        n_obs, got, _ = store.fetch_raw(ids)
        for k, w in enumerate(want):
            assert n_obs[k] == len(w)
            same_codes(got[k, : len(w)], w)
    finally:
        store.close()


# ---- 2. layout and exactness ----------------------------------------------------------------------------------------------------
# The tile (search_tile_h16 with ELEM = SA_ELEM_I8, sa_gemm.hip) walks a row of Dp / 64 chunks through a ring of four.  Fewer than 8
# chunks take the guarded turns alone: 1-4 chunks one turn, 5-7 a second turn that reloads 1-3 slots.  From 8 chunks on the
# branch-free steady state runs while 8 chunks remain and leaves 4 + (chunks % 4) to the guarded turns.
RING_NCH = [1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 17]


def integer_rows(rng, n, D):
    """rows that are their own codes: integers in -127 .. 127, every row with a +-127; asymmetric and k-dependent — a ramp in k that
    differs per row under random values — so that an operand taking other bytes than its partner, or a lane half left out, changes
    a dot product"""
    k = np.arange(D)
    x = rng.integers(-127, 128, (n, D))
    ramp = ((k[None, :] * (2 * np.arange(n)[:, None] + 3) + 5 * np.arange(n)[:, None]) % 61) - 30
    x = np.clip(x // 2 + ramp, -126, 126)
    x[np.arange(n), (7 * np.arange(n) + 3) % D] = np.where(np.arange(n) % 2, -127, 127)
    return x.astype(f32)


def assert_cells(got, want32, want64):
    """got == want32 bit for bit (NaN pattern included), and within CELL_TOL of f64"""
    assert got.shape == want32.shape and np.array_equal(np.isnan(got), np.isnan(want32))
    m = ~np.isnan(want32)
    err = float(np.abs(got[m].astype(np.float64) - want64[m]).max())
    bits = int((got[m].view(u32) != want32[m].view(u32)).sum())
    print("max |cell - f64| = %.3g over %d cells; %d cells differ from the f32 formula" % (err, int(m.sum()), bits))
    assert err <= CELL_TOL
    assert bits == 0


@pytest.mark.parametrize("D", [64 * n for n in RING_NCH] + [64 * 8 + 1])
def test_cells_are_the_f32_formula_on_exact_integers(engine, D):
    rng = np.random.default_rng(4000 + D)
    T, Q = 70, 5                                                   # 70 rows: the 64-row tile edge is crossed, on both sides in the join
    rows = integer_rows(rng, T, D)
    assert np.array_equal(I.codes(rows), rows)                    # codes equal values
    q_rows = integer_rows(np.random.default_rng(5000 + D), Q, D)[::-1].copy()
    store = I8Store(engine, "cosine", D, 1)
    try:
        ids = np.arange(1, T + 1)
        store.upsert(ids, [r[None, :] for r in rows])
        same_codes(store.fetch_raw(ids)[1][:, 0], rows)
        j = store.join_raw(3, INF, tap=True)[3].reshape(T, T)
        assert_cells(j, I.cells_f32(rows, rows), I.cells_f64(rows, rows))
        assert np.array_equal(j.view(u32), j.T.copy().view(u32))                        # cell (i, j) == cell (j, i)
        assert np.array_equal(np.diag(j).view(u32), np.full(T, f32(1)).view(u32))       # equal codes: exactly 1.0f
        s = store.search_raw(np.arange(1000, 1000 + Q), [r[None, :] for r in q_rows], 3, INF, tap=True)[3].reshape(Q, T)
        assert_cells(s, I.cells_f32(q_rows, rows), I.cells_f64(q_rows, rows))
    finally:
        store.close()


# ---- 3. the widest row ----------------------------------------------------------------------------------------------------------
def test_the_widest_row_overflows_nothing(engine):
    D = 131072
    rng = np.random.default_rng(6)
    sign = np.where(rng.integers(0, 2, D), f32(1), f32(-1)).astype(f32)
    c = f32(0.37)
    store = I8Store(engine, "cosine", D, 1)
    try:
        assert store.info()["Dp"] == D
        store.upsert([1, 2], [(c * sign)[None, :], (-c * sign)[None, :]])
        cells = store.search_raw([9], [(f32(5) * sign)[None, :]], 2, INF, tap=True)[3].reshape(2)
        assert np.array_equal(cells.view(u32), np.array([1, -1], f32).view(u32))        # 127^2 D = 2114060288 in the accumulator and the norms
        j = store.join_raw(1, INF, tap=True)[3].reshape(2, 2)
        assert np.array_equal(j.view(u32), np.array([[1, -1], [-1, 1]], f32).view(u32))
    finally:
        store.close()
    with pytest.raises(EngineError, match="feature_len 131073 above 131072") as ei:
        I8Store(engine, "cosine", D + 1, 1)
    assert ei.value.code == abi.SA_ERR_UNSUPPORTED


# ---- 4. winners and f64 weights equal the restatement on the engine's own cells -------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 32])
@pytest.mark.parametrize("D", [2, 65, 100, 1024])
def test_winners_equal_the_restatement_on_the_engines_cells(engine, K, D):
    rng = np.random.default_rng(1000 * K + D + 1)
    T, Q = 37, 6
    s_ids = rng.choice(np.arange(1, 500), T, replace=False)
    q_ids = np.concatenate([s_ids[:3], rng.choice(np.arange(500, 900), Q - 3, replace=False)])   # three queries are stored too
    store = I8Store(engine, "cosine", D, K)
    try:
        s_feats = bank(rng, T, K, D, zero_frac=0.15)
        store.upsert(s_ids, s_feats)
        q_feats = bank(rng, Q, K, D, ragged=K > 1, zero_frac=0.15)   # (K = 1: a ragged draw can leave no query with a row)
        q_feats[0] = rng.normal(0, 1, (K, D)).astype(f32)
        q_feats[1] = np.zeros((0, D), f32)   # a query without observations: no pairs
        _, cells, _ = TB.check_exact(store, q_ids, q_feats, 5, INF)
        want = I.tap(q_feats, s_feats, K)     # and the cells are the model's, NaN for absent observations and zero rows alike
        assert np.array_equal(np.isnan(cells), np.isnan(want))
        m = ~np.isnan(want)
        assert m.any() and np.array_equal(cells[m].view(u32), want[m].view(u32))
        lo, mid = TB.distance_quantile(cells, 0.05), TB.distance_quantile(cells, 0.5)
        for topn, md, mv, kb in ((1, mid, 1, INF), (5, lo, 0, INF), (64, mid, 3, TB.distance_quantile(cells, 0.9)), (64, INF, 1, INF),
                                 (5, mid, 1, TB.distance_quantile(cells, 0.3))):
            TB.check_exact(store, q_ids, q_feats, topn, md, mv, kb)
    finally:
        store.close()


# ---- 5. the surface -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,K,D", [(37, 5, 100), (130, 1, 64)])
def test_join_equals_stored_equals_host_fed(engine, T, K, D):
    rng = np.random.default_rng(100000 * T + 1000 * K + D)
    ids = rng.choice(np.arange(1, 5000), T, replace=False)
    feats = bank(rng, T, K, D, zero_frac=0.15)
    feats[1] = np.zeros((0, D), f32)
    feats[0], feats[2] = (rng.normal(0, 1, (K, D)).astype(f32) for _ in range(2))
    store = I8Store(engine, "cosine", D, K)
    try:
        store.upsert(ids, feats)
        order = store.order()
        cells = TB.three_ways(store, 5, INF)[3]      # host-fed with the FETCHED rows: the codes, fed back
        assert cells.shape == (T, K, T, K)
        flat = cells.reshape(T * K, T * K)
        m = ~np.isnan(flat)
        assert np.array_equal(m, m.T) and np.array_equal(flat[m].view(u32), flat.T[m].view(u32))   # symmetric to the bit
        lo, mid = TB.distance_quantile(cells, 0.05), TB.distance_quantile(cells, 0.5)
        for topn, md, mv, kb in ((1, mid, 1, INF), (5, lo, 0, INF), (64, mid, min(3, K), TB.distance_quantile(cells, 0.9))):
            j = TB.three_ways(store, topn, md, mv, kb)
            assert j[0].any()
    finally:
        store.close()


def check_against_fresh(engine, store, model, rng):
    assert [int(i) for i in store.order()] == model.order
    n_obs, feats, qual = store.fetch_raw(model.order)
    for k, i in enumerate(model.order):
        m = len(model.feats(i))
        assert n_obs[k] == m
        same_codes(feats[k, :m], model.feats(i))
        assert np.array_equal(qual[k, :m].view(u32), model.quality(i).view(u32))
    q_ids = [10**6 + k for k in range(4)] + model.order[:2]
    q_feats = [rng.normal(0, 1, (int(rng.integers(0, model.K + 1)), model.D)).astype(f32) for _ in q_ids]
    ref = I8Store(engine, "cosine", model.D, model.K)
    try:
        ref.upsert(model.order, [model.feats(i) for i in model.order])
        a = store.search_raw(q_ids, q_feats, 5, INF, tap=True)
        TB.same_bits(a, ref.search_raw(q_ids, q_feats, 5, INF, tap=True))
        md = TB.distance_quantile(a[3], 0.3)
        TB.same_bits(store.search_raw(q_ids, q_feats, 64, md, 2, tap=True), ref.search_raw(q_ids, q_feats, 64, md, 2, tap=True))
        assert a[0].any()
    finally:
        ref.close()


@pytest.mark.parametrize("keep", ["latest", "best"])
def test_append_and_merge_leave_what_a_fresh_store_holds(engine, keep):
    rng = np.random.default_rng(77 + (keep == "best"))
    K, D, T = 4, 100, 20
    store, model = I8Store(engine, "cosine", D, K), I.Model(K, D)
    try:
        ids = list(range(1, T + 1))
        feats = [rng.normal(0, 1, (int(rng.integers(2, K + 1)), D)).astype(f32) for _ in ids]
        qual = [rng.integers(0, 4, len(f)).astype(f32) for f in feats]
        for m in (store, model):
            m.append(ids, feats, qual, keep=keep)
        check_against_fresh(engine, store, model, rng)
        more = [rng.normal(0, 1, (int(rng.integers(0, K + 1)), D)).astype(f32) for _ in ids[:8]]
        mq = [rng.integers(0, 4, len(f)).astype(f32) for f in more]
        new = rng.normal(0, 1, (1, D)).astype(f32)
        for m in (store, model):   # known ids (some get no row) and a new one, under a capacity below K
            m.append(ids[:8] + [100], more + [new], mq + [np.ones(1, f32)], keep=keep, capacity=3)
        check_against_fresh(engine, store, model, rng)
        pairs = {2: [19, 7], 11: [3], 5: []}
        assert sum(len(model.feats(i)) for i in (2, 19, 7)) > 3   # a capacity below the merged count: the rule drops rows
        for m in (store, model):
            m.merge(pairs, keep=keep, capacity={2: 3, 11: 2, 5: 1})
        assert store.merge_stats()["tracks_moved"] > 0
        check_against_fresh(engine, store, model, rng)
    finally:
        store.close()


def attr_case(engine, seed):
    rng = np.random.default_rng(seed)
    T, K, D, Q = 37, 3, 100, 9
    ids = np.arange(1, T + 1) * 3
    feats = [rng.uniform(0, 1, (K if i % 3 == 0 else int(rng.integers(1, K + 1)), D)).astype(f32) - f32(0.5) for i in range(T)]
    spans = lambda n: [(int(rng.integers(1, 3)), int(s), int(s + rng.integers(0, 40))) for s in rng.integers(0, 100, n)]
    packed = lambda at: A.pack_attrs([a[0] for a in at], [a[1] for a in at], [a[2] for a in at])
    s_attrs, q_attrs = spans(T), spans(Q)
    q_ids = np.arange(1, Q + 1) * 3 + 1000
    q_ids[0] = ids[T // 2]   # one query carries a stored id
    q_feats = [rng.uniform(0, 1, (int(rng.integers(1, K + 1)), D)).astype(f32) - f32(0.5) for _ in range(Q)]
    store = I8Store(engine, "cosine", D, K)
    store.upsert(ids, feats)
    store.set_attrs_raw(ids, packed(s_attrs))
    return store, ids, s_attrs, q_ids, q_feats, q_attrs, packed


def test_compat_on_an_i8_store(engine):
    store, ids, s_attrs, q_ids, q_feats, q_attrs, packed = attr_case(engine, 61)
    try:
        rule = A.compat(same_key=True, disjoint=True)
        order = store.order()
        assert 0.0 < X.live_matrix(rule, q_attrs, s_attrs).mean() < 1.0
        md = TB.distance_quantile(store.search_raw(q_ids, q_feats, 5, INF, tap=True)[3], 0.5)
        for topn, mv in ((5, 2), (64, 1)):
            raw = store.search_raw(q_ids, q_feats, topn, md, mv, tap=True, compat=rule, q_attrs=packed(q_attrs))
            want, _ = X.restate(q_ids, order, raw[3], rule, q_attrs, s_attrs, topn, md, mv)
            assert want and TB.as_dict(raw, q_ids) == want
            TB.weight_bits(raw, q_ids, want)
            j = store.join_raw(topn, md, mv, tap=True, compat=rule)
            want, _ = X.join(order, j[3], rule, s_attrs, topn, md, mv)
            assert want and TB.as_dict(j, order) == want
            TB.weight_bits(j, order, want)
    finally:
        store.close()


def test_bestfit_on_an_i8_store(engine):
    store, ids, s_attrs, q_ids, q_feats, q_attrs, packed = attr_case(engine, 62)
    try:
        order = store.order()
        md = TB.distance_quantile(store.search_raw(q_ids, q_feats, 5, INF, tap=True)[3], 0.6)
        raw = store.search_bestfit_raw(q_ids, q_feats, 5, md, tap=True)
        want = BF.restate(q_ids, order, raw[4], md)
        assert want[1] > want[2] > 0   # some group lost its track to a better claimant
        TB.fit_equals(raw, q_ids, want, 5)
        st = store.bestfit_stats()
        assert (st["groups"], st["claimed"]) == (want[1], want[2])
        j = store.join_bestfit_raw(1, md, tap=True)
        want = BF.join(order, j[4], md)
        assert want[0]
        TB.fit_equals(j, order, want, 1)
    finally:
        store.close()


def absorb_frame(rng, a):
    """70 queries against the 70 stored tracks: every other one built on a stored track (each named once), the rest far from
    everything; every count of observations, none among them"""
    stored = [int(i) for i in a.order()]
    on = [stored[k] if k % 2 == 0 else None for k in range(70)]
    n_obs = [int(m) for m in rng.integers(0, a.K + 1, 70)]
    n_obs[:4] = [1, 2, 3, 0]
    return on, n_obs, TA.queries_on(rng, a, on, n_obs)


@pytest.mark.parametrize("keep", ["latest", "best"])
def test_absorb_equals_search_bestfit_then_append(engine, keep):
    rng = np.random.default_rng(90 + (keep == "best"))
    D, K, T = 100, 3, 70
    ids = np.arange(1, T + 1, dtype=u64)
    banks = [rng.normal(0, 1, (int(m), D)).astype(f32) for m in rng.integers(1, K + 1, T)]
    a, b = I8Store(engine, "cosine", D, K), I8Store(engine, "cosine", D, K)
    try:
        quality = [rng.uniform(0, 1, len(x)).astype(f32) for x in banks]
        for s in (a, b):
            s.append(ids, banks, quality, "latest")
        for frame in range(2):                                    # the second frame under "best" ranks by the device's mirror
            on, n_obs, feats = absorb_frame(rng, a)
            q_ids = np.arange(1000 + 100 * frame, 1070 + 100 * frame, dtype=u64)
            q_quality = [rng.uniform(0, 1, m).astype(f32) for m in n_obs]
            if keep == "latest":
                dest, st = TA.step(rng, a, b, q_ids, feats, 2, TA.CUT["cosine"], q_quality, 2)
            else:
                dest, st = TR.step(rng, a, b, q_ids, feats, 2, TA.CUT["cosine"], q_quality, 2)
            named = sum(1 for t, m in zip(on, n_obs) if t is not None and m)
            assert st["matched"] == named >= 20 and st["created"] == 70 - named and st["launches"] == 3
    finally:
        a.close()
        b.close()


SRC_NAME = {SA_ELEM_F32: "f32", SA_ELEM_F16: "f16", SA_ELEM_BF16: "bf16"}


@pytest.mark.parametrize("src", [SA_ELEM_F32, SA_ELEM_F16, SA_ELEM_BF16], ids=lambda e: "from_" + SRC_NAME[e])
def test_rows_from_device_memory_leave_the_bits_of_the_host_fed_calls(engine, src):
    """D = 33, rows D + 3 elements apart, gathered through an index: an upsert, a search and an absorb of rows in a device block
    against the same calls fed widen(rows) from the host.  The source carries a subnormal row, +-0, +-inf and NaNs
    (test_gpu_devrows.make_source): ZERO ROWS by either route."""
    rng = np.random.default_rng(700 + src)
    D, K, T = 33, TD.K, TD.T
    stride, eb = D + 3, DRef.ELEM_BYTES[src]
    ids = np.arange(1, T + 1, dtype=u64)
    n_obs = TD.ragged(rng, T)
    total = int(n_obs.sum())
    n_rows = total + 3
    bits = TD.make_source(rng, n_rows, D, src)
    index = rng.permutation(n_rows)[:total].astype(u32)
    wide = DRef.widen(bits, src)
    a, b = I8Store(engine, "cosine", D, K), I8Store(engine, "cosine", D, K)
    try:
        with TD.device_block(engine, TD.lay_rows(bits, stride, 1)) as ptr:
            base = ptr + eb                                        # the rows start one element into the block: 16-bit rows at odd addresses too
            dr = DeviceRows(base, n_rows, stride, src, index)
            a.upsert_rows(ids, n_obs, dr)
            st = a.devrows_stats()
            banks = TD.banks_of(wide, n_obs, index)
            b.upsert(ids, banks)
            TD.same_store(a, b)
            TD.same_search(rng, a, b, D)
            assert st["rows"] == total and st["src_bytes"] == total * D * eb and st["wide_rows"] == 0   # no row at a multiple of 8 or 16 bytes
            got = a.fetch_raw(ids)[1]
            with np.errstate(invalid="ignore", over="ignore"):
                for t, f in enumerate(banks):                      # and both hold the model's codes
                    same_codes(got[t, : len(f)], I.codes(f))
            # a search fed from the block against the host-fed one, TopN and BestFit
            q_ids = np.arange(5000, 5000 + 6, dtype=u64)
            q_n = np.array([1, 0, 3, 2, 3, 1], u32)
            q_index = rng.permutation(n_rows)[: int(q_n.sum())].astype(u32)
            q_dr = DeviceRows(base, n_rows, stride, src, q_index)
            q_banks = TD.banks_of(wide, q_n, q_index)
            TD.same_out(a.search_rows_raw(q_ids, q_n, q_dr, 3, TD.FAR, tap=True), b.search_raw(q_ids, q_banks, 3, TD.FAR, tap=True))
            TD.same_out(a.search_rows_raw(q_ids, q_n, q_dr, 3, TD.FAR, vote="bestfit", tap=True), b.search_bestfit_raw(q_ids, q_banks, 3, TD.FAR, tap=True))
        # absorb_rows: queries built on stored rows, laid out in a block of the source's element type
        for frame, keep in enumerate(("latest", "best")):
            stored = [int(i) for i in a.order() if len(a.fetch([i])[int(i)][0]) and a.fetch([i])[int(i)][0][0].any()]   # a first row that is no ZERO ROW
            on = [stored[0], None, stored[2], stored[3], None, stored[4]]
            f_n = np.array([1, 2, 3, 0, 1, 2], u32)
            f_total = int(f_n.sum())
            rows = np.concatenate(TA.queries_on(rng, a, on, f_n))
            f_index = rng.permutation(f_total + 2)[:f_total].astype(u32)
            f_bits = np.zeros((f_total + 2, D), f32 if src == SA_ELEM_F32 else u16)
            f_bits[f_index] = rows if src == SA_ELEM_F32 else TA.to_bits(rows, src)
            f_ids = np.arange(300 + 10 * frame, 306 + 10 * frame, dtype=u64)
            quality = rng.uniform(0, 1, f_total).astype(f32)
            f_banks = TD.banks_of(DRef.widen(f_bits, src), f_n, f_index)
            f_quality = [quality[int(f_n[:i].sum()): int(f_n[: i + 1].sum())] for i in range(len(f_n))]
            with TD.device_block(engine, TD.lay_rows(f_bits, stride, 0)) as ptr:
                f_dr = DeviceRows(ptr, f_total + 2, stride, src, f_index)
                if keep == "latest":
                    got = a.absorb_rows_raw(f_ids, f_n, f_dr, 2, TA.CUT["cosine"], quality=quality, capacity=2)
                    want = b.absorb_raw(f_ids, f_banks, 2, TA.CUT["cosine"], quality=f_quality, capacity=2)
                else:
                    got = a.absorb_keep_rows_raw(f_ids, f_n, f_dr, 2, TA.CUT["cosine"], quality=quality, capacity=2)
                    want = b.absorb_keep_raw(f_ids, f_banks, 2, TA.CUT["cosine"], quality=f_quality, capacity=2)
                assert a.devrows_stats() == {"rows": f_total, "wide_rows": f_total, "src_bytes": f_total * D * eb}   # every row by the wide load
                a.upsert_rows([900 + frame], [2], DeviceRows(ptr, f_total + 2, stride, src, f_index[:2]))   # and an upsert by that route
                b.upsert([900 + frame], [DRef.widen(f_bits, src)[f_index[:2]]])
            TA.same_out(got, want)
            TA.same_stores(rng, a, b)
            assert a.absorb_stats()["matched"] >= 2
    finally:
        a.close()
        b.close()


# ---- 6. refusals and info -------------------------------------------------------------------------------------------------------
def test_refusals_come_with_a_message(engine):
    with pytest.raises(EngineError, match="an i8 store is cosine only") as ei:
        I8Store(engine, "euclidean", 16, 2)
    assert ei.value.code == abi.SA_ERR_UNSUPPORTED
    with pytest.raises(EngineError) as ei:   # what sa_store_create refuses is refused here too
        I8Store(engine, "cosine", 16, 33)
    assert ei.value.code == abi.SA_ERR_UNSUPPORTED
    with pytest.raises(EngineError, match="unknown element type 8") as ei:   # sa_store_create_elem is as it was
        RetainStore(engine, "cosine", 16, 2, SA_ELEM_I8)
    assert ei.value.code == abi.SA_ERR_BAD_ARG
    store = I8Store(engine, "cosine", 16, 2)
    try:
        with pytest.raises(EngineError, match="unknown element type 8 of rows") as ei:   # source rows of int8 are not offered
            store.upsert_rows([1], [1], DeviceRows(0x1000, 1, 16, SA_ELEM_I8))
        assert ei.value.code == abi.SA_ERR_BAD_ARG and len(store) == 0
    finally:
        store.close()


@pytest.mark.parametrize("K,D", [(3, 100), (32, 512), (1, 2), (2, 65)])
def test_info(engine, K, D):
    rng = np.random.default_rng(91)
    T = 70   # past the first capacity of 64
    f32s, i8s = RetainStore(engine, "cosine", D, K, SA_ELEM_F32), I8Store(engine, "cosine", D, K)
    try:
        assert i8s.info()["feature_bytes"] == 0
        for s in (f32s, i8s):
            s.upsert(np.arange(1, T + 1), bank(rng, T, K, D, ragged=False))
        a, b = store_info(f32s), i8s.info()
        kp = 1 << (K - 1).bit_length()
        assert (a["elem"], b["elem"]) == (SA_ELEM_F32, SA_ELEM_I8) and SA_ELEM_I8 == 8
        assert b["struct_size"] == 24 and b["Kp"] == kp and b["Dp"] == -(-D // 64) * 64 and b["Dp"] % 64 == 0
        assert b["feature_bytes"] == 128 * kp * b["Dp"]
        if D == 512:
            assert 4 * b["feature_bytes"] == a["feature_bytes"]   # exactly a quarter
    finally:
        f32s.close()
        i8s.close()


def test_an_f32_and_an_i8_store_side_by_side(engine):
    rng = np.random.default_rng(81)
    K, D, T, Q = 3, 100, 37, 6
    ids, feats = np.arange(1, T + 1), bank(rng, T, K, D)
    q_ids, q_feats = np.arange(1000, 1000 + Q), bank(rng, Q, K, D, ragged=False)
    f32s, i8s = RetainStore(engine, "cosine", D, K, SA_ELEM_F32), I8Store(engine, "cosine", D, K)
    try:
        for s in (f32s, i8s):
            s.upsert(ids, feats)
        first = [s.search_raw(q_ids, q_feats, 5, 0.8, tap=True) for s in (f32s, i8s)]
        for _ in range(2):
            for s, want in zip((f32s, i8s), first):
                TB.same_bits(s.search_raw(q_ids, q_feats, 5, 0.8, tap=True), want)
                TB.same_bits(s.join_raw(3, 0.8, tap=True), s.search_stored_raw(s.order(), 3, 0.8, tap=True))
        m = ~np.isnan(first[0][3])
        assert not np.array_equal(first[0][3][m].view(u32), first[1][3][m].view(u32))   # their own results: the rows differ
        print("largest move of a cosine under the coding at D = %d: %.3g" % (D, float(np.abs(first[0][3][m].astype(np.float64) - first[1][3][m]).max())))
        TB.same_rows(f32s.fetch_raw(ids)[1], np.stack([np.concatenate([f, np.zeros((K - len(f), D), f32)]) for f in feats]))
    finally:
        f32s.close()
        i8s.close()
