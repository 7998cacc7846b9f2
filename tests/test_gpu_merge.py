"""Bank upkeep on the MI355X (similari_amd.merge.MergeStore over include/similari_merge.h) against tests/merge_ref.py.

No tolerance anywhere.  After every step the device store must hold what the model holds — the order of its slots, every bank's
rows (as uint32), qualities (as uint32) and count — and a host-fed search of it must return the bits the same search returns on a
FRESH store upserted from the model's banks: out_n, winners, weights (as uint64) and every cell (NaN positions as a mask).  Rows
travel with their norms, so this also pins that a moved norm is the norm an upsert computes."""
import math

import numpy as np
import pytest

import merge_ref as R
from similari_amd import abi
from similari_amd.engine import Engine, EngineError
from similari_amd.merge import MergeStore

pytestmark = pytest.mark.gpu
INF = math.inf
KINDS = ["cosine", "euclidean"]


@pytest.fixture(scope="module")
def engine():
    eng = Engine(abi.make_config(device=0))
    yield eng
    eng.close()


def rows(rng, n, D, kind):
    f = rng.uniform(0, 1, (n, D)).astype(np.float32)
    if kind == "cosine":
        f -= np.float32(0.5)
    return f


def same_bits(a, b):
    for x, y in zip(a[:2], b[:2]):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))
    if a[3] is not None or b[3] is not None:
        assert a[3].shape == b[3].shape
        assert np.array_equal(np.isnan(a[3]), np.isnan(b[3]))
        m = ~np.isnan(a[3])
        assert np.array_equal(a[3][m].view(np.uint32), b[3][m].view(np.uint32))


def fresh_from(engine, kind, model):
    st = MergeStore(engine, kind, model.D, model.K)
    if model.order:
        st.upsert(model.order, [model.feats(i) for i in model.order])
    return st


def check_banks(store, model, extra_ids=()):
    assert [int(i) for i in store.order()] == model.order and len(store) == len(model.order)
    ids = list(model.order) + list(extra_ids)
    if not ids:
        return
    n_obs, feats, qual = store.fetch_raw(ids)
    for k, i in enumerate(ids):
        want_f = model.feats(i) if i in model.banks else np.zeros((0, model.D), np.float32)
        want_q = model.quality(i) if i in model.banks else np.zeros(0, np.float32)
        m = len(want_f)
        assert n_obs[k] == m, (i, n_obs[k], m)
        assert np.array_equal(feats[k, :m].view(np.uint32), want_f.view(np.uint32)), i
        assert np.array_equal(qual[k, :m].view(np.uint32), want_q.view(np.uint32)), i
        assert not feats[k, m:].view(np.uint32).any() and not qual[k, m:].view(np.uint32).any()   # unfilled rows: +0.0


def check(engine, kind, store, model, rng, queries=6):
    """banks + a host-fed search against a fresh store of the model's banks (same slot order, so cells compare column by column
    through order())"""
    check_banks(store, model, extra_ids=[10**9])
    if not model.order:
        return
    q_ids = [10**6 + k for k in range(queries - 2)] + model.order[:2]   # foreign queries, and two that meet their own id in the store
    q_feats = [rows(rng, int(rng.integers(0, model.K + 1)), model.D, kind) for _ in q_ids]
    ref = fresh_from(engine, kind, model)
    try:
        assert np.array_equal(ref.order(), store.order())
        a = store.search_raw(q_ids, q_feats, 5, INF, tap=True)
        same_bits(a, ref.search_raw(q_ids, q_feats, 5, INF, tap=True))
        v = a[3][~np.isnan(a[3])]
        md = float(np.quantile(v, 0.3)) if v.size else 0.5
        same_bits(store.search_raw(q_ids, q_feats, 64, md, 2, tap=True), ref.search_raw(q_ids, q_feats, 64, md, 2, tap=True))
    finally:
        ref.close()


def seeded(engine, kind, K, D, T, rng, full=False):
    """A device store and its model: T tracks appended with random qualities (ties on purpose: a few levels only)."""
    store, model = MergeStore(engine, kind, D, K), R.Model(K, D)
    ids = list(range(1, T + 1))
    feats = [rows(rng, K if full else int(rng.integers(0, K + 1)), D, kind) for _ in ids]
    qual = [rng.integers(0, 4, len(f)).astype(np.float32) for f in feats]
    store.append(ids, feats, qual)
    model.append(ids, feats, qual)
    return store, model


# ---- 1. lifecycle parity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", [1, 3, 5, 32])
@pytest.mark.parametrize("D", [2, 100, 1024])
def test_lifecycle_parity(engine, kind, K, D):
    rng = np.random.default_rng(1000 * K + D + (kind == "cosine"))
    T = int(rng.integers(40, 151))
    store, model = seeded(engine, kind, K, D, T, rng)
    nxt = [T + 1]
    did = {"permute": 0, "moved": 0, "created": 0}

    def both(name, *a, **kw):
        getattr(store, name)(*a, **kw)
        getattr(model, name)(*a, **kw)
        check(engine, kind, store, model, rng)

    def some(n):
        return [int(i) for i in rng.choice(model.order, min(n, len(model.order)), replace=False)]

    def step_append():
        ids = some(12) + list(range(nxt[0], nxt[0] + 5))   # known ids (some get no row) and five new ones (one empty)
        nxt[0] += 5
        n = [int(rng.integers(0, K + 1)) for _ in ids]
        n[-1] = 0
        feats = [rows(rng, k, D, kind) for k in n]
        qual = [rng.integers(0, 4, k).astype(np.float32) for k in n]
        cap = [int(rng.integers(1, K + 1)) for _ in ids]
        did["created"] += 5
        both("append", ids, feats, qual, keep=("latest", "best")[int(rng.integers(2))], capacity=cap)

    def step_merge():
        pool = some(min(30, len(model.order)))
        pairs = {}
        while len(pool) >= 4:
            d = pool.pop()
            pairs[d] = [pool.pop() for _ in range(int(rng.integers(0, 4)))]
        cap = {d: int(rng.integers(1, K + 1)) for d in pairs}
        keep = ("latest", "best")[int(rng.integers(2))]
        both("merge", pairs, keep=keep, capacity=cap)
        st = store.merge_stats()
        did["moved"] += st["tracks_moved"]
        did["permute"] += st["rows_rewritten"]
        assert st["launches"] <= 3

    try:
        check(engine, kind, store, model, rng)
        step_append()
        step_merge()
        both("remove", some(5) + [10**7])
        ids = some(4) + [nxt[0]]
        nxt[0] += 1
        both("upsert", ids, [rows(rng, int(rng.integers(0, K + 1)), D, kind) for _ in ids])
        step_merge()
        step_append()
        both("merge", {model.order[-1]: [model.order[0]], model.order[1]: []}, keep="best")
        assert did["moved"] and did["permute"] and did["created"]
    finally:
        store.close()


# ---- 2. in-bank cycles ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", [32, 5])
def test_a_bank_reverses_in_place(engine, kind, K):
    """Ascending qualities under SA_KEEP_BEST with no source: every row of the bank reads another row of the same bank.  Then one
    better row from a source track lands between the own rows."""
    rng = np.random.default_rng(K)
    D = 40
    store, model = MergeStore(engine, kind, D, K), R.Model(K, D)
    try:
        feats = [rows(rng, K, D, kind), rows(rng, K, D, kind), rows(rng, 1, D, kind), rows(rng, 2, D, kind)]
        qual = [np.arange(K, dtype=np.float32), np.arange(K, dtype=np.float32), np.array([K - 1.5], np.float32), np.zeros(2, np.float32)]
        for m in (store, model):
            m.append([11, 12, 13, 14], feats, qual)
        for m in (store, model):
            m.merge({11: []}, keep="best")
        check(engine, kind, store, model, rng)
        assert np.array_equal(store.fetch([11])[11][0], feats[0][::-1]) and store.merge_stats()["rows_rewritten"] == K - K % 2
        for m in (store, model):
            m.merge({12: [13]}, keep="best")
        check(engine, kind, store, model, rng)
        got_f, got_q = store.fetch([12])[12]
        assert list(got_q[:3]) == [K - 1, K - 1.5, K - 2] and np.array_equal(got_f[1], feats[2][0]) and len(got_f) == K
        assert [int(i) for i in store.order()] == [11, 12, 14]
    finally:
        store.close()


# ---- 3. tail cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_tail_cases(engine, kind):
    rng = np.random.default_rng(3)
    K, D = 3, 24
    cases = [
        ("the destination is the last slot, a source is slot 0", lambda o: {o[-1]: [o[0]]}),
        ("the sources are the last slots", lambda o: {o[2]: [o[-1], o[-2]], o[0]: [o[-3]]}),
        ("every track but two is a source of the two others", lambda o: {o[4]: o[:4] + o[6:9], o[5]: o[9:][::-1]}),
        ("a store reduced to one track", lambda o: {o[6]: o[:6] + o[7:]}),
    ]
    for what, pairs_of in cases:
        for keep in ("latest", "best"):
            store, model = seeded(engine, kind, K, D, 12, rng, full=keep == "best")
            try:
                pairs = pairs_of(list(model.order))
                store.merge(pairs, keep=keep, capacity=2 if keep == "latest" else None)
                model.merge(pairs, keep=keep, capacity=2 if keep == "latest" else None)
                check(engine, kind, store, model, rng)
                assert len(store) == 12 - sum(len(v) for v in pairs.values()), what
            finally:
                store.close()


# ---- 4. many at once --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_many_destinations_in_one_call(engine, kind):
    rng = np.random.default_rng(4)
    K, D, N = 2, 32, 3000
    store, model = MergeStore(engine, kind, D, K), R.Model(K, D)
    small = MergeStore(engine, kind, D, K)
    try:
        ids = list(range(1, 2 * N + 1))
        feats = list(rows(rng, 2 * N, D, kind).reshape(2 * N, 1, D))
        qual = list(rng.integers(0, 3, (2 * N, 1)).astype(np.float32))
        for m in (store, model):
            m.append(ids, feats, qual)
        # the sources are the first N slots, the destinations the last N: every destination is rewritten where it lies, then moves
        pairs = {N + 1 + k: [1 + k] for k in range(N)}
        for m in (store, model):
            m.merge(pairs, keep="best")
        st = store.merge_stats()
        assert st["rows_rewritten"] >= N // 2 and st["tracks_moved"] == N and st["device_ms"] > 0
        assert st["bytes_moved"] == (4 * st["rows_rewritten"] + 2 * N * K) * (D * 4 + 4)
        check(engine, kind, store, model, rng)
        small.append([1, 2, 3], feats[:3], qual[:3])
        small.merge({3: [1]}, keep="best")
        one = small.merge_stats()
        assert one["tracks_moved"] == 1 and one["launches"] == st["launches"] == 3
    finally:
        store.close()
        small.close()


# ---- 5. growth --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_append_grows_the_store(engine, kind):
    rng = np.random.default_rng(5)
    K, D = 4, 20
    store, model = seeded(engine, kind, K, D, 60, rng)
    try:
        ids = list(range(1000, 1100))
        feats = [rows(rng, int(rng.integers(0, K + 1)), D, kind) for _ in ids]
        qual = [rng.uniform(-1, 1, len(f)).astype(np.float32) for f in feats]
        for m in (store, model):
            m.append(ids + [7], feats + [rows(np.random.default_rng(0), 1, D, kind)], qual + [[0.5]], keep="best")
        assert len(store) == 160
        check(engine, kind, store, model, rng)
    finally:
        store.close()


# ---- 6. the loop ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_join_merge_join(engine, kind):
    """Tracklets in pairs around common centres: the join names each as the other's top winner, the mutual ones are merged on the
    device, and the next join equals the join of a fresh store built from the model."""
    rng = np.random.default_rng(6)
    K, D, P = 4, 16, 30
    centres = rows(rng, P, D, kind) * 4
    ids = list(range(1, 2 * P + 1))
    # the voting ranks by smallest value and cosine is a similarity: there a tracklet's partner lies around the antipode
    sign = [-1.0 if kind == "cosine" and i % 2 == 0 else 1.0 for i in ids]
    feats = [(s * centres[(i - 1) // 2] + 0.05 * rows(rng, 2, D, kind)).astype(np.float32) for i, s in zip(ids, sign)]
    qual = [rng.integers(0, 3, 2).astype(np.float32) for _ in ids]
    store, model = MergeStore(engine, kind, D, K), R.Model(K, D)
    try:
        for m in (store, model):
            m.append(ids, feats, qual)
        for rnd in range(2):
            _, cells = store.join_topn(1, INF, tap=True)
            v = cells[~np.isnan(cells)]
            md = float(np.quantile(v, 0.5))
            win = {q: lst[0][0] for q, lst in store.join_topn(1, md).items()}
            pairs = {a: [b] for a, b in win.items() if a < b and win.get(b) == a}
            if rnd == 0:
                assert len(pairs) >= 5
            for m in (store, model):
                m.merge(pairs, keep="best")
            check_banks(store, model)
            ref = fresh_from(engine, kind, model)
            try:
                same_bits(store.join_raw(3, md, tap=True), ref.join_raw(3, md, tap=True))
            finally:
                ref.close()
    finally:
        store.close()


# ---- 7. upsert and remove manners -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_upsert_zeroes_and_remove_carries_qualities(engine, kind):
    rng = np.random.default_rng(7)
    K, D = 3, 8
    store, model = seeded(engine, kind, K, D, 9, rng, full=True)
    try:
        last = model.order[-1]
        own = model.quality(last).copy()
        assert store.fetch([2])[2][1].tolist() == model.quality(2).tolist()
        f = rows(rng, 2, D, kind)
        for m in (store, model):
            m.upsert([2], [f])
        assert store.fetch([2])[2][1].tolist() == [0.0, 0.0]
        for m in (store, model):
            m.remove([3])
        assert int(store.order()[2]) == last                      # the last track moved into the hole ...
        assert np.array_equal(store.fetch([last])[last][1], own)  # ... with its own qualities
        check(engine, kind, store, model, rng)
    finally:
        store.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_refusals_leave_the_store_as_it_was(engine, kind):
    rng = np.random.default_rng(8)
    K, D = 3, 8
    store, model = seeded(engine, kind, K, D, 8, rng)
    one = [rows(rng, 1, D, kind)]
    nan = np.array([np.nan], np.float32)
    bad = [
        lambda: store.merge({1: [2], 3: [2]}),            # an id twice: as a source of two
        lambda: store.merge({1: [2], 2: [3]}),            # ... as a source and a destination
        lambda: store.merge({1: [1]}),                    # dst == src
        lambda: store.merge({999: [1]}),                  # unknown destination
        lambda: store.merge({1: [999]}),                  # unknown source
        lambda: store.merge({0: [1]}),
        lambda: store.merge({1: [0]}),
        lambda: store.merge({1: [2]}, capacity=0),
        lambda: store.merge({1: [2]}, capacity=K + 1),
        lambda: store.merge({1: [2]}, keep=2),
        lambda: store.append([0], one),
        lambda: store.append([4, 4], one + one),
        lambda: store.append([4, 50], one + one, [[1.0], nan], keep="best"),
        lambda: store.append([4], one, [nan], keep="latest"),
        lambda: store.append([4, 50], one + one, capacity=[1, 0]),
        lambda: store.append([4], one, capacity=K + 1),
        lambda: store.append([4], one, keep=7),
        lambda: store.append([50, 4], one + [rows(rng, K + 1, D, kind)]),   # n_obs > K, after an id that would have been created
    ]
    try:
        for call in bad:
            with pytest.raises(EngineError) as ei:
                call()
            assert ei.value.code == abi.SA_ERR_BAD_ARG
            check_banks(store, model, extra_ids=[50, 999])
        # which check speaks: the rule of the call before its ids, and of several bad elements the first, whatever its fault
        long = rows(rng, K + 1, D, kind)
        for text, call in [
            ("unknown keep 7", lambda: store.append([0], one, keep=7)),
            ("%d observations for id 50" % (K + 1), lambda: store.append([50, 0], [long] + one)),
            ("id 0 at 1", lambda: store.append([50, 0, 50], one + one + [long])),
            ("id 4 twice", lambda: store.append([4, 4], one + [long])),
            ("unknown keep 2", lambda: store.merge({0: [1]}, keep=2)),
            ("destination id 0", lambda: store.merge({0: [999]})),
            ("unknown destination 999", lambda: store.merge({999: [0]})),
            ("source id 0", lambda: store.merge({1: [0, 999]})),
            ("unknown source 999", lambda: store.merge({1: [999, 0]})),
        ]:
            with pytest.raises(EngineError, match=text):
                call()
            check_banks(store, model, extra_ids=[50, 999])
        check(engine, kind, store, model, rng)
    finally:
        store.close()
