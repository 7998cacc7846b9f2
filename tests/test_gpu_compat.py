"""The attribute gates on the MI355X (similari_amd.attrs.AttrStore over include/similari_attrs.h).

No tolerance anywhere: winners, counts and f64 weight bits of a search under a rule equal the host restatement
(tests/compat_ref.py) on that call's own tap cells, a call without the tap — whose dead tiles leave early — returns the bits of
the call with it, and the three forms of a search (join, stored ids, host-fed banks) return the same bits under the same rule."""
import ctypes as C
import math

import numpy as np
import pytest

import compat_ref as X
import merge_ref
from similari_amd import abi, attrs as A
from similari_amd.attrs import AttrStore
from similari_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu
INF = math.inf
KINDS = ["cosine", "euclidean"]


@pytest.fixture(scope="module")
def engine():
    eng = Engine(abi.make_config(device=0))
    yield eng
    eng.close()


def kp_of(K):
    kp = 1
    while kp < K:
        kp *= 2
    return kp


def rule_of(flags, ready_at=X.INT64_MAX):
    return A.Compat(flags, ready_at)


def banks(rng, n, K, D, kind, ragged=True):
    out = []
    for i in range(n):
        k = int(rng.integers(1, K + 1)) if ragged and i % 3 else K
        f = rng.uniform(0, 1, (k, D)).astype(np.float32)
        out.append(f - 0.5 if kind == "cosine" else f)
    return out


def spans(rng, n):
    start = rng.integers(0, 100, n)
    return [(int(rng.integers(1, 3)), int(s), int(s + rng.integers(0, 40))) for s in start]


def packed(attrs):
    return A.pack_attrs([a[0] for a in attrs], [a[1] for a in attrs], [a[2] for a in attrs])


def build(engine, kind, D, K, ids, feats, s_attrs):
    store = AttrStore(engine, kind, D, K)
    store.upsert(ids, feats)
    store.set_attrs_raw(ids, packed(s_attrs))
    return store


def case(kind, T, K, Q, D, seed):
    rng = np.random.default_rng(seed)
    ids = np.arange(1, T + 1) * 3
    feats = banks(rng, T, K, D, kind)
    s_attrs = spans(rng, T)
    q_ids = np.arange(1, Q + 1) * 3 + 1000
    q_ids[0] = ids[T // 2]   # one query carries a stored id: the self pair stays out whatever the rule says
    q_feats = banks(rng, Q, K, D, kind)
    q_attrs = spans(rng, Q)
    return ids, feats, s_attrs, q_ids, q_feats, q_attrs


def quantile(cells, q):
    v = cells[~np.isnan(cells)]
    return float(np.quantile(v, q))


def as_dict(raw, ids):
    out_n, win, wt = raw[:3]
    assert np.all(win[np.arange(win.shape[1])[None, :] >= out_n[:, None]] == 0)
    return {int(q): [(int(win[i, r]), float(wt[i, r])) for r in range(int(out_n[i]))] for i, q in enumerate(ids) if out_n[i]}


def same_result(a, b):
    """out_n, winners and the f64 bits of the weights"""
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))


def same_cells(a, b):
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    m = ~np.isnan(a)
    assert np.array_equal(a[m].view(np.uint32), b[m].view(np.uint32))


def equals_model(raw, q_ids, want):
    assert as_dict(raw, q_ids) == want
    for i, q in enumerate(q_ids):   # f64 bits, not float equality
        lst = want.get(int(q), [])
        assert raw[0][i] == len(lst)
        assert np.array_equal(raw[2][i][: len(lst)].view(np.uint64), np.array([w for _, w in lst], np.float64).view(np.uint64))


RULES = [X.SAME_KEY, X.DISJOINT, X.SAME_KEY | X.DISJOINT, X.QUERY_FIRST, X.ONLY_READY]


def restatement(engine, kind, T, K, Q, D, seed, about_half=False):
    ids, feats, s_attrs, q_ids, q_feats, q_attrs = case(kind, T, K, Q, D, seed)
    median_end = int(np.median([a[2] for a in s_attrs]))
    store = build(engine, kind, D, K, ids, feats, s_attrs)
    try:
        order = store.order()
        assert list(order) == list(ids)
        plain = store.search_raw(q_ids, q_feats, 5, INF, tap=True)
        md = quantile(plain[3], 0.5)
        for flags in RULES:
            rule = rule_of(flags, median_end if flags & X.ONLY_READY else X.INT64_MAX)
            lv = X.live_matrix(rule, q_attrs, s_attrs)
            assert (0.3 < lv.mean() < 0.7) if about_half else (0.0 < lv.mean() < 1.0), (flags, lv.mean())
            for topn, mv in ((5, min(2, K)), (64, 1)):
                raw = store.search_raw(q_ids, q_feats, topn, md, mv, tap=True, compat=rule, q_attrs=packed(q_attrs))
                same_cells(raw[3], plain[3])   # the tap keeps the cells of dead pairs
                want, M = X.restate(q_ids, order, raw[3], rule, q_attrs, s_attrs, topn, md, mv)
                assert want
                equals_model(raw, q_ids, want)
                for q, lst in want.items():
                    qi = list(q_ids).index(q)
                    assert all(lv[qi, list(order).index(w)] for w, _ in lst)
                same_result(raw, store.search_raw(q_ids, q_feats, topn, md, mv, compat=rule, q_attrs=packed(q_attrs)))
            dead = ~lv
            assert np.isfinite(raw[3][np.broadcast_to(dead[:, None, :, None], raw[3].shape)]).any()
    finally:
        store.close()


@pytest.mark.parametrize("kind", KINDS)
def test_flags_0_is_the_plain_call(engine, kind):
    """Item 1."""
    K, D, T, Q = 5, 64, 37, 21
    ids, feats, s_attrs, q_ids, q_feats, q_attrs = case(kind, T, K, Q, D, 11)
    store = build(engine, kind, D, K, ids, feats, s_attrs)
    other = build(engine, kind, D, K, ids, feats, s_attrs)
    try:
        none = A.compat()
        md = quantile(store.search_raw(q_ids, q_feats, 5, INF, tap=True)[3], 0.4)
        some = ids[[0, 5, 17, 36]]
        for tap in (False, True):
            pairs_ = [
                (store.search_raw(q_ids, q_feats, 5, md, 2, tap=tap), store.search_raw(q_ids, q_feats, 5, md, 2, tap=tap, compat=none, q_attrs=packed(q_attrs))),
                (store.search_stored_raw(some, 5, md, 2, withdraw=True, tap=tap), store.search_stored_raw(some, 5, md, 2, withdraw=True, tap=tap, compat=none)),
                (store.join_raw(5, md, 2, tap=tap), store.join_raw(5, md, 2, tap=tap, compat=none)),
            ]
            for a, b in pairs_:
                assert a[0].any()
                same_result(a, b)
                if tap:
                    same_cells(a[3], b[3])
            # the join was the last one.  No rule kills a group, but a ragged diagonal tile may own none at all (no q < t in range:
            # euclidean here, the last track's row tile): it leaves early like any tile without a live group, as the model counts
            tiles, dead = X.dead_tiles(kind, kp_of(K), X.NO_RULE, s_attrs, s_attrs, join=True)
            assert store.compat_stats() == {"tiles": tiles, "tiles_skipped": 0 if tap else dead}
            assert tiles == store.join_stats()["tiles"] and dead == (kind == "euclidean")
        plan = {int(ids[2]): [int(ids[9]), int(ids[20])], int(ids[30]): [int(ids[1])]}
        store.merge(plan, keep="latest", capacity=4, compat=none)
        other.merge(plan, keep="latest", capacity=4)
        assert np.array_equal(store.order(), other.order())
        for x, y in zip(store.fetch_raw(store.order()), other.fetch_raw(other.order())):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        at = dict(zip(ids.tolist(), s_attrs))
        got = store.get_attrs(store.order())
        for d, srcs in plan.items():
            assert got[d] == (at[d][0], min(at[i][1] for i in [d] + srcs), max(at[i][2] for i in [d] + srcs))
            assert other.get_attrs([d])[d] == at[d]   # plain merge: the destination's attributes stay
        same_result(store.join_raw(5, md), other.join_raw(5, md))
    finally:
        store.close()
        other.close()


@pytest.mark.parametrize("kind", KINDS)
def test_restatement(engine, kind):
    """Item 2: T = 37 x K = 5 against Q = 21, ragged last tiles in both kinds."""
    restatement(engine, kind, 37, 5, 21, 64, 21, about_half=True)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K,T,Q,D", [(1, 130, 70, 32), (32, 6, 4, 64)])
def test_group_geometry(engine, kind, K, T, Q, D):
    """Item 4: one slot per group (4096 groups in a cosine tile) and 32 x 32 slots per group (four groups in a tile)."""
    restatement(engine, kind, T, K, Q, D, 40 + K)


def dark_case(kind, seed=31):
    """Item 3's arrangement: the first 16 stored tracks carry a key no query has, the last 8 are not ready."""
    K, D, T, Q = 5, 64, 37, 21
    ids, feats, s_attrs, q_ids, q_feats, q_attrs = case(kind, T, K, Q, D, seed)
    ready = 1000
    s_attrs = [(99, s, e) if i < 16 else (k, s, ready + 1 + i) if i >= T - 8 else (k, s, e) for i, (k, s, e) in enumerate(s_attrs)]
    return K, D, ids, feats, s_attrs, q_ids, q_feats, q_attrs, rule_of(X.SAME_KEY | X.ONLY_READY, ready)


@pytest.mark.parametrize("kind", KINDS)
def test_skip_equals_no_skip(engine, kind):
    """Item 3."""
    K, D, ids, feats, s_attrs, q_ids, q_feats, q_attrs, rule = dark_case(kind)
    kp = kp_of(K)
    store = build(engine, kind, D, K, ids, feats, s_attrs)
    try:
        qa = packed(q_attrs)
        some = ids[[1, 8, 20, 22, 30, 36]]
        md = quantile(store.search_raw(q_ids, q_feats, 5, INF, tap=True)[3], 0.5)
        forms = [
            (lambda tap: store.search_raw(q_ids, q_feats, 7, md, 2, tap=tap, compat=rule, q_attrs=qa), X.dead_tiles(kind, kp, rule, q_attrs, s_attrs)),
            (lambda tap: store.search_stored_raw(some, 7, md, 2, tap=tap, compat=rule),
             X.dead_tiles(kind, kp, rule, X.attrs_of(ids, s_attrs, some), s_attrs)),
            (lambda tap: store.join_raw(7, md, 2, tap=tap, compat=rule), X.dead_tiles(kind, kp, rule, s_attrs, s_attrs, join=True)),
        ]
        for call, (tiles, dead) in forms:
            fast = call(False)
            st = store.compat_stats()
            assert st == {"tiles": tiles, "tiles_skipped": dead} and 0 < dead < tiles
            slow = call(True)
            assert store.compat_stats() == {"tiles": tiles, "tiles_skipped": 0}
            assert fast[0].any()
            same_result(fast, slow)
        # the tap call is the model (so the skipping call is too)
        raw = store.search_raw(q_ids, q_feats, 7, md, 2, tap=True, compat=rule, q_attrs=qa)
        equals_model(raw, q_ids, X.restate(q_ids, ids, raw[3], rule, q_attrs, s_attrs, 7, md, 2)[0])
        j = store.join_raw(7, md, 2, tap=True, compat=rule)
        equals_model(j, ids, X.join(ids, j[3], rule, s_attrs, 7, md, 2)[0])
        # a plain call afterwards is untouched by any of it
        same_result(store.join_raw(7, md, 2), store.join_raw(7, md, 2, compat=A.compat()))
    finally:
        store.close()


@pytest.mark.parametrize("kind", KINDS)
def test_the_largest_distance_sits_in_a_dead_pair(engine, kind):
    """Item 5: M follows the model, and every weight with it — a gate that only hid winners would return the plain weights."""
    K, D, T, Q = 3, 64, 20, 6
    ids, feats, s_attrs, q_ids, q_feats, q_attrs = case(kind, T, K, Q, D, 51)
    s_attrs = [(1, s, e) for _, s, e in s_attrs]
    q_attrs = [(1, s, e) for _, s, e in q_attrs]
    q_ids[0] = 1000   # no self pair here: the maximum over the tap's other columns is M
    far = 7
    s_attrs[far] = (2,) + s_attrs[far][1:]
    if kind == "euclidean":
        feats[far] = feats[far] + 40.0
    else:   # the engine's cosine figure grows with similarity: a bank parallel to a query row holds the call's largest one
        feats[far] = np.tile(2.0 * q_feats[2][0], (K, 1)).astype(np.float32)
    store = build(engine, kind, D, K, ids, feats, s_attrs)
    try:
        rule = rule_of(X.SAME_KEY)
        plain = store.search_raw(q_ids, q_feats, 64, INF, tap=True)
        cells = plain[3]
        top = np.nanmax(cells)
        rest = np.nanmax(np.delete(cells, far, axis=2))
        assert np.nanmax(cells[:, :, far, :]) == top and rest < top
        for tap in (True, False):
            raw = store.search_raw(q_ids, q_feats, 64, INF, tap=tap, compat=rule, q_attrs=packed(q_attrs))
            want, M = X.restate(q_ids, ids, cells, rule, q_attrs, s_attrs, 64, INF)
            assert M == rest
            equals_model(raw, q_ids, want)
        got, was = as_dict(raw, q_ids), as_dict(plain, q_ids)
        for q in got:
            old = dict(was[q])
            assert int(ids[far]) in old and int(ids[far]) not in dict(got[q])
            assert all(w != old[i] for i, w in got[q])   # the same groups otherwise, every weight another one
    finally:
        store.close()


def one_way_pairs(res, s_ids):
    return [(q, w) for q, lst in res.items() for w, _ in lst if q not in [x for x, _ in res.get(w, [])]]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flags", [X.SAME_KEY | X.DISJOINT, X.QUERY_FIRST, X.ONLY_READY])
def test_join(engine, kind, flags):
    """Item 6."""
    K, D, T = 5, 64, 37
    ids, feats, s_attrs, _, _, _ = case(kind, T, K, 1, D, 61)
    rule = rule_of(flags, int(np.median([a[2] for a in s_attrs])) if flags & X.ONLY_READY else X.INT64_MAX)
    store = build(engine, kind, D, K, ids, feats, s_attrs)
    try:
        order = store.order()
        md = quantile(store.join_raw(5, INF, tap=True)[3], 0.5)
        n_obs, fetched, _ = store.fetch_raw(order)
        host = [fetched[i, : n_obs[i]] for i in range(T)]
        for topn, mv in ((5, 2), (64, 1)):
            j = store.join_raw(topn, md, mv, tap=True, compat=rule)
            blocks = store.join_stats()["blocks"]
            assert store.last_stats()["groups"] == blocks
            s = store.search_stored_raw(order, topn, md, mv, tap=True, compat=rule)
            f = store.search_raw(order, host, topn, md, mv, tap=True, compat=rule, q_attrs=packed(s_attrs))
            for other in (s, f, store.join_raw(topn, md, mv, compat=rule)):
                same_result(j, other)
            same_cells(j[3], s[3])
            same_cells(j[3], f[3])
            want, _ = X.join(order, j[3], rule, s_attrs, topn, md, mv)
            equals_model(j, order, want)
            assert blocks == len(X.surviving_pairs(order, j[3], rule, s_attrs, md, mv)) > 0
        full = as_dict(j, order)   # topn 64: every surviving direction is listed
        if flags & (X.QUERY_FIRST | X.ONLY_READY):
            assert one_way_pairs(full, order)    # live in exactly one direction: in one track's winners and not in the other's
        else:
            assert not one_way_pairs(full, order)
        who = ids[[3, 12, 13, 30]].tolist() + [5555]
        raw = store.search_stored_raw(who, 9, md, 1, withdraw=True, tap=True, compat=rule)
        want, _ = X.search_stored(order, raw[3], who, rule, s_attrs, 9, md, 1, withdraw=True)
        equals_model(raw, who, want)
        assert not {w for lst in want.values() for w, _ in lst} & set(who)
        same_result(raw, store.search_stored_raw(who, 9, md, 1, withdraw=True, compat=rule))
    finally:
        store.close()


@pytest.mark.parametrize("kind", KINDS)
def test_pool_rerun(engine, kind):
    """Item 7: a fresh store whose first search is a compat join of 60 tracks in two keys: 870 surviving pairs against a first pool of
    256 blocks.  The rerun skips the same tiles."""
    rng = np.random.default_rng(71)
    K, D, T = 4, 64, 60
    ids, feats = np.arange(1, T + 1), banks(rng, T, K, D, kind, ragged=False)
    s_attrs = [(1 + (i >= 30), 0, 10) for i in range(T)]
    rule = rule_of(X.SAME_KEY)
    store = build(engine, kind, D, K, ids, feats, s_attrs)
    try:
        first = store.join_raw(10, INF, compat=rule)
        st = store.last_stats()
        assert st["reruns"] == 1 and st["groups"] == 2 * (30 * 29 // 2) > 256 and store.join_stats()["blocks"] == st["groups"]
        tiles, dead = X.dead_tiles(kind, K, rule, s_attrs, s_attrs, join=True)
        assert store.compat_stats() == {"tiles": tiles, "tiles_skipped": dead} and dead > 0
        again = store.join_raw(10, INF, tap=True, compat=rule)
        assert store.last_stats()["reruns"] == 0
        same_result(first, again)
        equals_model(again, ids, X.join(ids, again[3], rule, s_attrs, 10, INF)[0])
    finally:
        store.close()


@pytest.mark.parametrize("kind", KINDS)
def test_attributes_travel(engine, kind):
    """Item 8."""
    K, D, T, Q = 5, 64, 37, 21
    ids, feats, s_attrs, q_ids, q_feats, q_attrs = case(kind, T, K, Q, D, 81)
    rule = rule_of(X.SAME_KEY | X.DISJOINT)
    model = X.Model(K, D)
    model.upsert(ids, feats)
    model.set_attrs(ids, s_attrs)
    store = build(engine, kind, D, K, ids, feats, s_attrs)
    fresh = None
    try:
        rng = np.random.default_rng(82)

        def check():
            nonlocal fresh
            order = [int(i) for i in store.order()]
            assert order == model.order
            assert store.get_attrs(order) == {i: model.attrs[i] for i in order}
            fresh = build(engine, kind, D, K, order, [model.feats(i) for i in order], model.attrs_in_order())
            try:
                qa = packed(q_attrs)
                same_result(store.search_raw(q_ids, q_feats, 5, INF, 2, compat=rule, q_attrs=qa),
                            fresh.search_raw(q_ids, q_feats, 5, INF, 2, compat=rule, q_attrs=qa))
                same_result(store.join_raw(5, INF, 2, compat=rule), fresh.join_raw(5, INF, 2, compat=rule))
            finally:
                fresh.close()

        check()
        gone = ids[[4, 17, 18]].tolist() + [9999]
        store.remove(gone)
        model.remove(gone)
        check()
        plan = {int(ids[2]): [int(ids[9]), int(ids[20])], int(ids[30]): [int(ids[1])]}
        store.merge(plan)
        model.merge(plan)
        check()
        rep = [int(ids[3]), int(ids[36]), 7777]
        new = banks(rng, 3, K, D, kind)
        store.upsert(rep, new)
        model.upsert(rep, new)
        assert store.get_attrs([7777]) == {7777: (0, 0, 0)} and store.get_attrs([int(ids[3])])[int(ids[3])] == s_attrs[3]
        check()
        store.append([8888, int(ids[5])], [new[0][:1], new[1][:1]])
        model.append([8888, int(ids[5])], [new[0][:1], new[1][:1]])
        assert store.get_attrs([8888, 4242]) == {8888: (0, 0, 0)}
        out, known = store.get_attrs_raw([8888, 4242])
        assert list(known) == [True, False] and out[1].tolist() == (0, 0, 0)
        check()
    finally:
        store.close()


@pytest.mark.parametrize("kind", KINDS)
def test_merge(engine, kind):
    """Item 9."""
    rng = np.random.default_rng(91)
    K, D, T = 4, 64, 12
    ids = np.arange(1, T + 1)
    feats = banks(rng, T, K, D, kind)
    s_attrs = [(1 + (i >= 8), 10 * i, 10 * i + 10) for i in range(T)]   # back to back: disjoint, two keys
    s_attrs[5] = (1, 15, 18)                                              # inside track 2's span (10..20)
    rule = rule_of(X.SAME_KEY | X.DISJOINT)
    model = X.Model(K, D)
    model.upsert(ids, feats)
    model.set_attrs(ids, s_attrs)
    store = build(engine, kind, D, K, ids, feats, s_attrs)
    try:
        def state():
            order = store.order()
            return order, store.fetch_raw(order), store.get_attrs(order)

        def unchanged(before):
            after = state()
            assert np.array_equal(before[0], after[0]) and before[2] == after[2]
            for x, y in zip(before[1], after[1]):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32))

        before = state()
        refused = [
            {2: [6]},          # 15..18 overlaps 10..20
            {1: [10]},         # another key
            {1: [3, 2]},       # 2 (10..20) fits the original 1 (0..10) but not 1 after it absorbed 3 (20..30): 0..30
            {4: [5], 2: [6]},  # the second destination refuses: the first one's merge must not have happened
        ]
        for plan in refused:
            with pytest.raises(X.Incompatible):
                model.copy().merge(plan, rule=rule)
            with pytest.raises(EngineError) as ei:
                store.merge(plan, compat=rule)
            assert ei.value.code == abi.SA_ERR_BAD_ARG and "not compatible" in str(ei.value)
            unchanged(before)
        assert X.live(rule.flags, rule.ready_at, s_attrs[0], s_attrs[1])   # the third plan's claim about the original destination
        plan = {1: [2, 3], 9: [10]}
        store.merge(plan, keep="latest", capacity=3, compat=rule)
        model.merge(plan, keep=merge_ref.LATEST, capacity=3, rule=rule)
        order = [int(i) for i in store.order()]
        assert order == model.order
        got = store.get_attrs(order)
        assert got == {i: model.attrs[i] for i in order} and got[1] == (1, 0, 30) and got[9] == (2, 80, 100)
        fetched = store.fetch(order)
        for i in order:
            assert np.array_equal(fetched[i][0].view(np.uint32), model.feats(i).view(np.uint32))
        fresh = build(engine, kind, D, K, order, [model.feats(i) for i in order], model.attrs_in_order())
        try:
            a, b = store.join_raw(5, INF, compat=rule), fresh.join_raw(5, INF, compat=rule)
            assert a[0].any()
            same_result(a, b)
        finally:
            fresh.close()
    finally:
        store.close()


def test_refusals(engine):
    """Item 10: every refusal of the header, the store unchanged afterwards."""
    K, D, T, Q = 3, 64, 9, 4
    ids, feats, s_attrs, q_ids, q_feats, q_attrs = case("euclidean", T, K, Q, D, 101)
    store = build(engine, "euclidean", D, K, ids, feats, s_attrs)
    try:
        lib, h = store.lib, store.h
        ok = A.compat(same_key=True)
        qa = packed(q_attrs)
        prm = A.sa_topn_params(5, 1, 1.0, INF)
        out_n, win, wt = np.zeros(T, np.uint32), np.zeros((T, 5), np.uint64), np.zeros((T, 5), np.float64)
        outs = (out_n.ctypes.data_as(C.POINTER(C.c_uint32)), win.ctypes.data_as(C.POINTER(C.c_uint64)), wt.ctypes.data_as(C.POINTER(C.c_double)), None)
        idp = np.ascontiguousarray(ids, np.uint64)
        idp_c = idp.ctypes.data_as(C.POINTER(C.c_uint64))

        def state():
            return store.order(), store.get_attrs_raw(store.order())[0].tolist(), store.join_raw(5, INF, compat=ok), store.fetch_raw(store.order())

        def struct(size=16, flags=1, ready=0):
            return A.sa_compat(size, flags, ready)

        bad_rules = [struct(size=8), struct(size=24), struct(flags=16), struct(flags=0x80000001), struct(flags=X.DISJOINT | X.QUERY_FIRST),
                     struct(flags=X.SAME_KEY | X.DISJOINT | X.QUERY_FIRST)]
        backwards = qa.copy()
        backwards["start"][1], backwards["end"][1] = 9, 8
        calls = []
        for r in bad_rules:
            calls += [lambda r=r: store.search_raw(q_ids, q_feats, 5, 1.0, compat=r, q_attrs=qa),
                      lambda r=r: store.search_stored_raw(ids[:3], 5, 1.0, compat=r),
                      lambda r=r: store.join_raw(5, 1.0, compat=r),
                      lambda r=r: store.merge({int(ids[0]): [int(ids[1])]}, compat=r)]
        calls += [
            lambda: store.merge({int(ids[0]): [int(ids[1])]}, compat=A.compat(ready_at=5)),          # ONLY_READY is no rule of a merge
            lambda: store.merge_raw(None, "latest", ids[:1], [1], ids[1:2]),                            # null sa_compat
            lambda: store._chk(lib.sa_store_join_topn_compat(h, C.byref(prm), None, *outs)),
            lambda: store._chk(lib.sa_store_search_stored_compat(h, C.byref(prm), None, 0, 2, idp_c, *outs)),
            lambda: store._chk(lib.sa_store_search_topn_compat(h, C.byref(prm), None, 0, None, None, None, None, *outs)),
            lambda: store.search_raw(q_ids, q_feats, 5, 1.0, compat=ok, q_attrs=None),                 # null q_attrs
            lambda: store.search_raw(q_ids, q_feats, 5, 1.0, compat=ok, q_attrs=backwards),            # start > end
            lambda: store.set_attrs([int(ids[0])], [1], [9], [8]),
            lambda: store.set_attrs([int(ids[0]), 0], [1, 1], [0, 0], [1, 1]),
            lambda: store.set_attrs([int(ids[0]), int(ids[0])], [1, 1], [0, 0], [1, 1]),
            lambda: store.set_attrs([int(ids[0]), 4242], [1, 1], [0, 0], [1, 1]),                      # an unknown id: nothing is set
            lambda: store._chk(lib.sa_store_set_attrs(h, 1, idp_c, None)),
            lambda: store._chk(lib.sa_store_get_attrs(h, 1, idp_c, None, None)),
            # what the plain calls refuse, refused the same way
            lambda: store.search_raw(q_ids, q_feats, 5, float("nan"), compat=ok, q_attrs=qa),
            lambda: store.search_raw([7, 7], q_feats[:2], 5, 1.0, compat=ok, q_attrs=qa[:2]),
            lambda: store.search_stored_raw([int(ids[0]), 0], 5, 1.0, compat=ok),
            lambda: store.search_stored_raw(ids[:2], 5, 1.0, flags=2, compat=ok),
            lambda: store.join_raw(0, 1.0, compat=ok),
            lambda: store.merge({int(ids[0]): [4242]}, compat=ok),
            lambda: store.merge({int(ids[0]): [int(ids[0])]}, compat=ok),
            lambda: store.merge({int(ids[0]): [int(ids[1])]}, keep=7, compat=A.compat()),
            lambda: store.merge({int(ids[0]): [int(ids[1])]}, capacity=K + 1, compat=A.compat()),
        ]
        before = state()
        for n, call in enumerate(calls):
            with pytest.raises(EngineError) as ei:
                call()
            assert ei.value.code == abi.SA_ERR_BAD_ARG, n
            after = state()
            assert np.array_equal(before[0], after[0]) and before[1] == after[1], n
            same_result(before[2], after[2])
            for x, y in zip(before[3], after[3]):
                assert np.array_equal(x, y), n
        with pytest.raises(EngineError) as ei:
            store.join_raw(65, 1.0, compat=ok)
        assert ei.value.code == abi.SA_ERR_UNSUPPORTED
        # which check speaks: the rule before the params (a merge: before keep and capacity), the params before everything the call
        # lists, and of several bad elements the first, whatever its fault
        nan, small, two = float("nan"), struct(size=8), [int(ids[0]), int(ids[1])]
        for text, call in [
            ("sa_compat.struct_size 8", lambda: store.search_raw([7, 7], q_feats[:2], 5, nan, compat=small, q_attrs=qa[:2])),
            ("sa_compat.struct_size 8", lambda: store.search_stored_raw(ids[:2], 5, nan, flags=2, compat=small)),
            ("sa_compat.struct_size 8", lambda: store.join_raw(0, 1.0, compat=small)),
            ("sa_compat.struct_size 8", lambda: store.merge({int(ids[0]): [int(ids[1])]}, keep=7, compat=small)),
            ("null sa_compat", lambda: store._chk(lib.sa_store_join_topn_compat(h, None, None, *outs))),
            ("null sa_compat", lambda: store._chk(lib.sa_store_search_stored_compat(h, None, None, 2, 2, idp_c, *outs))),
            ("null sa_compat", lambda: store._chk(lib.sa_store_search_topn_compat(h, None, None, 1, None, None, None, None, *outs))),
            ("null params", lambda: store._chk(lib.sa_store_join_topn_compat(h, None, C.byref(struct()), *outs))),
            ("must not be NaN", lambda: store.search_raw([7, 7], q_feats[:2], 5, nan, compat=ok, q_attrs=None)),
            ("null argument", lambda: store.search_raw([7, 7], q_feats[:2], 5, 1.0, compat=ok, q_attrs=None)),
            ("id 7 twice", lambda: store.search_raw([7, 7], q_feats[:2], 5, 1.0, compat=ok, q_attrs=backwards[:2])),
            ("query 8 starts after it ends", lambda: store.search_raw([7, 8], q_feats[:2], 5, 1.0, compat=ok, q_attrs=backwards[:2])),
            ("must not be NaN", lambda: store.search_stored_raw(ids[:2], 5, nan, flags=2, compat=ok)),
            ("unknown flag bits 0x2", lambda: store.search_stored_raw([], 5, 1.0, flags=2, compat=ok)),
            ("unknown keep 7", lambda: store.merge({0: [int(ids[1])]}, keep=7, compat=A.compat())),
            ("unknown id 4242", lambda: store.set_attrs([4242, 0], [1, 1], [0, 0], [1, 1])),
            ("id 0 at 1", lambda: store.set_attrs([two[0], 0, 4242], [1, 1, 1], [0, 0, 0], [1, 1, 1])),
            ("id %d starts after it ends" % two[0], lambda: store.set_attrs(two + [0], [1, 1, 1], [9, 0, 0], [8, 1, 1])),
            ("id %d twice" % two[0], lambda: store.set_attrs([two[0], two[0]], [1, 1], [0, 9], [1, 8])),
            ("id %d starts after it ends" % two[1], lambda: store.set_attrs(two + [4242], [1, 1, 1], [0, 9, 0], [1, 8, 1])),
        ]:
            with pytest.raises(EngineError, match=text):
                call()
        after = state()
        assert np.array_equal(before[0], after[0]) and before[1] == after[1]
        # the int64 extremes are times like any other
        store.set_attrs(ids[:2], [1, 1], [X.INT64_MIN, X.INT64_MAX], [X.INT64_MIN, X.INT64_MAX])
        assert store.get_attrs(ids[:2]) == {int(ids[0]): (1, X.INT64_MIN, X.INT64_MIN), int(ids[1]): (1, X.INT64_MAX, X.INT64_MAX)}
        rule = rule_of(X.QUERY_FIRST)
        j = store.join_raw(64, INF, tap=True, compat=rule)
        now = [store.get_attrs([int(i)])[int(i)] for i in store.order()]
        equals_model(j, store.order(), X.join(store.order(), j[3], rule, now, 64, INF)[0])
        got = as_dict(j, store.order())
        assert int(ids[1]) in dict(got[int(ids[0])]) and int(ids[1]) not in got
    finally:
        store.close()
