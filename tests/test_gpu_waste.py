"""Tracks that leave an engine's table enter a feature store on the MI355X (similari_amd.waste over include/similari_waste.h).

The contract admits no tolerance: sa_tracks_waste returns, and leaves in the store and in the engine, exactly the bits of
sa_tracks_get_state per id, the compaction of the present slots, sa_store_append and sa_tracks_remove_many.  So every case runs one
visual engine E with two stores of the same options — store A takes the one call, store B the host sequence (tests/waste_ref.py) fed
from the state read BEFORE the call — and a twin engine E2 with the same tables that takes the plain removal.  Compared: out_n_obs,
and of both stores order(), fetch_raw rows, counts and qualities as uint32, the attributes and a tapped search bit for bit
(tests/test_gpu_absorb.py's same_stores); of both engines sa_tracks_order and sa_tracks_get_state of every remaining track.
sa_tracks_waste_absorb is held the same way against get_state + sa_store_absorb_keep + remove.

Shapes are the smallest at which the capture can go wrong: bank depths 1, 3, 5, 16 into stores of the same depth and of 32 (Kp differs
from K), rows of 1, 31, 33, 257 and 1024 elements (padding on both sides, a second pass of a lane), every presence pattern a bank can
have, 1 to 65 leaving tracks (a second wave and workgroup), 14 scenes (a second launch).  Engines are made once per (K, D); every
case works on scenes of its own."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import absorb_cases as AC
import absorb_ref as AR
import test_gpu_absorb as TA
import waste_ref as WR
from similari_amd import abi, attrs as AT, waste as W
from similari_amd.engine import Engine, EngineError
from similari_amd.f16 import SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_F32
from similari_amd.i8 import SA_ELEM_I8, I8Store
from similari_amd.retain import RetainStore

pytestmark = pytest.mark.gpu
u8, u32, u64, f32 = np.uint8, np.uint32, np.uint64, np.float32
F32, BF16, F16, I8 = SA_ELEM_F32, SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_I8
NAME = {F32: "f32", BF16: "bf16", F16: "f16", I8: "i8"}
CUT = TA.CUT
ZERO = {"tracks": 0, "launches_capture": 0, "reserved": 0, "rows": 0, "feature_bytes_h2d": 0, "feature_bytes_d2h": 0, "table_bytes_d2h": 0,
        "capture_ms": 0.0}


# ---- engines and stores --------------------------------------------------------------------------
class Twins:
    """(E, E2) per (K, D), made on first use; fresh scene numbers for every case."""

    def __init__(self):
        self.made, self.scene = {}, itertools.count(1)

    def get(self, K, D):
        if (K, D) not in self.made:
            self.made[(K, D)] = tuple(Engine(abi.make_config(device=0, visual="cosine", feature_len=D, max_observations=K)) for _ in range(2))
        return self.made[(K, D)]

    def scenes(self, n):
        return [next(self.scene) for _ in range(n)]

    def close(self):
        for pair in self.made.values():
            for e in pair:
                e.close()


@pytest.fixture(scope="module")
def twins():
    t = Twins()
    yield t
    t.close()


def make(engine, elem, kind, D, K):
    return I8Store(engine, "cosine", D, K) if elem == I8 else RetainStore(engine, kind, D, K, elem)


class Stores:
    """Store A for the one call, store B for the host sequence, both on E."""

    def __init__(self, engine, elem, kind, D, K):
        self.all = []
        for _ in range(2):
            self.all.append(make(engine, elem, kind, D, K))
        self.a, self.b = self.all

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for s in self.all:
            s.close()


def same(rng, a, b, rule=None):
    if len(a) or len(b):
        TA.same_stores(rng, a, b, rule)
    else:
        assert TA.state(a) == TA.state(b)


def fill_both(tw, K, D, scene, ids, present, feats, quality, seed):
    for e in tw:
        WR.fill(e, scene, ids, present, feats, quality, np.random.default_rng(seed))


def both_routes(rng, tw, st, K, D, leaving, keep="latest", capacity=None):
    """One waste through both routes, everything compared; -> (n_obs, waste stats of store A)."""
    E, E2 = tw
    scenes = sorted({s for s, _ in WR.items(leaving)})
    ids, rows, quality = WR.leaving_rows(E, leaving, K, D)
    flat, n_obs = W.waste_raw(E, st.a, leaving, keep, capacity)
    ws, ma = W.last(st.a), st.a.merge_stats()
    if len(ids):
        st.b.append(ids, rows, quality, keep, capacity)
    WR.remove_many(E2, leaving)
    assert flat.tobytes() == ids.tobytes() and n_obs.dtype == u32 and [int(m) for m in n_obs] == [len(r) for r in rows]
    same(rng, st.a, st.b)
    assert WR.snapshot(E, scenes, K, D) == WR.snapshot(E2, scenes, K, D)
    if len(ids):
        mb = st.b.merge_stats()
        assert all(ma[k] == mb[k] for k in ("launches", "rows_rewritten", "tracks_moved")), (ma, mb)
    with_ids = sum(1 for _, x in WR.items(leaving) if len(x))
    assert ws["struct_size"] == C.sizeof(W.sa_waste_stats) == 56
    assert ws["feature_bytes_h2d"] == 0 and ws["feature_bytes_d2h"] == 0
    assert ws["tracks"] == len(ids) and ws["rows"] == sum(len(r) for r in rows)
    assert ws["launches_capture"] == math.ceil(with_ids / 12)
    assert ws["table_bytes_d2h"] == len(ids) * 4 * (1 + (1 << (st.a.K - 1).bit_length()))   # a count and Kp qualities per track
    return n_obs, ws


# ---- 1. every bank depth, store depth and row length; every presence pattern --------------------
@pytest.mark.parametrize("D", [1, 31, 33, 257, 1024])
@pytest.mark.parametrize("K,deep", [(K, deep) for K in (1, 3, 5, 16) for deep in (False, True)], ids=lambda v: str(v))
def test_every_depth_and_row_length(twins, K, deep, D):
    rng = np.random.default_rng(1000 * K + D + (7 if deep else 0))
    tw, (scene,) = twins.get(K, D), twins.scenes(1)
    pats = WR.patterns(K)
    n = len(pats) + 4
    ids, present, feats, quality = WR.table(rng, n, K, D, first_id=10)
    fill_both(tw, K, D, scene, ids, present, feats, quality, 5)
    with Stores(tw[0], F32, "cosine", D, 32 if deep else K) as st:
        leave = list(ids[: len(pats)]) + [ids[-2]]   # every pattern and one random bank; three tracks stay, the last row among them
        n_obs, ws = both_routes(rng, tw, st, K, D, {scene: leave})
        assert [int(m) for m in n_obs[: len(pats)]] == [int(p.sum()) for p in pats.values()]
        got = st.a.fetch_raw(np.array(leave, u64))
        for i, (name, p) in enumerate(pats.items()):   # against the table as it was uploaded, no library call between
            m = int(p.sum())
            assert np.array_equal(got[1][i, :m].view(u32), feats[i][p != 0].view(u32)), name
            assert np.array_equal(got[2][i, :m].view(u32), quality[i][p != 0].view(u32)), name
        assert [int(t) for t in tw[0].order(scene)] == [int(t) for t in ids if t not in leave]


# ---- 2. all four element types, f16 with both metrics -------------------------------------------
FORMS = [(F32, "cosine"), (F32, "euclidean"), (F16, "cosine"), (F16, "euclidean"), (BF16, "cosine"), (I8, "cosine")]


@pytest.mark.parametrize("K,Ks,D", [(3, 5, 33), (5, 5, 257)], ids=lambda v: str(v))
@pytest.mark.parametrize("elem,kind", FORMS, ids=lambda v: NAME.get(v, v) if isinstance(v, int) else v)
def test_every_store_type_rounds_as_its_host_fed_call(twins, elem, kind, K, Ks, D):
    rng = np.random.default_rng(200 + elem * 10 + K)
    tw, (scene,) = twins.get(K, D), twins.scenes(1)
    ids, present, feats, quality = WR.table(rng, 12, K, D)
    feats[6] *= 1e-6   # small rows (f16 subnormals, an i8 scale of its own)
    feats[7] *= 300.0
    fill_both(tw, K, D, scene, ids, present, feats, quality, 6)
    with Stores(tw[0], elem, kind, D, Ks) as st:
        both_routes(rng, tw, st, K, D, {scene: ids[:10]})
        both_routes(rng, tw, st, K, D, {scene: ids[10:]})   # into the store the first call left


# ---- 3. the leaving sets -------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["one", "two", "65", "first and last", "every row"])
def test_leaving_sets(twins, which):
    K, D, T = 3, 33, 70
    rng = np.random.default_rng(300 + len(which))
    tw, (scene,) = twins.get(K, D), twins.scenes(1)
    ids, present, feats, quality = WR.table(rng, T, K, D, first_id=500)
    fill_both(tw, K, D, scene, ids, present, feats, quality, 7)
    leave = {"one": ids[33:34], "two": ids[[40, 12]], "65": ids[rng.permutation(T)[:65]], "first and last": ids[[0, T - 1]], "every row": ids}[which]
    with Stores(tw[0], F32, "cosine", D, K) as st:
        both_routes(rng, tw, st, K, D, {scene: leave})
        assert tw[0].count(scene) == T - len(leave)
        assert [int(t) for t in st.a.order()] == [int(t) for t in leave]   # created in call order


# ---- 4. more scenes than one launch takes --------------------------------------------------------
def test_fourteen_scenes_in_one_call(twins):
    K, D = 3, 33
    rng = np.random.default_rng(400)
    tw, scenes = twins.get(K, D), twins.scenes(15)
    leaving, first = [], 1
    for k, s in enumerate(scenes):
        ids, present, feats, quality = WR.table(rng, 5, K, D, first_id=first)
        first += 5
        fill_both(tw, K, D, s, ids, present, feats, quality, 8 + k)
        take = [] if k == 6 else list(ids) if k == 3 else list(ids[rng.permutation(5)[: 1 + k % 4]])   # a scene of no ids is skipped; one loses every row
        leaving.append((s, take))
    with Stores(tw[0], F32, "cosine", D, 4) as st:
        n_obs, ws = both_routes(rng, tw, st, K, D, leaving)
        assert ws["launches_capture"] == 2 and ws["tracks"] == sum(len(x) for _, x in leaving)
        assert tw[0].count(scenes[3]) == 0 and tw[0].count(scenes[6]) == 5


# ---- 5. a store that holds some of the ids already ----------------------------------------------
@pytest.mark.parametrize("elem", [F32, I8], ids=lambda v: NAME[v])
@pytest.mark.parametrize("keep", ["latest", "best"])
def test_known_ids_are_joined_under_the_rule(twins, keep, elem):
    K, Ks, D = 3, 5, 33
    rng = np.random.default_rng(500 + elem)
    tw, (scene,) = twins.get(K, D), twins.scenes(1)
    ids, present, feats, quality = WR.table(rng, 10, K, D, first_id=21)
    fill_both(tw, K, D, scene, ids, present, feats, quality, 9)
    with Stores(tw[0], elem, "cosine", D, Ks) as st:
        held = [int(ids[0]), int(ids[1]), int(ids[5]), 900, 901]   # 21: all present, 22: none; two tracks of the store's own
        banks = [rng.uniform(-1, 1, (m, D)).astype(f32) for m in (4, 2, 5, 3, 1)]
        qual = [rng.uniform(0.05, 1, len(b)).astype(f32) for b in banks]
        for s in st.all:
            s.append(held, banks, qual, "latest")
        n_obs, ws = both_routes(rng, tw, st, K, D, {scene: ids[:8]}, keep, 4)   # 4 + 3 observations into a capacity of 4: the rule cuts
        counts = dict(zip([int(t) for t in ids[:8]], st.a.fetch_raw(ids[:8])[0]))
        assert counts[21] == 4 and counts[22] == 2 and st.a.fetch_raw(np.array([900], u64))[0][0] == 3
        both_routes(rng, tw, st, K, D, {scene: ids[8:]}, keep, 1)


# ---- 6. refusals ---------------------------------------------------------------------------------
def test_refusals_leave_engine_and_store_as_they_were(twins):
    K, D = 3, 33
    rng = np.random.default_rng(600)
    tw, (s1, s2) = twins.get(K, D), twins.scenes(2)
    E, E2 = tw
    for s, first in ((s1, 1), (s2, 1)):   # the two scenes hold the same ids: an id twice across the call
        ids, present, feats, quality = WR.table(rng, 6, K, D, first_id=first)
        fill_both(tw, K, D, s, ids, present, feats, quality, 10)
    plain = Engine(abi.make_config(device=0))
    with Stores(E, F32, "cosine", D, K) as st, Stores(E2, F32, "cosine", D, K) as other, Stores(E, F32, "cosine", D + 1, K) as longer, \
            Stores(E, F32, "cosine", D, K - 1) as shallow, Stores(plain, F32, "cosine", D, K) as flat:
        st.a.append([6, 77], [rng.uniform(-1, 1, (2, D)).astype(f32)] * 2, None, "latest")
        before = (WR.snapshot(E, [s1, s2], K, D), TA.state(st.a))
        cases = [
            (abi.SA_ERR_BAD_ARG, "not visual", plain, flat.a, {s1: [1]}, {}),
            (abi.SA_ERR_BAD_ARG, "another engine", E, other.a, {s1: [1]}, {}),
            (abi.SA_ERR_BAD_ARG, "feature_len", E, longer.a, {s1: [1]}, {}),
            (abi.SA_ERR_BAD_ARG, "bank depth", E, shallow.a, {s1: [1]}, {}),
            (abi.SA_ERR_BAD_ARG, "id 0", E, st.a, {s1: [1, 0]}, {}),
            (abi.SA_ERR_BAD_ARG, "twice in one call", E, st.a, {s1: [1, 2], s2: [3, 1]}, {}),
            (abi.SA_ERR_BAD_ARG, "twice in one call", E, st.a, {s1: [2, 2]}, {}),
            (abi.SA_ERR_BAD_ARG, "unknown keep", E, st.a, {s1: [1]}, dict(keep=7)),
            (abi.SA_ERR_BAD_ARG, "capacity 0", E, st.a, {s1: [1, 2]}, dict(capacity=[1, 0])),
            (abi.SA_ERR_BAD_ARG, "capacity 4", E, st.a, {s1: [1]}, dict(capacity=K + 1)),
            (abi.SA_ERR_BAD_ARG, "appears twice", E, st.a, [(s1, [1]), (s2, [2]), (s1, [3])], {}),
            (abi.SA_ERR_NOT_FOUND, "unknown scene", E, st.a, {s1: [1], 999999: [2]}, {}),
            (abi.SA_ERR_NOT_FOUND, "unknown track id", E, st.a, {s1: [1, 55]}, {}),
        ]
        for code, text, eng, store, leaving, kw in cases:
            with pytest.raises(EngineError) as err:
                W.waste_raw(eng, store, leaving, **kw)
            assert err.value.code == code and text in str(err.value), (text, str(err.value))
            got = W.last(store)
            assert {k: got[k] for k in ZERO} == ZERO, text
            assert (WR.snapshot(E, [s1, s2], K, D), TA.state(st.a)) == before, text
        # null arguments, past the Python face
        lib = W._lib(st.a)
        one, ids1 = np.array([1], u32), np.array([1], u64)
        ptr = (C.POINTER(C.c_uint64) * 1)(ids1.ctypes.data_as(C.POINTER(C.c_uint64)))
        sid = np.array([s1], u64)
        u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        assert lib.sa_tracks_waste(E.h, None, 0, 1, sid.ctypes.data_as(u64p), one.ctypes.data_as(u32p), ptr, None, None) == abi.SA_ERR_BAD_ARG
        assert lib.sa_tracks_waste(None, st.a.h, 0, 1, sid.ctypes.data_as(u64p), one.ctypes.data_as(u32p), ptr, None, None) == abi.SA_ERR_BAD_ARG
        assert lib.sa_tracks_waste(E.h, st.a.h, 0, 1, None, one.ctypes.data_as(u32p), ptr, None, None) == abi.SA_ERR_BAD_ARG
        assert lib.sa_tracks_waste(E.h, st.a.h, 0, 1, sid.ctypes.data_as(u64p), None, ptr, None, None) == abi.SA_ERR_BAD_ARG
        assert lib.sa_tracks_waste(E.h, st.a.h, 0, 1, sid.ctypes.data_as(u64p), one.ctypes.data_as(u32p), None, None, None) == abi.SA_ERR_BAD_ARG
        null = (C.POINTER(C.c_uint64) * 1)()
        assert lib.sa_tracks_waste(E.h, st.a.h, 0, 1, sid.ctypes.data_as(u64p), one.ctypes.data_as(u32p), null, None, None) == abi.SA_ERR_BAD_ARG
        assert (WR.snapshot(E, [s1, s2], K, D), TA.state(st.a)) == before
        # the absorb's own: an id that the store holds, a rule without attributes, no rows asked for
        for text, leaving, kw in [("is a stored track's", {s1: [6]}, {}), ("come together", {s1: [1]}, dict(compat=AT.compat(same_key=True))),
                                  ("topn", {s1: [1]}, dict(topn=0))]:
            args = dict(topn=1, max_distance=CUT["cosine"])
            args.update(kw)
            with pytest.raises(EngineError) as err:
                W.waste_absorb_raw(E, st.a, leaving, **args)
            assert err.value.code == abi.SA_ERR_BAD_ARG and text in str(err.value), (text, str(err.value))
            assert (WR.snapshot(E, [s1, s2], K, D), TA.state(st.a)) == before, text
        # nothing to do is no refusal, and changes nothing
        assert W.waste(E, st.a, {}) == {} and W.waste(E, st.a, {s1: []}) == {}
        assert (WR.snapshot(E, [s1, s2], K, D), TA.state(st.a)) == before
        # and the call still works behind all of them
        both_routes(rng, tw, Pair(st.a, other_b(st, rng, D)), K, D, {s1: [1, 2], s2: [3]})
    plain.close()


class Pair:
    def __init__(self, a, b):
        self.a, self.b, self.all = a, b, [a, b]


def other_b(st, rng, D):
    """Store B of the refusal case, brought to what store A holds."""
    ids = st.a.order()
    n_obs, feats, qual = st.a.fetch_raw(ids)
    st.b.append(ids, [feats[i, : n_obs[i]] for i in range(len(ids))], [qual[i, : n_obs[i]] for i in range(len(ids))], "latest")
    return st.b


# ---- 7. waste_absorb: the leaving tracks are the queries of one absorb --------------------------
@pytest.mark.parametrize("elem", [F32, I8], ids=lambda v: NAME[v])
@pytest.mark.parametrize("keep", ["latest", "best"])
@pytest.mark.parametrize("ruled", [False, True], ids=["plain", "rule"])
def test_waste_absorb_is_get_state_absorb_keep_remove(twins, ruled, keep, elem):
    K, Ks, D, T, n = 3, 4, 33, 30, 40
    rng = np.random.default_rng(700)
    tw, (scene, scene2) = twins.get(K, D), twins.scenes(2)
    E, E2 = tw
    g_ids, g_banks = AC.banks(rng, T, Ks, D)
    # 40 leaving tracks: the first 20 near-duplicates of gallery tracks 1..20 (each named once: the negation of its first row plus a
    # little noise, a cosine store's nearest), the other 20 random rows, far from everything; one of those has no feature row at all
    ids, present, feats, quality = WR.table(rng, n + 3, K, D, first_id=1001)
    present[:20, 0] = 1   # a near-duplicate has at least one row
    present[25] = 0
    for i in range(20):
        feats[i] = -g_banks[i][0][None, :] + rng.normal(0, 1e-3, (K, D))
    feats = (feats * present[:, :, None]).astype(f32)
    # the premise, on the CPU (tests/absorb_ref.py): every near-duplicate is matched to its track, every other query is created, and no
    # winner is decided by a tie of weights
    model = AR.Model(Ks, D, "cosine")
    model.upsert(g_ids, g_banks)
    rows = [feats[i][present[i] != 0] for i in range(n)]
    res, dest = model.absorb(ids[:n], rows, 64, CUT["cosine"])
    assert [dest[int(t)] for t in ids[:n]] == [int(g_ids[i]) for i in range(20)] + [int(t) for t in ids[20:n]]
    for q, lst in res.items():
        assert len(lst) < 2 or lst[0][1] > lst[1][1], q
    assert len({lst[0][2] for lst in res.values()}) == len(res)   # no two queries name one stored track
    fill_both(tw, K, D, scene, ids[:24], present[:24], feats[:24], quality[:24], 11)
    fill_both(tw, K, D, scene2, ids[24:], present[24:], feats[24:], quality[24:], 12)
    leaving = [(scene2, ids[24:n]), (scene, ids[:24])]
    call = np.concatenate([ids[24:n], ids[:24]])
    rule = AT.compat(same_key=True) if ruled else None
    q_attrs = AT.pack_attrs([1 if t % 5 else 2 for t in call], [int(t) for t in call], [int(t) + 3 for t in call]) if ruled else None
    with Stores(E, elem, "cosine", D, Ks) as st:
        g_qual = [rng.uniform(0.05, 1, len(b)).astype(f32) for b in g_banks]
        for s in st.all:
            s.append(g_ids, g_banks, g_qual, "latest")
        for s in st.all:
            s.set_attrs(g_ids, [1] * T, list(range(T)), [t + 2 for t in range(T)])
        q_ids, q_rows, q_quality = WR.leaving_rows(E, leaving, K, D)
        assert q_ids.tobytes() == call.tobytes()
        flat, got = W.waste_absorb_raw(E, st.a, leaving, 2, CUT["cosine"], keep, 3, rule, q_attrs)
        ws, rt = W.last(st.a), st.a.retain_stats()
        want = st.b.absorb_keep_raw(q_ids, q_rows, 2, CUT["cosine"], keep, 1, math.inf, q_quality, 3, rule, q_attrs)
        WR.remove_many(E2, leaving)
        TA.same_out(got, want)
        same(rng, st.a, st.b, rule)
        assert WR.snapshot(E, [scene, scene2], K, D) == WR.snapshot(E2, [scene, scene2], K, D)
        assert [int(t) for t in E.order(scene2)] == [int(t) for t in ids[n:]] and E.count(scene) == 0
        ref = st.b.retain_stats()
        assert all(rt[k] == ref[k] for k in ("matched", "created", "rows_moved", "launches", "host_waits", "keep", "qual_upload_bytes"))
        matched = sum(1 for t, d in zip(call, got[4]) if int(t) != int(d))
        if elem == F32:
            assert matched == (16 if ruled else 20)   # under the rule the near-duplicates of another key are created
        assert rt["matched"] == matched and rt["created"] == n - matched
        assert ws["tracks"] == n and ws["launches_capture"] == 1 and ws["feature_bytes_h2d"] == 0 and ws["feature_bytes_d2h"] == 0
        assert ws["rows"] == sum(len(r) for r in q_rows)
