"""Ready tracks handed from one feature store to another on the MI355X (similari_amd.handover over include/similari_handover.h).

The contract admits no tolerance: sa_store_hand_over returns, and leaves in both stores, exactly the bits of fetch + get_attrs on the
source, absorb_keep on the destination and remove on the source.  So every case runs twin PAIRS of stores in one engine — (src A,
dst A) through the one call, (src B, dst B) through the three existing calls — and compares the call's five outputs, and of both
stores order(), fetch_raw rows and qualities as uint32, the attributes, and a tapped search bit for bit (tests/test_gpu_absorb.py's
same_out and same_stores: the cells carry the norms, the groups need d_nobs / d_ids to agree).  The removal, which sa_store_remove now
shares, is held besides against a host model of "the last track moves into the hole", which no library call takes part in.

Shapes are the smallest at which the fill and the compaction can go wrong: D in {5, 33, 64} with K 1, 3, 5 on either side (Kp 4
against 8, Dp 32 / 64 against 64), rows of 260 and 1024 elements for the second pass of a lane, 1 to 1025 tracks against 700 for the
second wave and workgroup, 70 tracks of which up to 65 leave."""
import ctypes as C
import math

import numpy as np
import pytest

import absorb_cases as AC
import test_gpu_absorb as TA
from similari_amd import abi, attrs as AT, handover as H
from similari_amd.engine import Engine, EngineError
from similari_amd.f16 import SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_F32
from similari_amd.i8 import SA_ELEM_I8, I8Store
from similari_amd.merge import SA_KEEP_BEST, SA_KEEP_LATEST
from similari_amd.retain import RetainStore

pytestmark = pytest.mark.gpu
u32, u64, f32 = np.uint32, np.uint64, np.float32
F32, BF16, F16, I8 = SA_ELEM_F32, SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_I8
NAME = {F32: "f32", BF16: "bf16", F16: "f16", I8: "i8"}
FAR, CUT = TA.FAR, TA.CUT
COSINE_ONLY = (BF16, I8)   # cosine for i8 and bf16, both metrics elsewhere
PAIRS = [(s, d) for d in (F32, F16, BF16) for s in (F32, F16, BF16)] + [(F32, I8), (F16, I8), (BF16, I8), (I8, I8)]
FORMS = [(s, d, kind) for s, d in PAIRS for kind in (("cosine",) if d in COSINE_ONLY else ("cosine", "euclidean"))]
SHAPES = [(5, 1, 1), (33, 3, 5), (64, 5, 5)]   # (D, K_src, K_dst)
ZERO_RETAIN = {"step_ms": 0.0, "matched": 0, "created": 0, "rows_moved": 0, "launches": 0, "host_waits": 0, "keep": 0, "qual_upload_bytes": 0}


def form_id(v):
    return NAME.get(v, v) if isinstance(v, int) else str(v)


@pytest.fixture(scope="module")
def engine():
    eng = Engine(abi.make_config(device=0))
    yield eng
    eng.close()


# ---- stores --------------------------------------------------------------------------------------
def make(engine, elem, kind, D, K):
    return I8Store(engine, "cosine", D, K) if elem == I8 else RetainStore(engine, kind, D, K, elem)


def src_kind(elem, kind):
    """visual_kind may differ between the stores (rows are rows): the source takes the other metric where its type has both."""
    return "cosine" if elem in COSINE_ONLY else {"cosine": "euclidean", "euclidean": "cosine"}[kind]


class Pairs:
    """(src A, dst A) for the one call, (src B, dst B) for the three."""

    def __init__(self, engine, se, de, kind, D, Ks, Kd):
        self.stores = []
        for _ in range(4):   # one at a time: a failed creation leaves the earlier ones to close()
            first = len(self.stores) < 2
            self.stores.append(make(engine, se if first else de, src_kind(se, kind) if first else kind, D, Ks if first else Kd))
        self.sa, self.sb, self.da, self.db = self.stores

    def fill(self, which, ids, banks, quality):
        for s in (self.sa, self.sb) if which == "src" else (self.da, self.db):
            s.append(ids, banks, quality, "latest")

    def close(self):
        for s in self.stores:
            s.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def qualities(rng, banks):
    return [rng.uniform(0, 1, len(x)).astype(f32) for x in banks]


def same(rng, a, b, rule=None):
    """TA.same_stores; a store that holds nothing has no search to compare."""
    if len(a) or len(b):
        TA.same_stores(rng, a, b, rule)
    else:
        assert TA.state(a) == TA.state(b)


def three_calls(src, dst, ids, topn, cut, keep, capacity=None, rule=None):
    """The sequence of the header through the calls that were there before; -> the absorb's five outputs."""
    ids = np.asarray(ids, u64)
    n_obs, feats, qual = src.fetch_raw(ids)
    attrs, known = src.get_attrs_raw(ids)
    assert known.all()
    rows = [feats[i, : n_obs[i]] for i in range(len(ids))]
    q = [qual[i, : n_obs[i]] for i in range(len(ids))]
    out = dst.absorb_keep_raw(ids, rows, topn, cut, keep, 1, math.inf, q, capacity, rule, attrs if rule is not None else None)
    src.remove(ids)
    return out


def both_routes(rng, pr, ids, topn, cut, keep, capacity=None, rule=None):
    """One hand-over through both routes, everything compared; -> (dest, handover stats, retain stats of dst A)."""
    ids = np.asarray(ids, u64)
    taken = int(pr.sa.fetch_raw(ids)[0].sum()) if len(ids) else 0
    got = H.hand_over_raw(pr.sa, pr.da, ids, topn, cut, keep, capacity, rule)
    st, rt = H.last(pr.da), dict(pr.da.retain_stats(), reruns=pr.da.last_stats()["reruns"], groups=pr.da.last_stats()["groups"])
    want = three_calls(pr.sb, pr.db, ids, topn, cut, keep, capacity, rule)
    TA.same_out(got, want)
    same(rng, pr.da, pr.db, rule)
    same(rng, pr.sa, pr.sb)
    ref = pr.db.retain_stats()
    assert all(rt[k] == ref[k] for k in ("matched", "created", "rows_moved", "launches", "host_waits", "keep", "qual_upload_bytes"))
    assert pr.da.last_stats()["groups"] == pr.db.last_stats()["groups"] and pr.da.bestfit_stats()["claimed"] == pr.db.bestfit_stats()["claimed"]
    assert st["struct_size"] == C.sizeof(H.sa_handover_stats) == 56
    assert st["feature_bytes_h2d"] == 0 and st["feature_bytes_d2h"] == 0 and st["rows"] == taken
    assert st["launches_fill"] == (1 if len(ids) else 0) and st["launches_compact"] in (0, 1)
    assert (st["tracks_moved"] > 0) == (st["launches_compact"] == 1)
    return got[4], st, rt


def built_on(rng, dst, on, n_obs, D, noise=1e-3):
    """Banks for source tracks: on[i] a stored id of dst — rows on that track's first row (a cosine store: its negation), so it wins —
    or None: random rows."""
    return TA.queries_on(rng, dst, on, n_obs, noise) if any(t is not None for t in on) else [rng.uniform(-1, 1, (int(m), D)).astype(f32) for m in n_obs]


def parity_case(rng, pr, kind, D, Ks, Kd, T=40, n=12):
    """T stored destination tracks with random qualities; n source tracks and two that stay: half built on destination rows (two of
    them on one track: one is matched, the other created), some with fewer than K observations, one with none."""
    d_ids, d_banks = AC.banks(rng, T, Kd, D)
    pr.fill("dst", d_ids, d_banks, qualities(rng, d_banks))
    stored = [int(i) for i in d_ids]
    on = [stored[3], stored[3], None, stored[T - 1], None, stored[0], None, stored[17 % T], None, stored[8], None, None, None, stored[6]][: n + 2]
    n_obs = [Ks, 1, Ks, max(Ks - 1, 1), 1, Ks, 0, 1, max(Ks - 2, 1), Ks, Ks, 1, Ks, Ks][: n + 2]
    s_ids = np.arange(1000, 1000 + n + 2, dtype=u64)
    s_banks = built_on(rng, pr.da, on, n_obs, D)
    pr.fill("src", s_ids, s_banks, qualities(rng, s_banks))
    # handed over out of store order: slots 11, 0, 10, 1, ..; 1012 and 1013 stay
    order = [s_ids[i] for pair in zip(range(n - 1, n // 2 - 1, -1), range(n // 2)) for i in pair]
    return np.array(order, u64), s_ids


# ---- 1. parity over forms ------------------------------------------------------------------------
@pytest.mark.parametrize("keep", ["latest", "best"])
@pytest.mark.parametrize("D,Ks,Kd", SHAPES, ids=str)
@pytest.mark.parametrize("se,de,kind", FORMS, ids=form_id)
def test_a_hand_over_leaves_the_bits_of_fetch_absorb_remove(engine, se, de, kind, D, Ks, Kd, keep):
    rng = np.random.default_rng(10000 * se + 1000 * de + 10 * D + Ks + (kind == "cosine") * 100 + (keep == "best") * 7)
    with Pairs(engine, se, de, kind, D, Ks, Kd) as pr:
        ids, s_ids = parity_case(rng, pr, kind, D, Ks, Kd)
        capacity = None if keep == "latest" else rng.integers(1, Kd + 1, len(ids)).astype(u32)
        dest, st, rt = both_routes(rng, pr, ids, 2, CUT[kind], keep, capacity)
        assert rt["matched"] >= 1 and rt["created"] >= 1 and rt["matched"] + rt["created"] == len(ids)
        assert rt["matched"] == int((dest != ids).sum()) and rt["keep"] == {"latest": SA_KEEP_LATEST, "best": SA_KEEP_BEST}[keep]
        rest = [int(i) for i in pr.sa.order()]
        assert sorted(rest) == [1012, 1013] and st["rows"] > 0
        # the two that stayed leave too, the last one first (no track moves): a second hand-over ranks by the quality mirror the
        # first one left in dst
        dest, st, rt = both_routes(rng, pr, rest[::-1], 2, CUT[kind], keep)
        assert len(pr.sa) == 0 and st["launches_compact"] == 0


# ---- 2. rows wider than one pass of a wave -------------------------------------------------------
@pytest.mark.parametrize("D", [260, 1024], ids=str)
@pytest.mark.parametrize("se,de,kind", [(F32, F32, "euclidean"), (F16, F32, "cosine"), (F32, I8, "cosine")], ids=form_id)
def test_rows_wider_than_one_pass(engine, se, de, kind, D):
    """260 elements: 65 pieces of an f32 row, the second pass is one lane alone; 1024: four full passes.  The copy path, the widen
    path, and the codes of an i8 store."""
    rng = np.random.default_rng(20000 + 10 * D + se + 3 * de)
    with Pairs(engine, se, de, kind, D, 3, 3) as pr:
        ids, s_ids = parity_case(rng, pr, kind, D, 3, 3, T=12, n=8)
        dest, st, rt = both_routes(rng, pr, ids, 2, CUT[kind], "best", 2)
        assert rt["matched"] >= 1 and rt["created"] >= 1


# ---- 3. the source's compaction ------------------------------------------------------------------
T_SRC = 70
SETS = {"none": [], "last": [T_SRC - 1], "first": [0], "all": list(range(T_SRC)), "every_second": list(range(0, T_SRC, 2)),
        "65_of_70": [int(x) for x in np.random.default_rng(3).permutation(T_SRC)[:65]]}


def last_into_hole(order, gone):
    order = list(order)
    for i in gone:
        p = order.index(i)
        order[p] = order[-1]
        order.pop()
    return order


@pytest.mark.parametrize("route", ["hand_over", "take", "remove"])
@pytest.mark.parametrize("which", list(SETS), ids=str)
@pytest.mark.parametrize("elem", [F32, I8], ids=form_id)
def test_the_sources_compaction_equals_sequential_removal(engine, elem, which, route):
    """70 stored tracks; the set leaves through one call on A, one id at a time on B.  Order, banks, qualities and attributes of A
    are held against B and against the host's own replay; the banks on the device through a tapped search."""
    rng = np.random.default_rng(30000 + elem)
    D, K = 33, 3
    kind = "cosine"
    a, b, dst = make(engine, elem, kind, D, K), make(engine, elem, kind, D, K), make(engine, elem, kind, D, K)
    try:
        ids, banks = AC.banks(rng, T_SRC, K, D)
        quality = qualities(rng, banks)
        for s in (a, b):
            s.append(ids, banks, quality, "latest")
            s.set_attrs(ids, ids % 5, np.arange(T_SRC), np.arange(T_SRC) + 3)
        held = {int(i): a.fetch([i])[int(i)] for i in ids}
        held_attrs = a.get_attrs(ids)
        gone = [int(ids[k]) for k in SETS[which]]
        if route == "hand_over":
            out = H.hand_over_raw(a, dst, gone, 1, CUT[kind], "latest")
            assert len(dst) == len(gone) and [int(d) for d in out[4]] == gone   # an empty dst creates every track
            st = H.last(dst)
            got = dst.fetch(gone) if gone else {}
            assert dst.get_attrs(gone) == {g: (0, 0, 0) for g in gone}          # no rule: no attribute arrives
        elif route == "take":
            taken = H.take(a, gone)
            st = H.last(a)
            got = {g: taken[g][:2] for g in gone}
            assert all(taken[g][2] == held_attrs[g] for g in gone)
        else:
            a.remove(gone)
            st = H.last(a)
            got = {}
        for g, (rows, q) in got.items():
            assert rows.tobytes() == held[g][0].tobytes() and q.tobytes() == held[g][1].tobytes(), g
        for g in gone:
            b.remove([g])
        want = last_into_hole([int(i) for i in ids], gone)
        assert [int(i) for i in a.order()] == want
        left = a.fetch(want) if want else {}
        for t in want:
            assert left[t][0].tobytes() == held[t][0].tobytes() and left[t][1].tobytes() == held[t][1].tobytes(), t
        assert a.get_attrs(list(ids)) == {t: held_attrs[t] for t in want}
        same(rng, a, b)
        moves = sum(1 for p, t in enumerate(want) if int(ids[p]) != t)
        assert st["tracks_moved"] == moves and st["launches_compact"] == (1 if moves else 0)
        assert st["feature_bytes_h2d"] == 0 and st["feature_bytes_d2h"] == 0
        if which == "65_of_70":
            assert len(want) == 5 and moves >= 1
    finally:
        for s in (a, b, dst):
            s.close()


# ---- 4. grid edges -------------------------------------------------------------------------------
def test_one_to_1025_tracks_against_700(engine):
    """D = 32, K = 1: the fill's grid is n rows, four per workgroup — one wave alone, a full scan chunk and one past it — and the
    absorb behind it meets its own wave and chunk edges.  The launch counts do not depend on n."""
    D, K, T = 32, 1, 700
    counts = {}
    for n in (1, 64, 65, 1025):
        rng = np.random.default_rng(40000 + n)
        with Pairs(engine, F32, F32, "euclidean", D, K, K) as pr:
            d_ids, d_banks = AC.banks(rng, T, K, D)
            pr.fill("dst", d_ids, d_banks, qualities(rng, d_banks))
            perm = rng.permutation(T)
            on = [int(d_ids[perm[i]]) if i % 3 == 0 and i < T - 1 else None for i in range(n + 3)]
            on[n - 1] = int(d_ids[perm[T - 1]])   # the last one handed over is matched
            s_ids = np.arange(5000, 5000 + n + 3, dtype=u64)
            s_banks = built_on(rng, pr.da, on, [1] * (n + 3), D)
            pr.fill("src", s_ids, s_banks, qualities(rng, s_banks))
            dest, st, rt = both_routes(rng, pr, s_ids[:n], 1, CUT["euclidean"], "latest")
            assert int(dest[n - 1]) == on[n - 1] and rt["matched"] >= 1 and (n == 1 or rt["created"] >= 1)
            assert [int(i) for i in pr.sa.order()] == last_into_hole([int(i) for i in s_ids], [int(i) for i in s_ids[:n]])
            assert st["rows"] == n and st["tracks_moved"] == min(n, 3)
            counts[n] = (st["launches_fill"], st["launches_compact"], rt["launches"])
    assert len(set(counts.values())) == 1 and counts[1] == (1, 1, 3), counts


# ---- 5. under a rule -----------------------------------------------------------------------------
def test_under_a_rule_the_sources_attributes_are_the_queries(engine):
    rng = np.random.default_rng(50)
    D, K, T = 33, 3, 12
    rule = AT.compat(same_key=True, disjoint=True)
    with Pairs(engine, F16, F32, "cosine", D, K, K) as pr:
        d_ids, d_banks = AC.banks(rng, T, K, D)
        pr.fill("dst", d_ids, d_banks, qualities(rng, d_banks))
        for s in (pr.da, pr.db):
            s.set_attrs(d_ids, d_ids % 3, np.arange(T) * 10, np.arange(T) * 10 + 5)
        on = [1, 2, 3, 4, None, 5, 6]   # 0, 1: matched; 2: another key; 3: overlapping span; 4: far; 5: no observation; 6: for the call without a rule
        n_obs = [2, 1, 1, 3, 1, 0, 2]
        s_ids = np.arange(100, 107, dtype=u64)
        s_banks = built_on(rng, pr.da, on, n_obs, D)
        pr.fill("src", s_ids, s_banks, qualities(rng, s_banks))
        for s in (pr.sa, pr.sb):
            s.set_attrs(s_ids, [1, 2, 1, 1, 0, 2, 0], [1000, 1000, 1000, 32, 1000, 1000, 2000], [1005, 1007, 1005, 40, 1001, 1001, 2001])
        dest, st, rt = both_routes(rng, pr, s_ids[:6], 2, CUT["cosine"], "best", 3, rule)
        assert [int(d) for d in dest] == [1, 2, 102, 103, 104, 105]
        got = pr.da.get_attrs(list(d_ids) + list(s_ids[:6]))
        assert got[1] == (1, 0, 1005) and got[2] == (2, 10, 1007) and got[3] == (0, 20, 25)   # the union; an unmatched one stays
        assert got[102] == (1, 1000, 1005) and got[103] == (1, 32, 40) and got[104] == (0, 1000, 1001) and got[105] == (2, 1000, 1001)
        # without a rule no attribute of dst changes: the matched track keeps its own, the attributes of 106 do not arrive
        before = pr.da.get_attrs(list(pr.da.order()))
        dest, st, rt = both_routes(rng, pr, s_ids[6:], 2, CUT["cosine"], "best")
        assert [int(d) for d in dest] == [6] and pr.da.get_attrs(list(pr.da.order())) == before
        assert len(pr.sa) == 0
    # a created track without a rule: attributes (0, 0, 0)
    with Pairs(engine, F32, F32, "cosine", D, K, K) as pr:
        pr.fill("src", [7], [rng.uniform(-1, 1, (2, D)).astype(f32)], None)
        for s in (pr.sa, pr.sb):
            s.set_attrs([7], [4], [1], [9])
        dest, st, rt = both_routes(rng, pr, [7], 1, CUT["cosine"], "latest")
        assert pr.da.get_attrs([7]) == {7: (0, 0, 0)}


# ---- 6. ready and take ---------------------------------------------------------------------------
def test_ready_take_and_the_pipeline_end_to_end(engine):
    rng = np.random.default_rng(60)
    D, K = 33, 3
    I64_MIN, I64_MAX = -2**63, 2**63 - 1
    with Pairs(engine, F32, F32, "cosine", D, K, K) as pr:
        ids, banks = AC.banks(rng, 9, K, D)
        pr.fill("src", ids, banks, qualities(rng, banks))

        def host_filter(s, at):
            order = s.order()
            a, _ = s.get_attrs_raw(order)
            return [int(i) for i, x in zip(order, a) if int(x["end"]) <= at]

        # no attributes ever set: every track is {0, 0, 0}
        assert H.ready(pr.sa, 0) == [int(i) for i in pr.sa.order()] and H.ready(pr.sa, -1) == [] and H.ready(pr.sa, I64_MIN) == []
        assert H.ready(pr.sa, I64_MAX) == [int(i) for i in ids]
        ends = [5, I64_MAX, 20, I64_MIN, 7, 20, 21, 0, 19]
        for s in (pr.sa, pr.sb):
            s.set_attrs(ids, ids % 2, [I64_MIN if e == I64_MIN else min(e, 0) for e in ends], ends)
        for at in (I64_MIN, -1, 0, 5, 6, 19, 20, 21, I64_MAX - 1, I64_MAX):
            assert H.ready(pr.sa, at) == host_filter(pr.sa, at), at
        assert H.ready(pr.sa, I64_MIN) == [4] and len(H.ready(pr.sa, I64_MAX)) == 9
        # the count alone, and a short buffer
        n = C.c_uint32()
        out = np.zeros(2, u64)
        assert pr.sa.lib.sa_store_ready(pr.sa.h, 20, None, 0, C.byref(n)) == 0 and n.value == 7
        assert pr.sa.lib.sa_store_ready(pr.sa.h, 20, out.ctypes.data_as(C.POINTER(C.c_uint64)), 2, C.byref(n)) == 0 and n.value == 7
        assert [int(x) for x in out] == H.ready(pr.sa, 20)[:2]
        # take: fetch's bits plus the attributes, and the ids are gone (an unknown id: nothing, and it is ignored)
        want = [3, 77, 9, 1]
        f_n, f_rows, f_q = pr.sa.fetch_raw(want)
        f_attrs, _ = pr.sa.get_attrs_raw(want)
        t_n, t_rows, t_q, t_attrs = H.take_raw(pr.sa, want)
        TA.same_out((t_n, t_rows.view(u32), t_q.view(u32)), (f_n, f_rows.view(u32), f_q.view(u32)))
        assert t_attrs.tobytes() == f_attrs.tobytes() and t_n[1] == 0
        pr.sb.remove(want)
        same(rng, pr.sa, pr.sb)
        assert sorted(int(i) for i in pr.sa.order()) == [2, 4, 5, 6, 7, 8] and H.last(pr.sa)["launches_compact"] == 1
        # the pipeline, twice: what is ready at 7 leaves for the gallery, then what is ready at 20
        for at in (7, 20):
            baked = H.ready(pr.sa, at)
            assert baked == host_filter(pr.sb, at) and baked
            both_routes(rng, pr, baked, 1, CUT["cosine"], "best")
            assert H.ready(pr.sa, at) == []
        assert sorted(int(i) for i in pr.sa.order()) == [2, 7] and {4, 5, 8} <= {int(i) for i in pr.da.order()} <= {4, 5, 6, 8}


# ---- 7. refusals ---------------------------------------------------------------------------------
def test_refusals_leave_both_stores_as_they_were(engine):
    rng = np.random.default_rng(70)
    D, K, T = 33, 3, 8
    with Pairs(engine, F32, F32, "cosine", D, K, K) as pr:
        d_ids, d_banks = AC.banks(rng, T, K, D)
        pr.fill("dst", d_ids, d_banks, qualities(rng, d_banks))
        s_ids = np.array([40, 41, 42, 43, 3], u64)   # 3 is an id of dst too
        s_banks = built_on(rng, pr.da, [1, None, 2, None, None], [2, 1, 3, 0, 1], D)
        pr.fill("src", s_ids, s_banks, qualities(rng, s_banks))
        both_routes(rng, pr, [40], 1, CUT["cosine"], "best")   # the mirror of dst is valid from here on
        others = {
            "engine": Engine(abi.make_config(device=0)),
        }
        others.update(other_engine=RetainStore(others["engine"], "cosine", D, K, F32), narrow=RetainStore(engine, "cosine", D - 1, K, F32),
                      short=RetainStore(engine, "cosine", D, 2, F32), i8=I8Store(engine, "cosine", D, K), f16=RetainStore(engine, "cosine", D, K, F16))
        try:
            others["i8"].upsert([41], [s_banks[1]])
            others["other_engine"].upsert([41], [s_banks[1]])
            others["narrow"].upsert([41], [s_banks[1][:, : D - 1]])
            src, dst = pr.sa, pr.da
            before = TA.state(src), TA.state(dst)
            h = H.hand_over_raw
            o = others
            cases = [   # (code, a word of the message, src, dst, ids, topn, further arguments)
                (abi.SA_ERR_BAD_ARG, "one store", src, src, [41], 1, {}),
                (abi.SA_ERR_BAD_ARG, "two engines", o["other_engine"], dst, [41], 1, {}),
                (abi.SA_ERR_BAD_ARG, "feature_len", o["narrow"], dst, [41], 1, {}),
                (abi.SA_ERR_BAD_ARG, "does not hold", src, dst, [41, 999], 1, {}),
                (abi.SA_ERR_BAD_ARG, "id 0", src, dst, [0, 41], 1, {}),
                (abi.SA_ERR_BAD_ARG, "twice", src, dst, [41, 41], 1, {}),
                (abi.SA_ERR_BAD_ARG, "observations", src, o["short"], [41, 42], 1, {}),
                (abi.SA_ERR_UNSUPPORTED, "i8 source", o["i8"], o["f16"], [41], 1, {}),
                (abi.SA_ERR_UNSUPPORTED, "i8 source", o["i8"], dst, [41], 1, {}),
                (abi.SA_ERR_BAD_ARG, "stored", src, dst, [41, 3], 1, {}),                                   # the absorb's own: dst holds 3
                (abi.SA_ERR_BAD_ARG, "unknown keep", src, dst, [41], 1, dict(keep=2)),
                (abi.SA_ERR_BAD_ARG, "topn", src, dst, [41], 0, {}),
                (abi.SA_ERR_BAD_ARG, "capacity", src, dst, [41, 42], 1, dict(capacity=[1, K + 1])),
                (abi.SA_ERR_BAD_ARG, "unknown rule bits", src, dst, [41], 1, dict(compat=AT.Compat(0x100))),
                (abi.SA_ERR_BAD_ARG, "exclude each other", src, dst, [41], 1, dict(compat=AT.compat(disjoint=True, query_first=True))),
            ]
            for code, word, s, d, ids, topn, kw in cases:
                was = TA.state(s), TA.state(d)
                with pytest.raises(EngineError) as ex:
                    h(s, d, ids, topn, 0.5, **kw)
                assert ex.value.code == code and word in str(ex.value), (word, ex.value.code, str(ex.value))
                assert (TA.state(s), TA.state(d)) == was and (TA.state(src), TA.state(dst)) == before, word
                assert d.retain_stats() == ZERO_RETAIN, word
                assert H.last(d)["launches_fill"] == 0 and H.last(d)["rows"] == 0, word
            assert len(others["i8"]) == 1 and len(others["short"]) == 0 and len(others["f16"]) == 0
            # null ids and null outputs through the C call itself
            from similari_amd.search import sa_topn_params

            prm = sa_topn_params(1, 1, 0.5, math.inf)
            ids = np.array([41], u64)
            out_n, win, wt, dest = np.zeros(1, u32), np.zeros((1, 1), u64), np.zeros((1, 1), np.float64), np.zeros(1, u64)
            p64, p32, pd = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_double)
            full = [ids.ctypes.data_as(p64), None, out_n.ctypes.data_as(p32), win.ctypes.data_as(p64), None, wt.ctypes.data_as(pd), dest.ctypes.data_as(p64)]
            for hole in (0, 2, 6):
                args = list(full)
                args[hole] = None
                rc = dst.lib.sa_store_hand_over(src.h, dst.h, 0, C.byref(prm), None, 1, *args)
                assert rc == abi.SA_ERR_BAD_ARG and "null argument" in dst.lib.sa_last_error(dst.engine.h).decode(), hole
                assert (TA.state(src), TA.state(dst)) == before, hole
            # n == 0 does nothing
            got = h(src, dst, [], 1, 0.5)
            assert len(got[0]) == 0 and (TA.state(src), TA.state(dst)) == before
            # the mirror of dst is as it was — valid —, and the next hand-over equals the twin without an upload
            pr.sb.remove([3])
            src.remove([3])
            dest, st, rt = both_routes(rng, pr, [42, 41, 43], 1, CUT["cosine"], "best")
            assert int(dest[0]) == 2 and rt["qual_upload_bytes"] == 0
        finally:
            for k in ("other_engine", "narrow", "short", "i8", "f16"):
                others[k].close()
            others["engine"].close()


# ---- 8. the counters, small against large --------------------------------------------------------
def test_no_feature_byte_crosses_the_bus_and_rows_are_counted(engine):
    """both_routes asserts the counters of every hand-over in this file; here they are held for one small and one large call into
    the same destination, with the observations counted by hand."""
    rng = np.random.default_rng(80)
    D, K = 64, 5
    with Pairs(engine, BF16, F16, "cosine", D, K, K) as pr:
        n_obs = [int(m) for m in rng.integers(0, K + 1, 200)]
        s_ids = np.arange(1, 201, dtype=u64)
        banks = [rng.uniform(-1, 1, (m, D)).astype(f32) for m in n_obs]
        pr.fill("src", s_ids, banks, qualities(rng, banks))
        seen = []
        for ids in (s_ids[:2], s_ids[2:190]):
            dest, st, rt = both_routes(rng, pr, ids, 1, CUT["cosine"], "best")
            k = int(ids[0]) - 1
            assert st["rows"] == sum(n_obs[k: k + len(ids)]) and st["feature_bytes_h2d"] == st["feature_bytes_d2h"] == 0
            assert st["fill_ms"] > 0 and st["compact_ms"] > 0
            seen.append((st["launches_fill"], st["launches_compact"]))
        assert seen[0] == seen[1] == (1, 1)


# ---- 9. a pool rerun applies everything once -----------------------------------------------------
def test_a_pool_rerun_applies_everything_once(engine):
    """As tests/test_gpu_retain.py: 24 x 21 groups outgrow a fresh pool, dst's search runs twice over the query rows the fill wrote
    once, the step rides behind the second run, and src's removal runs once behind it."""
    rng = np.random.default_rng(90)
    D, K, T, n = 33, 3, 21, 24
    with Pairs(engine, F32, F16, "euclidean", D, K, K) as pr:
        d_ids = np.arange(1, T + 1, dtype=u64)
        d_banks = [rng.uniform(-1, 1, (K, D)).astype(f32) for _ in range(T)]
        pr.fill("dst", d_ids, d_banks, qualities(rng, d_banks))
        s_ids = np.arange(500, 500 + n + 2, dtype=u64)
        s_banks = [rng.uniform(-1, 1, (K, D)).astype(f32) for _ in range(n + 2)]
        pr.fill("src", s_ids, s_banks, qualities(rng, s_banks))
        dest, st, rt = both_routes(rng, pr, s_ids[:n], 3, FAR, "best", 2)
        assert rt["groups"] == n * T and rt["reruns"] == 1 and rt["launches"] == 3 and rt["host_waits"] == 3
        assert rt["matched"] >= 1 and rt["created"] >= n - T
        assert st["launches_fill"] == 1 and st["launches_compact"] == 1 and st["tracks_moved"] == 2 and st["rows"] == n * K
        assert [int(i) for i in pr.sa.order()] == last_into_hole([int(i) for i in s_ids], [int(i) for i in s_ids[:n]])
