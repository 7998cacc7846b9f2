"""A frame's tracks absorbed in one call on the MI355X (similari_amd.absorb.AbsorbStore over include/similari_absorb.h).

The contract admits no tolerance: a call returns, and leaves in the store, exactly the bits of search_bestfit followed by append
(and set_attrs under a rule).  So every case runs twin stores in one engine — A through absorb, B through the two calls — and
compares after every step: the outputs, order(), fetch_raw rows and qualities as uint32, and a tapped search of both stores bit for
bit, whose cells carry the norms and whose groups need d_nobs / d_ids to agree.  Shapes are the smallest at which the step can go
wrong: D in {5, 33, 64}, K in {1, 3, 5} (Kp = 1, 4, 8: a bank that is always full, and padding slots), 6-40 stored tracks, 1-24 queries.

Two tests go past the first turn of the step's loops (tests/absorb_cases.py builds them): a frame of up to 2100 queries against 700
stored tracks — the second wave and the second and third chunk of the scan, matched slots in every lane group of the id walk — and
banks of rows wider than one pass of a wave, shifted in place.  Both are held, beyond the twin, against the plain host model
(tests/merge_ref.py and its rounding subclasses) and against a probe search, which reads the device's id table."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest

import absorb_cases as AC
import hipmem
from similari_amd import abi, attrs as AT
from similari_amd.absorb import AbsorbStore
from similari_amd.devrows import DeviceRows
from similari_amd.engine import Engine, EngineError
from similari_amd.f16 import SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_F32

pytestmark = pytest.mark.gpu
u16, u32, u64, f32 = np.uint16, np.uint32, np.uint64, np.float32
F32, BF16, F16 = SA_ELEM_F32, SA_ELEM_BF16, SA_ELEM_F16
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
STORES = [(F32, "cosine"), (F32, "euclidean"), (F16, "cosine"), (F16, "euclidean"), (BF16, "cosine")]
SHAPES = [(5, 1), (33, 3), (64, 5)]   # (D, K)
FAR = 3.0e38                          # above every distance
CUT = AC.CUT                          # a query built on a stored row lies below the cut, random rows lie far above it


@pytest.fixture(scope="module")
def engine():
    eng = Engine(abi.make_config(device=0))
    yield eng
    eng.close()


# ---- comparisons ---------------------------------------------------------------------------------
def same_out(a, b):
    """Two tuples of arrays (or None): dtype, shape and every bit."""
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), i
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape, i
            assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), "output %d differs" % i


def same_bits(a, b):
    """same_bits of tests/test_gpu_merge.py: two tapped search results (out_n, winners, weights, cells)."""
    for x, y in zip(a[:2], b[:2]):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))
    assert a[3].shape == b[3].shape
    assert np.array_equal(np.isnan(a[3]), np.isnan(b[3]))
    m = ~np.isnan(a[3])
    assert np.array_equal(a[3][m].view(np.uint32), b[3][m].view(np.uint32))


def state(s):
    ids = s.order()
    n_obs, feats, qual = s.fetch_raw(ids)
    attrs = s.get_attrs_raw(ids)[0].tobytes() if len(ids) else b""
    return len(s), ids.tobytes(), n_obs.tobytes(), feats.view(u32).tobytes(), qual.view(u32).tobytes(), attrs


def same_stores(rng, a, b, rule=None):
    """order(), rows and qualities as uint32, attributes, and one tapped search of both (under the rule too when there is one)."""
    assert state(a) == state(b)
    nq = 4
    q_ids = np.arange(900001, 900001 + nq, dtype=u64)
    q = [rng.uniform(-1, 1, (int(m), a.D)).astype(f32) for m in rng.integers(1, a.K + 1, nq)]
    same_bits(a.search_raw(q_ids, q, 3, FAR, tap=True), b.search_raw(q_ids, q, 3, FAR, tap=True))
    if rule is not None:
        qa = AT.pack_attrs([0, 1, 2, 0], [0] * nq, [1] * nq)
        same_bits(a.search_raw(q_ids, q, 3, FAR, tap=True, compat=rule, q_attrs=qa), b.search_raw(q_ids, q, 3, FAR, tap=True, compat=rule, q_attrs=qa))


# ---- the two routes ------------------------------------------------------------------------------
def dest_of(q_ids, out_n, win):
    """Step 2 of the header on the BestFit call's outputs."""
    return np.array([win[i, 0] if out_n[i] >= 1 and win[i, 0] != q else q for i, q in enumerate(q_ids)], u64)


def union_attrs(b, dest, q_ids, q_attrs):
    """Step 4 for store B, which has run its append: a created track takes the query's attributes, a matched one the union."""
    have, _ = b.get_attrs_raw(dest)
    out = np.array(q_attrs, copy=True)
    for i, (d, q) in enumerate(zip(dest, q_ids)):
        if d != q:
            out[i]["key"] = have[i]["key"]
            out[i]["start"] = min(int(have[i]["start"]), int(q_attrs[i]["start"]))
            out[i]["end"] = max(int(have[i]["end"]), int(q_attrs[i]["end"]))
    return out


def step(rng, a, b, q_ids, feats, topn, cut, quality=None, capacity=None, rule=None, q_attrs=None, min_votes=1, keep_below=math.inf):
    """One frame through both routes, everything compared; -> (dest, absorb_stats)."""
    q_ids = np.asarray(q_ids, u64)
    got = a.absorb_raw(q_ids, feats, topn, cut, min_votes, keep_below, quality, capacity, rule, q_attrs)
    st = dict(a.absorb_stats(), reruns=a.last_stats()["reruns"], groups=a.last_stats()["groups"])   # of the absorb's own search
    out_n, win, trk, wt, _ = b.search_bestfit_raw(q_ids, feats, topn, cut, min_votes, keep_below, compat=rule, q_attrs=q_attrs)
    dest = dest_of(q_ids, out_n, win)
    b.append(dest, feats, quality, "latest", capacity)
    if rule is not None and len(q_ids):
        b.set_attrs_raw(dest, union_attrs(b, dest, q_ids, q_attrs))
    same_out(got, (out_n, win, trk, wt, dest))
    same_stores(rng, a, b, rule)
    n = len(q_ids)
    assert st["matched"] + st["created"] == n and st["matched"] == int((dest != q_ids).sum())
    return dest, st


def twin_of(engine, kind, D, K, elem, ids, banks):
    a, b = AbsorbStore(engine, kind, D, K, elem), AbsorbStore(engine, kind, D, K, elem)
    for s in (a, b):
        s.upsert(ids, banks)
    return a, b


def twin(engine, kind, D, K, elem, T, rng):
    if T:
        return twin_of(engine, kind, D, K, elem, *AC.banks(rng, T, K, D))
    return AbsorbStore(engine, kind, D, K, elem), AbsorbStore(engine, kind, D, K, elem)


def queries_on(rng, store, on, n_obs, noise=1e-3):
    """One query per entry of `on`: a stored id — its rows are that track's first row (a cosine store: its negation) plus a little
    noise, so the track is its winner — or None: random rows, far from everything."""
    banks = {int(t): store.fetch([t])[int(t)][0] for t, m in zip(on, n_obs) if t is not None and m != 0}
    return AC.frame(rng, banks, on, n_obs, store.kind, noise, D=store.D)[0]


# ---- 1. five consecutive frames, every store type and shape -------------------------------------
@pytest.mark.parametrize("D,K", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("elem,kind", STORES, ids=lambda v: NAME.get(v, v) if isinstance(v, int) else v)
def test_five_frames_leave_the_bits_of_search_then_append(engine, elem, kind, D, K):
    """Banks fill, shift and shrink.  Frame capacities: NULL, NULL, 2 (< n0 for a full bank: the zeroed tail), 1, one per query.
    Every frame has matched queries, two queries built on one stored track (one matched, one created), a query far from everything,
    a query without observations, and a full-length query into a bank (drop >= n0 once the capacity is below K)."""
    rng = np.random.default_rng(100 * elem + 10 * K + (kind == "cosine"))
    a, b = twin(engine, kind, D, K, elem, 6, rng)
    try:
        next_id = 1000
        caps = [None, None, min(2, K), 1, "mixed"]
        sizes = [7, 24, 9, 12, 1]
        for frame, (cap, Q) in enumerate(zip(caps, sizes)):
            stored = [int(i) for i in a.order()]
            full = [t for t in stored if len(a.fetch([t])[t][0]) == K]
            on = [stored[0], stored[0], None, stored[1 % len(stored)], None] + [stored[k % len(stored)] if k % 3 else None for k in range(2, 21)]
            n_obs = [1, 1, 1, K, 0] + [int(m) for m in rng.integers(0, K + 1, 19)]
            if full:
                on[3] = full[-1]   # K rows into a full bank
            on, n_obs = on[:Q], n_obs[:Q]
            if Q == 1:
                on, n_obs = [stored[2]], [K]
            seen = set()
            for k, t in enumerate(on):   # beyond the first pair each stored track is named once
                if k >= 2 and t is not None:
                    on[k] = None if t in seen or t == stored[0] else t
                    seen.add(t)
            q_ids = np.arange(next_id, next_id + Q, dtype=u64)
            next_id += Q
            feats = queries_on(rng, a, on, n_obs)
            quality = [rng.uniform(0, 1, int(m)).astype(f32) for m in n_obs] if frame != 1 else None
            capacity = rng.integers(1, K + 1, Q).astype(u32) if cap == "mixed" else cap
            dest, st = step(rng, a, b, q_ids, feats, 2, CUT[kind], quality, capacity)
            assert st["launches"] == 3 and st["host_waits"] == 2 and st["reruns"] == 0
            if frame == 0:   # two queries on one stored track: one is matched, the other created (later frames find the loser's track too)
                assert (dest[0] == stored[0]) != (dest[1] == stored[0]) and {int(dest[0]), int(dest[1])} - {stored[0]} <= {int(q_ids[0]), int(q_ids[1])}
            if Q > 1:   # the best group of the call holds its claim and is its query's entry 0; query 4 has no observation
                assert st["matched"] >= 1 and st["created"] >= 1
    finally:
        a.close()
        b.close()


# ---- 2. edge frames ------------------------------------------------------------------------------
def test_edge_frames(engine):
    rng = np.random.default_rng(2)
    D, K = 33, 3
    a, b = twin(engine, "euclidean", D, K, F32, 0, rng)
    try:
        # an empty store: every query is created, the one without observations too
        q_ids = np.arange(10, 18, dtype=u64)
        n_obs = [1, 0, 3, 2, 1, 1, 3, 2]
        dest, st = step(rng, a, b, q_ids, queries_on(rng, a, [None] * 8, n_obs), 2, CUT["euclidean"], capacity=2)
        assert np.array_equal(dest, q_ids) and st["created"] == 8 and st["launches"] == 2 and st["host_waits"] == 1
        assert np.array_equal(a.order(), q_ids) and list(a.fetch_raw(q_ids)[0]) == [1, 0, 2, 2, 1, 1, 2, 2]
        # n_queries == 0: nothing happens
        before = state(a)
        dest, st = step(rng, a, b, np.zeros(0, u64), [], 2, CUT["euclidean"])
        assert state(a) == before
        assert a.absorb_stats() == {"step_ms": 0.0, "matched": 0, "created": 0, "rows_moved": 0, "launches": 0, "host_waits": 0}
        # no match at all
        dest, st = step(rng, a, b, [30, 31, 32], queries_on(rng, a, [None] * 3, [1, 2, 3]), 2, CUT["euclidean"])
        assert st["matched"] == 0 and len(a) == 11
        # every query matched, each on its own stored track (the empty track 11 cannot be one)
        on = [10, 12, 13, 14, 15]
        dest, st = step(rng, a, b, [40, 41, 42, 43, 44], queries_on(rng, a, on, [3, 3, 1, 2, 3]), 1, CUT["euclidean"], capacity=[1, 3, 2, 3, 2])
        assert [int(d) for d in dest] == on and st["created"] == 0 and len(a) == 11
        # the whole old bank leaves: three rows into a bank of two at capacity 3, and into a bank at capacity 1
        n0 = a.fetch_raw([12, 13])[0]
        dest, st = step(rng, a, b, [50, 51], queries_on(rng, a, [12, 13], [3, 3]), 1, CUT["euclidean"], capacity=[3, 1])
        assert [int(d) for d in dest] == [12, 13] and list(a.fetch_raw([12, 13])[0]) == [3, 1] and n0[0] >= 1
    finally:
        a.close()
        b.close()


# ---- 3. growth: T + n_queries crosses the store's capacity ---------------------------------------
def test_the_reservation_reallocates_mid_sequence(engine):
    """A store's device arrays start at 64 tracks.  40 stored and 24 queries fit; the next frame's T + 24 does not, so the arrays move
    before the search that feeds the step, with matched queries in the same frame."""
    rng = np.random.default_rng(3)
    D, K = 33, 3
    a, b = twin(engine, "cosine", D, K, F16, 40, rng)
    try:
        next_id = 2000
        for frame in range(3):
            stored = [int(i) for i in a.order()]
            on = [stored[k] if k % 6 == 0 else None for k in range(24)]
            n_obs = [int(m) for m in rng.integers(1, K + 1, 24)]
            dest, st = step(rng, a, b, np.arange(next_id, next_id + 24, dtype=u64), queries_on(rng, a, on, n_obs), 1, CUT["cosine"], capacity=2)
            next_id += 24
            assert st["matched"] == 4 and st["created"] == 20
        assert len(a) == 100
    finally:
        a.close()
        b.close()


# ---- 4. a pool rerun: the step is applied once ---------------------------------------------------
def test_a_pool_rerun_applies_the_step_once(engine):
    """Fresh stores (a first pool holds 256 blocks): 24 queries of three rows against 21 full banks, max_distance above every
    distance: 504 groups, so the search runs twice.  The step rides behind the second run alone."""
    rng = np.random.default_rng(4)
    D, K, T, Q = 33, 3, 21, 24
    a, b = AbsorbStore(engine, "euclidean", D, K, F16), AbsorbStore(engine, "euclidean", D, K, F16)
    try:
        ids = np.arange(1, T + 1, dtype=u64)
        banks = [rng.uniform(-1, 1, (K, D)).astype(f32) for _ in range(T)]
        for s in (a, b):
            s.upsert(ids, banks)
        feats = [rng.uniform(-1, 1, (K, D)).astype(f32) for _ in range(Q)]
        dest, st = step(rng, a, b, np.arange(500, 500 + Q, dtype=u64), feats, 3, FAR, capacity=2)
        assert st["groups"] == Q * T == 504 and st["reruns"] == 1
        assert st["launches"] == 3 and st["host_waits"] == 3
        assert st["matched"] >= 1 and st["created"] >= Q - T   # at most one query per stored track
    finally:
        a.close()
        b.close()


# ---- 5. under a rule -----------------------------------------------------------------------------
def test_under_a_rule_matched_and_created_tracks_get_their_attributes(engine):
    rng = np.random.default_rng(5)
    D, K, T = 33, 3, 12
    a, b = twin(engine, "cosine", D, K, F32, T, rng)
    try:
        ids = np.arange(1, T + 1, dtype=u64)
        for s in (a, b):
            s.set_attrs(ids, ids % 3, np.arange(T) * 10, np.arange(T) * 10 + 5)
        rule = AT.compat(same_key=True, disjoint=True)
        # query k is built on stored track k + 1.  0, 1: same key, later span: matched.  2: another key: dead pair, created.
        # 3: same key, overlapping span: dead pair, created.  4: far from everything.  5: no observation.
        on = [1, 2, 3, 4, None, 5]
        q_ids = np.arange(100, 106, dtype=u64)
        q_attrs = AT.pack_attrs([1, 2, 1, 1, 0, 2], [1000, 1000, 1000, 32, 1000, 1000], [1005, 1007, 1005, 40, 1001, 1001])
        dest, st = step(rng, a, b, q_ids, queries_on(rng, a, on, [2, 1, 1, 3, 1, 0]), 2, CUT["cosine"], capacity=3, rule=rule, q_attrs=q_attrs)
        assert [int(d) for d in dest] == [1, 2, 102, 103, 104, 105]
        got = a.get_attrs(list(ids) + list(q_ids))
        assert got[1] == (1, 0, 1005) and got[2] == (2, 10, 1007)          # the union keeps the destination's key
        assert got[3] == (0, 20, 25) and got[4] == (1, 30, 35)              # untouched
        assert got[102] == (1, 1000, 1005) and got[103] == (1, 32, 40) and got[104] == (0, 1000, 1001) and got[105] == (2, 1000, 1001)
        assert 100 not in got and 101 not in got
        # a second frame sees the merged spans: a query inside the widened span of track 1 is a dead pair now
        q_attrs = AT.pack_attrs([1, 2], [500, 2000], [600, 2001])
        dest, st = step(rng, a, b, [110, 111], queries_on(rng, a, [1, 2], [1, 1]), 2, CUT["cosine"], rule=rule, q_attrs=q_attrs)
        assert [int(d) for d in dest] == [110, 2]
    finally:
        a.close()
        b.close()


# ---- 5a. past the first turn of the step's loops --------------------------------------------------
def holds(store, model):
    """order() and fetch_raw of every id, as uint32, against a host model (merge_ref.Model, or its rounding subclass)."""
    ids = store.order()
    assert [int(i) for i in ids] == model.order
    same_out(store.fetch_raw(ids), AC.held(model, model.order))


def probe(store, case, tracks):
    """A TopN search whose query k sits on a row of tracks[k]: rank 0 names exactly that id.  The rows say that the step wrote the
    right slots, the ids that d_ids and d_nobs agree with them — fetch reads the host's table and cannot see the device's."""
    q_ids, q = AC.probes(case, tracks)
    out_n, win, _, _ = store.search_raw(q_ids, q, 1, CUT[case["kind"]])
    assert np.array_equal(out_n, np.ones(len(tracks), u32)) and [int(w) for w in win[:, 0]] == [int(t) for t in tracks]


def run_case(engine, case):
    """One frame through step() — the twin, every output and the whole store — and then, independent of the twin: the destinations
    the data dictates and the store the host model leaves.  -> (a, b, dest, stats); the caller closes."""
    a, b = twin_of(engine, case["kind"], case["D"], case["K"], case["elem"], case["ids"], case["banks"])
    try:
        holds(a, case["model"])
        old = a.order()
        dest, st = step(case["rng"], a, b, case["q_ids"], case["feats"], 2, CUT[case["kind"]], case["quality"], case["capacity"])
        assert np.array_equal(dest, case["expected_dest"])
        created = case["q_ids"][dest == case["q_ids"]]
        assert np.array_equal(a.order(), np.concatenate([old, created]))   # the old order, then the created ids in query order
        holds(a, case["after"])
        assert st["launches"] == 3
        return a, b, dest, st
    except BaseException:
        a.close()
        b.close()
        raise


@pytest.mark.parametrize("Q", sorted({q for q, _ in AC.WAVE_QS}))
def test_a_frame_past_one_wave_and_one_scan_chunk(engine, Q):
    """700 stored tracks, Q queries, f32 euclidean, D = 33, K = 2.  Q = 64 fills one wave of k_absorb_rank and 65 opens the second
    (its base comes out of w_sum[]); 1024 fills one chunk and 1025 opens the second (the carry; a last chunk of one query); 2100 has
    three chunks with a ragged last one.  65 and 1025 run with the lone last query created and with it matched.  The matched slots
    lie all over [0, 700): every lane group u of k_absorb_match's walk and its second and third turn.  Nothing is asserted about
    reruns: several hundred groups survive the cut and outgrow a fresh pool, which test_a_pool_rerun_applies_the_step_once covers."""
    for last in [l for q, l in AC.WAVE_QS if q == Q]:
        case = AC.wave_case(Q, last)
        a, b, dest, st = run_case(engine, case)
        try:
            q_ids = case["q_ids"]
            matched = dest != q_ids
            slots = dest[matched].astype(np.int64) - 1   # ids 1..T were upserted in this order: id t lies in slot t - 1
            if last is not None:
                assert bool(matched[-1]) == last
            if Q == 2100:   # the paths were met
                for lo, hi in AC.SCAN_CHUNKS:
                    assert matched[lo:hi].any() and not matched[lo:hi].all(), (lo, hi)
                for lo, hi in AC.SLOT_RANGES:
                    assert ((slots >= lo) & (slots < hi)).any(), (lo, hi)
            # the device's id table: a created track with a row out of every scan chunk (its first and its last), a matched track out
            # of every slot range, and stored tracks the frame left alone
            n_obs = np.array(case["n_obs"])
            tracks = []
            for lo, hi in AC.SCAN_CHUNKS:
                fresh = [int(q) for q in q_ids[lo:hi][~matched[lo:hi] & (n_obs[lo:hi] > 0)]]
                tracks += fresh[:1] + fresh[1:][-1:]
            for lo, hi in AC.SLOT_RANGES:
                tracks += [int(s) + 1 for s in slots[(slots >= lo) & (slots < hi)][:2]]
            tracks += [int(t) for t in case["ids"] if int(t) not in set(dest.tolist())][:3]
            assert len(set(tracks)) == len(tracks) >= (17 if Q == 2100 else 6)   # 2100: two per chunk, two per range, three at rest
            probe(a, case, tracks)
            probe(b, case, tracks)
        finally:
            a.close()
            b.close()


@pytest.mark.parametrize("elem,kind,D", AC.WIDE_FORMS, ids=lambda v: NAME.get(v, v) if isinstance(v, int) and v < 3 else str(v))
def test_banks_shift_in_place_at_widths_beyond_one_pass(engine, elem, kind, D):
    """k_absorb_move gives lane l the 16-byte pieces l, l + 64, .. of a row.  f32 at D = 260: Dp 288, 72 pieces, the second pass is
    lanes 0-7 alone; f32 at 1024: four full passes; f16 at 1024: 128 pieces; bf16 at 520: Dp 544, 68 pieces.  The frame
    (absorb_cases.wide_case) shifts a bank onto itself by two and by three rows, replaces one whole, leaves one where it is and
    creates tracks with 0, 1 and K rows — a row torn between two passes of a lane shows in fetch_raw against the host model."""
    case = AC.wide_case(elem, kind, D)
    a, b, dest, st = run_case(engine, case)
    try:
        assert st["matched"] == 6 and st["created"] == 4 and st["host_waits"] == 2 and st["reruns"] == 0
        touched = [1, 2, 3, 4, 5, 7, 505, 506]   # every track the frame gave a row
        probe(a, case, touched + [8, 12])
        probe(b, case, touched + [8, 12])
    finally:
        a.close()
        b.close()


# ---- 6. rows from device memory ------------------------------------------------------------------
@contextlib.contextmanager
def device_block(engine, image):
    ptr = hipmem.malloc(image.nbytes)
    try:
        hipmem.upload(ptr, image)
        engine.register_device_block(ptr, image.nbytes, 0)
        yield ptr
    finally:
        engine.unregister_device_block(ptr)
        hipmem.free(ptr)


def to_bits(x, elem):
    return x.astype(np.float16).view(u16) if elem == F16 else (x.view(u32) >> 16).astype(u16)


@pytest.mark.parametrize("store_elem,kind,src_elem", [(F16, "euclidean", F16), (F32, "cosine", BF16)], ids=["f16_into_f16", "bf16_into_f32"])
def test_absorb_rows_from_device_memory(engine, store_elem, kind, src_elem):
    """Strided 16-bit rows gathered through an index: absorb_rows against search_rows (BestFit) followed by append_rows."""
    rng = np.random.default_rng(6 + src_elem)
    D, K, T = 33, 3, 10
    a, b = twin(engine, kind, D, K, store_elem, T, rng)
    try:
        next_id = 300
        for frame in range(2):
            stored = [int(i) for i in a.order()]
            on = [stored[0], stored[0], None, stored[3], stored[4], None, stored[5]]
            n_obs = np.array([1, 2, 3, 3, 1, 0, 2], u32)
            q_ids = np.arange(next_id, next_id + len(on), dtype=u64)
            next_id += len(on)
            total = int(n_obs.sum())
            rows = np.concatenate(queries_on(rng, a, on, n_obs))
            index = rng.permutation(total + 2)[:total].astype(u32)
            bits = np.zeros((total + 2, D), u16)
            bits[index] = to_bits(rows, src_elem)
            stride = D + 3
            img = np.full((total + 1) * stride + D, 0x7FFF, u16)   # NaN patterns between the rows
            for r in range(total + 2):
                img[r * stride: r * stride + D] = bits[r]
            quality = rng.uniform(0, 1, total).astype(f32)
            with device_block(engine, img) as ptr:
                dr = DeviceRows(ptr, total + 2, stride, src_elem, index)
                got = a.absorb_rows_raw(q_ids, n_obs, dr, 2, CUT[kind], quality=quality, capacity=2)
                st = a.absorb_stats()
                out_n, win, trk, wt, _ = b.search_rows_raw(q_ids, n_obs, dr, 2, CUT[kind], vote="bestfit")
                dest = dest_of(q_ids, out_n, win)
                b.append_rows(dest, n_obs, dr, quality, 2)
            same_out(got, (out_n, win, trk, wt, dest))
            same_stores(rng, a, b)
            assert a.devrows_stats()["rows"] == total and st["matched"] >= 2 and st["created"] >= 2 and st["host_waits"] == 2
    finally:
        a.close()
        b.close()


# ---- 7. stats ------------------------------------------------------------------------------------
def test_launches_do_not_depend_on_the_number_of_queries(engine):
    rng = np.random.default_rng(7)
    D, K = 64, 5
    a, b = twin(engine, "cosine", D, K, BF16, 30, rng)
    try:
        stored = [int(i) for i in a.order()]
        _, one = step(rng, a, b, [700], queries_on(rng, a, [stored[0]], [2]), 1, CUT["cosine"])
        on = [stored[k] if k % 2 else None for k in range(24)]
        _, many = step(rng, a, b, np.arange(800, 824, dtype=u64), queries_on(rng, a, on, [1 + k % K for k in range(24)]), 1, CUT["cosine"])
        assert one["launches"] == many["launches"] == 3 and one["host_waits"] == many["host_waits"] == 2
        assert one["matched"] == 1 and one["rows_moved"] == 2 and many["matched"] + many["created"] == 24
        assert one["step_ms"] > 0 and many["step_ms"] > 0
    finally:
        a.close()
        b.close()


# ---- 8. refusals ---------------------------------------------------------------------------------
def test_refusals_leave_the_store_as_it_was(engine):
    rng = np.random.default_rng(8)
    D, K, T = 33, 3, 8
    a, b = twin(engine, "cosine", D, K, F32, T, rng)
    b.close()
    try:
        before = state(a)
        ok_ids = np.array([50, 51], u64)
        ok = [rng.uniform(-1, 1, (2, D)).astype(f32), rng.uniform(-1, 1, (1, D)).astype(f32)]
        rule = AT.compat(same_key=True)
        qa = AT.pack_attrs([0, 1], [0, 0], [5, 5])
        nan_q = [np.array([0.5, np.nan], f32), np.array([0.5], f32)]
        cases = [
            (abi.SA_ERR_BAD_ARG, "stored", lambda: a.absorb_raw([50, 3], ok, 1, 0.5)),                       # a query id the store holds
            (abi.SA_ERR_BAD_ARG, "id 0", lambda: a.absorb_raw([0, 51], ok, 1, 0.5)),
            (abi.SA_ERR_BAD_ARG, "twice", lambda: a.absorb_raw([50, 50], ok, 1, 0.5)),
            (abi.SA_ERR_BAD_ARG, "observations", lambda: a.absorb_raw(ok_ids, [rng.uniform(-1, 1, (K + 1, D)).astype(f32), ok[1]], 1, 0.5)),
            (abi.SA_ERR_BAD_ARG, "topn", lambda: a.absorb_raw(ok_ids, ok, 0, 0.5)),
            (abi.SA_ERR_UNSUPPORTED, "topn", lambda: a.absorb_raw(ok_ids, ok, 65, 0.5)),
            (abi.SA_ERR_BAD_ARG, "NaN", lambda: a.absorb_raw(ok_ids, ok, 1, math.nan)),
            (abi.SA_ERR_BAD_ARG, "capacity", lambda: a.absorb_raw(ok_ids, ok, 1, 0.5, capacity=[1, 0])),
            (abi.SA_ERR_BAD_ARG, "capacity", lambda: a.absorb_raw(ok_ids, ok, 1, 0.5, capacity=[K + 1, 1])),
            (abi.SA_ERR_BAD_ARG, "NaN quality", lambda: a.absorb_raw(ok_ids, ok, 1, 0.5, quality=nan_q)),
            (abi.SA_ERR_BAD_ARG, "q_attrs without a rule", lambda: a.absorb_raw(ok_ids, ok, 1, 0.5, attrs=qa)),
            (abi.SA_ERR_BAD_ARG, "null argument", lambda: a.absorb_raw(ok_ids, ok, 1, 0.5, compat=rule)),     # a rule without q_attrs
            (abi.SA_ERR_BAD_ARG, "starts after", lambda: a.absorb_raw(ok_ids, ok, 1, 0.5, compat=rule, attrs=AT.pack_attrs([0, 1], [9, 0], [5, 5]))),
            (abi.SA_ERR_BAD_ARG, "unknown rule bits", lambda: a.absorb_raw(ok_ids, ok, 1, 0.5, compat=AT.Compat(0x100), attrs=qa)),
            (abi.SA_ERR_BAD_ARG, "null rows", lambda: a.absorb_rows_raw(ok_ids, [2, 1], None, 1, 0.5)),
        ]
        for code, word, call in cases:
            with pytest.raises(EngineError) as ex:
                call()
            assert ex.value.code == code and word in str(ex.value), (word, ex.value.code, str(ex.value))
            assert state(a) == before, word
            assert a.absorb_stats()["launches"] == 0
        # null out_dest, null q_feats with observations: through the C call itself
        from similari_amd.search import _p, pack_tracks, sa_topn_params

        prm = sa_topn_params(1, 1, 0.5, math.inf)
        ids, n_obs, feats = pack_tracks(ok_ids, ok, D)
        out_n, win, wt, dest = np.zeros(2, u32), np.zeros((2, 1), u64), np.zeros((2, 1), np.float64), np.zeros(2, u64)
        for word, f, d in [("null argument", feats, None), ("null q_feats", None, dest)]:
            rc = a.lib.sa_store_absorb(a.h, C.byref(prm), None, 2, _p(ids, C.c_uint64), _p(n_obs, C.c_uint32), _p(f, C.c_float), None, None, None,
                                       _p(out_n, C.c_uint32), _p(win, C.c_uint64), None, _p(wt, C.c_double), _p(d, C.c_uint64))
            assert rc == abi.SA_ERR_BAD_ARG and word in a.lib.sa_last_error(a.engine.h).decode(), word
            assert state(a) == before, word
        # the next valid call succeeds
        res, dest = a.absorb(ok_ids, ok, 1, -2.0)   # below every similarity: nothing is kept
        assert res == {} and dest == {50: 50, 51: 51} and len(a) == T + 2
    finally:
        a.close()
