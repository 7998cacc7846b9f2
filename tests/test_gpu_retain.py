"""A frame's tracks absorbed under "keep the best" on the MI355X (similari_amd.retain.RetainStore over include/similari_retain.h).

The contract admits no tolerance: sa_store_absorb_keep returns, and leaves in the store, exactly the bits of search_bestfit followed by
append(keep) (and set_attrs under a rule).  So every case runs twin stores in one engine — A through absorb_keep, B through the two
calls, whose kernels this feature does not touch — and compares after every step what tests/test_gpu_absorb.py compares: the outputs,
order(), fetch_raw rows and qualities as uint32, the attributes, and a tapped search of both stores bit for bit.  fetch reads the
qualities from the host's table; what the step wrote into the device's mirror shows in the next keep-best frame, which ranks by it —
every sequence here therefore runs at least two such frames in a row, the second one without an upload.

Shapes are the smallest at which the step can go wrong: D in {5, 33, 64}, K in {1, 3, 5} (Kp = 1, 4, 8), K = 32 for the full wave,
rows of 65 to 256 pieces for the second pass of a lane, 5 to 1025 queries against 700 tracks for the second wave, workgroup and scan chunk."""
import math

import numpy as np
import pytest

import absorb_cases as AC
import merge_ref as M
import test_gpu_absorb as TA
from similari_amd import abi, attrs as AT
from similari_amd.devrows import DeviceRows
from similari_amd.engine import Engine, EngineError
from similari_amd.f16 import SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_F32
from similari_amd.merge import SA_KEEP_BEST, SA_KEEP_LATEST
from similari_amd.retain import RetainStore

pytestmark = pytest.mark.gpu
u16, u32, u64, f32 = np.uint16, np.uint32, np.uint64, np.float32
F32, BF16, F16 = SA_ELEM_F32, SA_ELEM_BF16, SA_ELEM_F16
NAME = TA.NAME
FAR, CUT = TA.FAR, TA.CUT
INF = f32(np.inf)


@pytest.fixture(scope="module")
def engine():
    eng = Engine(abi.make_config(device=0))
    yield eng
    eng.close()


# ---- the two routes ------------------------------------------------------------------------------
def step(rng, a, b, q_ids, feats, topn, cut, quality=None, capacity=None, rule=None, q_attrs=None, keep="best"):
    """One frame through both routes, everything compared; -> (dest, retain_stats with the search's reruns and groups)."""
    q_ids = np.asarray(q_ids, u64)
    got = a.absorb_keep_raw(q_ids, feats, topn, cut, keep, 1, math.inf, quality, capacity, rule, q_attrs)
    st = dict(a.retain_stats(), reruns=a.last_stats()["reruns"], groups=a.last_stats()["groups"])
    out_n, win, trk, wt, _ = b.search_bestfit_raw(q_ids, feats, topn, cut, 1, math.inf, compat=rule, q_attrs=q_attrs)
    dest = TA.dest_of(q_ids, out_n, win)
    b.append(dest, feats, quality, keep, capacity)
    if rule is not None and len(q_ids):
        b.set_attrs_raw(dest, TA.union_attrs(b, dest, q_ids, q_attrs))
    TA.same_out(got, (out_n, win, trk, wt, dest))
    TA.same_stores(rng, a, b, rule)
    assert st["matched"] + st["created"] == len(q_ids) and st["matched"] == int((dest != q_ids).sum())
    assert st["keep"] == {"latest": SA_KEEP_LATEST, "best": SA_KEEP_BEST}[keep]
    absorb = a.absorb_stats()
    assert all(st[k] == absorb[k] for k in absorb)   # the fields of sa_absorb_stats are those of the same call
    return dest, st


def twin(engine, kind, D, K, elem, ids=None, banks=None, quality=None):
    """Twin stores holding the banks in the given order with the given qualities (appended under "latest", which keeps that order)."""
    a, b = RetainStore(engine, kind, D, K, elem), RetainStore(engine, kind, D, K, elem)
    if ids is not None:
        for s in (a, b):
            if quality is None:
                s.upsert(ids, banks)
            else:
                s.append(ids, banks, quality, "latest")
    return a, b


def random_twin(engine, kind, D, K, elem, T, rng):
    ids, banks = AC.banks(rng, T, K, D)
    return twin(engine, kind, D, K, elem, ids, banks, [rng.uniform(0, 1, len(x)).astype(f32) for x in banks])


def kp(K):
    """a bank's padded length: the power of two at or above K"""
    return 1 << (int(K) - 1).bit_length()


def small_case():
    """absorb_cases.wave_case's store (700 ragged banks, f32 euclidean, D = 33, K = 2) with a frame of five queries: the fifth is the
    second workgroup's first wave.  Slots from both ends of the store; the last query is matched."""
    rng = np.random.default_rng(7005)
    ids, bk = AC.banks(rng, 700, 2, 33)
    case = AC.start(rng, AC.ELEM_F32, "euclidean", 33, 2, ids, bk)
    return AC.finish(rng, case, [699, None, 2, None, 350], [1, 2, 2, 0, 2], np.arange(10000, 10005, dtype=u64), np.array([2, 1, 1, 2, 2], u32))


def bank_quality(s, t):
    return [float(x) for x in s.fetch([t])[int(t)][1]]


# ---- 1. five consecutive frames, every store type and shape -------------------------------------
@pytest.mark.parametrize("D,K", TA.SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("elem,kind", TA.STORES, ids=lambda v: NAME.get(v, v) if isinstance(v, int) else v)
def test_five_frames_leave_the_bits_of_search_then_append_best(engine, elem, kind, D, K):
    """Banks with random qualities in bank order (unsorted), then five frames.  Capacities: NULL, NULL, 2 (< n0 for a full bank: the
    zeroed tail), 1, one per query.  Qualities: uniform, and in frame 1 drawn from three values, so ties between old and new rows
    decide.  Every frame has matched queries, two queries built on one stored track, a query far from everything, one without
    observations and a full-length query into a bank.  The mirror goes up in frame 0 alone."""
    rng = np.random.default_rng(1000 + 100 * elem + 10 * K + (kind == "cosine"))
    a, b = random_twin(engine, kind, D, K, elem, 6, rng)
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
            feats = TA.queries_on(rng, a, on, n_obs)
            if frame == 1:
                quality = [rng.choice([0.25, 0.5, 0.75], int(m)).astype(f32) for m in n_obs]
            else:
                quality = [rng.uniform(0, 1, int(m)).astype(f32) for m in n_obs]
            capacity = rng.integers(1, K + 1, Q).astype(u32) if cap == "mixed" else cap
            T0 = len(a)
            dest, st = step(rng, a, b, q_ids, feats, 2, CUT[kind], quality, capacity)
            assert st["launches"] == 3 and st["host_waits"] == 2 and st["reruns"] == 0
            assert st["qual_upload_bytes"] == (T0 * kp(a.K) * 4 if frame == 0 else 0)
            if Q > 1:
                assert st["matched"] >= 1 and st["created"] >= 1
            for t in a.order():   # whatever a frame touched lies in quality order; the rest was appended under "latest"
                q = bank_quality(a, t)
                if int(t) >= 1000 or int(t) in {int(d) for d, m in zip(dest, n_obs) if m}:
                    assert q == sorted(q, reverse=True), (int(t), q)
    finally:
        a.close()
        b.close()


# ---- 2. the permutation's corners ----------------------------------------------------------------
def test_the_corners_of_the_permutation(engine):
    """One frame, K = 5 (Kp = 8), every query on its own stored track:
        1  bank ascending, one new row below all of it at capacity 5: the bank is reversed in place, the new row is dropped;
        2  every new row better than every old one;  3  every new row worse: an unsorted bank is only reordered;
        4  all qualities equal: the stable order stays, the last new row is dropped;  5  -0.0 against 0.0: equal, the same;
        6  +inf and -inf on both sides;  7  a full bank at capacity 2: it shrinks and its tail is zeroed;
        8  named by a query without rows: no vote, the query becomes an empty track and the unsorted bank stays unsorted;
        then created tracks: K unsorted rows at capacity 3 (sorted and cut), one row, none.
    Held against the twin, the host model (tests/merge_ref.py) and, for the plain cases, the order written out here."""
    rng = np.random.default_rng(21)
    D, K = 33, 5
    bank_q = {1: [0.1, 0.2, 0.3, 0.4, 0.5], 2: [0.5, 0.4, 0.3], 3: [0.3, 0.5, 0.4], 4: [0.5] * 4, 5: [0.0, -0.0, 0.0],
              6: [INF, 1.0, -INF], 7: [0.9, 0.1, 0.8, 0.2, 0.7], 8: [0.1, 0.9, 0.5]}
    new_q = {1: [0.05], 2: [0.9, 0.8], 3: [0.1, 0.05], 4: [0.5, 0.5], 5: [-0.0, 0.0], 6: [-INF, INF], 7: [0.5], 8: []}
    cap = {1: 5, 2: 5, 3: 3, 4: 5, 5: 4, 6: 5, 7: 2, 8: 5}
    ids = np.arange(1, 9, dtype=u64)
    banks = [rng.uniform(-1, 1, (len(bank_q[int(t)]), D)).astype(f32) for t in ids]
    quality = [np.array(bank_q[int(t)], f32) for t in ids]
    a, b = twin(engine, "euclidean", D, K, F32, ids, banks, quality)
    try:
        model = M.Model(K, D)
        model.append(ids, banks, quality, M.LATEST)
        TA.holds(a, model)
        on = list(range(1, 9)) + [None, None, None]
        n_obs = [len(new_q[t]) for t in range(1, 9)] + [K, 1, 0]
        q_ids = np.arange(101, 112, dtype=u64)
        host = {int(t): x for t, x in zip(ids, banks)}
        feats, expected = AC.frame(rng, host, on, n_obs, "euclidean", q_ids=q_ids)
        q_quality = [np.array(new_q[t], f32) for t in range(1, 9)] + [np.array([0.2, 0.9, 0.2, 0.6, 0.9], f32), np.array([0.3], f32), np.zeros(0, f32)]
        capacity = np.array([cap[t] for t in range(1, 9)] + [3, 5, 5], u32)
        dest, st = step(rng, a, b, q_ids, feats, 1, CUT["euclidean"], q_quality, capacity)
        assert np.array_equal(dest, expected) and [int(d) for d in dest] == [1, 2, 3, 4, 5, 6, 7, 108, 109, 110, 111]
        model.append(dest, feats, q_quality, M.BEST, capacity)
        TA.holds(a, model)
        # the orders, written out
        old = {int(t): x for t, x in zip(ids, banks)}
        got = {t: a.fetch([t])[t] for t in list(range(1, 9)) + [108, 109, 110, 111]}
        assert np.array_equal(got[1][0], old[1][::-1]) and got[1][1].tolist() == [f32(x) for x in (0.5, 0.4, 0.3, 0.2, 0.1)]
        assert np.array_equal(got[2][0], np.concatenate([feats[1], old[2]]))
        assert np.array_equal(got[3][0], old[3][[1, 2, 0]])
        assert np.array_equal(got[4][0], np.concatenate([old[4], feats[3][:1]]))
        assert np.array_equal(got[5][0], np.concatenate([old[5], feats[4][:1]]))
        assert got[5][1].view(u32).tolist() == np.array([0.0, -0.0, 0.0, -0.0], f32).view(u32).tolist()   # each zero keeps its sign
        assert np.array_equal(got[6][0], np.stack([old[6][0], feats[5][1], old[6][1], old[6][2], feats[5][0]]))
        assert np.array_equal(got[7][0], old[7][[0, 2]])
        assert np.array_equal(got[8][0], old[8]) and got[8][1].tolist() == [f32(x) for x in (0.1, 0.9, 0.5)]
        assert len(got[108][0]) == 0 and len(got[111][0]) == 0
        assert np.array_equal(got[109][0], feats[8][[1, 4, 3]]) and len(got[110][0]) == 1
        n_raw, f_raw, q_raw = a.fetch_raw([7])
        assert n_raw[0] == 2 and not f_raw[0, 2:].any() and not q_raw[0, 2:].view(u32).any()
        # a second frame ranks by what the step wrote into the mirror: all eight tracks again, nothing uploaded
        q2 = np.arange(201, 209, dtype=u64)
        host = {t: got[t][0] for t in range(1, 9)}
        feats2, _ = AC.frame(rng, host, list(range(1, 9)), [2] * 8, "euclidean", q_ids=q2)
        quality2 = [rng.choice([0.0, 0.3, 0.5, 0.95], 2).astype(f32) for _ in range(8)]
        dest, st = step(rng, a, b, q2, feats2, 1, CUT["euclidean"], quality2, 4)
        assert [int(d) for d in dest] == list(range(1, 9)) and st["qual_upload_bytes"] == 0
        model.append(dest, feats2, quality2, M.BEST, 4)
        TA.holds(a, model)
    finally:
        a.close()
        b.close()


def test_a_full_wave_32_stored_rows_and_32_new_ones(engine):
    """K = 32: a full bank and 32 new rows are 64 observations, one per lane, lane 63 included; a bank of 20 takes 32 (52 lanes) and
    a created track sorts its own 32.  Qualities are drawn from eight values, so ties run across the old and the new rows.  Two
    frames: the second ranks by the mirror."""
    rng = np.random.default_rng(22)
    D, K = 33, 32
    ids = np.array([1, 2, 3], u64)
    banks = [rng.uniform(-1, 1, (m, D)).astype(f32) for m in (32, 20, 32)]
    levels = np.linspace(0, 1, 8).astype(f32)
    quality = [rng.choice(levels, len(x)).astype(f32) for x in banks]
    a, b = twin(engine, "euclidean", D, K, F32, ids, banks, quality)
    try:
        model = M.Model(K, D)
        model.append(ids, banks, quality, M.LATEST)
        for frame in range(2):
            host = {t: a.fetch([t])[t][0] for t in (1, 2, 3)}
            q_ids = np.arange(100 + 10 * frame, 104 + 10 * frame, dtype=u64)
            feats, expected = AC.frame(rng, host, [1, 2, None, 3], [32, 32, 32, 1], "euclidean", q_ids=q_ids)
            q_quality = [rng.choice(levels, len(x)).astype(f32) for x in feats]
            dest, st = step(rng, a, b, q_ids, feats, 1, CUT["euclidean"], q_quality, None if frame == 0 else [32, 7, 32, 31])
            assert np.array_equal(dest, expected) and st["matched"] == 3 and st["launches"] == 3
            assert (st["qual_upload_bytes"] == 0) == (frame == 1)
            model.append(dest, feats, q_quality, M.BEST, None if frame == 0 else [32, 7, 32, 31])
            TA.holds(a, model)
        assert [len(a.fetch([t])[t][0]) for t in (1, 2, 3)] == [32, 7, 31]
    finally:
        a.close()
        b.close()


# ---- 3. rows beyond one pass of the wave ---------------------------------------------------------
@pytest.mark.parametrize("elem,kind,D", AC.WIDE_FORMS, ids=lambda v: NAME.get(v, v) if isinstance(v, int) and v < 3 else str(v))
def test_banks_permute_in_place_at_widths_beyond_one_pass(engine, elem, kind, D):
    """f32 at D = 260 (65 pieces + padding: the second pass is a few lanes alone) and 1024, f16 at 1024, bf16 at 520.  K = 5: a full
    ascending bank is reversed in place (every row but the middle one crosses another), an unsorted one takes two rows in between
    its own, one shrinks to two, a created track sorts five rows — a row torn between two passes of a lane, or read after it was
    overwritten, differs from the twin, whose rows go through staging."""
    rng = np.random.default_rng(8100 + 10 * D + elem)
    K = 5
    ids = np.arange(1, 5, dtype=u64)
    banks = [rng.uniform(-1, 1, (m, D)).astype(f32) for m in (5, 3, 5, 2)]
    quality = [np.array(x, f32) for x in ([0.1, 0.2, 0.3, 0.4, 0.5], [0.3, 0.9, 0.6], [0.5, 0.1, 0.4, 0.2, 0.3], [0.7, 0.8])]
    a, b = twin(engine, kind, D, K, elem, ids, banks, quality)
    try:
        stored = {int(t): a.fetch([t])[int(t)][0] for t in ids}   # as the store rounds them
        q_ids = np.arange(50, 55, dtype=u64)
        feats = TA.queries_on(rng, a, [1, 2, 3, None, None], [1, 2, 1, 5, 0])
        q_quality = [np.array(x, f32) for x in ([0.05], [0.7, 0.4], [0.45], [0.2, 0.8, 0.4, 1.0, 0.6], [])]
        dest, st = step(rng, a, b, q_ids, feats, 1, CUT[kind], q_quality, [5, 5, 2, 5, 5])
        assert [int(d) for d in dest] == [1, 2, 3, 53, 54] and st["launches"] == 3 and st["reruns"] == 0
        got = {t: a.fetch([t])[t] for t in (1, 2, 3, 4, 53)}
        assert np.array_equal(got[1][0], stored[1][::-1])                                   # reversed, the new row dropped
        assert np.array_equal(got[2][0][[0, 2, 4]], stored[2][[1, 2, 0]])                   # 0.9 (0.7) 0.6 (0.4) 0.3
        assert got[2][1].tolist() == [f32(x) for x in (0.9, 0.7, 0.6, 0.4, 0.3)]
        assert np.array_equal(got[3][0][0], stored[3][0]) and got[3][1].tolist() == [f32(0.5), f32(0.45)]
        assert np.array_equal(got[4][0], stored[4])                                         # not named: as it was
        assert got[53][1].tolist() == [f32(x) for x in (1.0, 0.8, 0.6, 0.4, 0.2)]
        n_raw, f_raw, _ = a.fetch_raw([3])
        assert n_raw[0] == 2 and not f_raw[0, 2:].any()
        # again, by the mirror: the reversed bank takes rows into its middle
        feats = TA.queries_on(rng, a, [1, 53], [2, 2])
        dest, st = step(rng, a, b, [60, 61], feats, 1, CUT[kind], [np.array([0.35, 0.25], f32), np.array([0.9, 0.1], f32)], 5)
        assert [int(d) for d in dest] == [1, 53] and st["qual_upload_bytes"] == 0
        assert bank_quality(a, 1) == [float(f32(x)) for x in (0.5, 0.4, 0.35, 0.3, 0.25)]
    finally:
        a.close()
        b.close()


# ---- 4. frame sizes: the second wave, workgroup and scan chunk ------------------------------------
@pytest.mark.parametrize("Q,last", [(5, True), (64, None), (65, True), (1025, False)])
def test_frames_of_many_queries_against_700_tracks(engine, Q, last):
    """absorb_cases.wave_case (Q = 5: small_case above): 700 ragged banks of up to two rows, f32 euclidean, D = 33, K = 2, about
    three queries in ten on a stored track.  Before the frame every stored track of one row takes a second one with a random quality (under "latest": the bank
    is then (0, q), unsorted), so old and new rows interleave.  Held against the twin and against the plain host model."""
    case = small_case() if Q == 5 else AC.wave_case(Q, last)
    rng = case["rng"]
    a, b = twin(engine, case["kind"], case["D"], case["K"], case["elem"], case["ids"], case["banks"])
    try:
        model = case["model"]
        single = [int(t) for t in case["ids"] if len(model.banks[int(t)]) == 1]
        extra = [rng.uniform(-1, 1, (1, case["D"])).astype(f32) for _ in single]
        extra_q = [rng.uniform(0, 1, 1).astype(f32) for _ in single]
        for s in (a, b):
            s.append(single, extra, extra_q, "latest")
        model.append(single, extra, extra_q, M.LATEST)
        TA.holds(a, model)
        dest, st = step(rng, a, b, case["q_ids"], case["feats"], 2, CUT[case["kind"]], case["quality"], case["capacity"])
        assert np.array_equal(dest, case["expected_dest"])
        assert st["launches"] == 3 and st["qual_upload_bytes"] == 700 * kp(a.K) * 4
        model.append(dest, case["feats"], case["quality"], M.BEST, case["capacity"])
        TA.holds(a, model)
        if last is not None:
            assert bool(dest[-1] != case["q_ids"][-1]) == last
        # a second, small frame on tracks the first one touched and created: ranked by the mirror
        touched = [int(d) for d, q, m in zip(dest, case["q_ids"], case["n_obs"]) if m][:6]
        feats = TA.queries_on(rng, a, touched, [2] * len(touched))
        quality = [rng.uniform(0, 1, 2).astype(f32) for _ in touched]
        q2 = np.arange(50000, 50000 + len(touched), dtype=u64)
        dest2, st = step(rng, a, b, q2, feats, 1, CUT[case["kind"]], quality)
        assert [int(d) for d in dest2] == touched and st["qual_upload_bytes"] == 0
        model.append(dest2, feats, quality, M.BEST)
        TA.holds(a, model)
    finally:
        a.close()
        b.close()


# ---- 5. the mirror ------------------------------------------------------------------------------
def test_every_writer_of_the_quality_table_marks_the_mirror(engine):
    """A keep-best absorb right after another uploads nothing.  After each other call that writes the host's quality table — append
    under either rule, merge, remove, upsert, an absorb under "latest", a reservation that reallocates — the next one uploads the
    whole table (T * Kp * 4 bytes) and still equals the twin; the one after it uploads nothing again."""
    rng = np.random.default_rng(31)
    D, K = 33, 3
    a, b = random_twin(engine, "cosine", D, K, F16, 12, rng)
    try:
        next_id = [500]

        def frame(expect_upload):
            stored = [int(i) for i in a.order()]
            on = [stored[0], None, stored[3], stored[len(stored) // 2]]
            n_obs = [2, 3, 1, 3]
            q_ids = np.arange(next_id[0], next_id[0] + 4, dtype=u64)
            next_id[0] += 4
            T0 = len(a)
            quality = [rng.uniform(0, 1, m).astype(f32) for m in n_obs]
            dest, st = step(rng, a, b, q_ids, TA.queries_on(rng, a, on, n_obs), 1, CUT["cosine"], quality, 3)
            assert st["qual_upload_bytes"] == (T0 * kp(a.K) * 4 if expect_upload else 0), st
            assert st["matched"] == 3

        def both(f):
            for s in (a, b):
                f(s)

        row = lambda n=1: rng.uniform(-1, 1, (n, D)).astype(f32)
        frame(True)
        frame(False)
        x, q = [row(2)], [np.array([0.9, 0.2], f32)]
        both(lambda s: s.append([2], x, q, "best", 3))
        frame(True)
        frame(False)
        both(lambda s: s.append([3], x, q, "latest", 3))
        frame(True)
        frame(False)
        both(lambda s: s.merge({5: [6]}, "best", 3))
        frame(True)
        frame(False)
        both(lambda s: s.remove([7]))
        frame(True)
        frame(False)
        y = [row(3)]
        both(lambda s: s.upsert([8], y))
        frame(True)
        frame(False)
        stored = [int(i) for i in a.order()]
        latest_q = TA.queries_on(rng, a, [stored[1], None], [2, 1])
        for s in (a, b):
            s.absorb_raw([900, 901], latest_q, 1, CUT["cosine"], quality=[np.array([0.3, 0.6], f32), np.array([0.1], f32)], capacity=3)
        TA.same_stores(rng, a, b)
        frame(True)
        frame(False)
        # the device arrays hold 64 tracks: this frame's T + n_queries goes past them, the reservation reallocates ahead of the step
        T0 = len(a)
        assert T0 < 64
        n = 66 - T0
        q_ids = np.arange(2000, 2000 + n, dtype=u64)
        stored = [int(i) for i in a.order()]
        on = [stored[0], stored[2]] + [None] * (n - 2)
        n_obs = [2, 1] + [int(m) for m in rng.integers(0, K + 1, n - 2)]
        quality = [rng.uniform(0, 1, m).astype(f32) for m in n_obs]
        dest, st = step(rng, a, b, q_ids, TA.queries_on(rng, a, on, n_obs), 1, CUT["cosine"], quality, 3)
        assert st["qual_upload_bytes"] == T0 * kp(a.K) * 4 and st["created"] == n - 2 and len(a) == T0 + n - 2 >= 64
        frame(False)
    finally:
        a.close()
        b.close()


def test_keep_latest_through_the_new_entry_point_is_absorb(engine):
    rng = np.random.default_rng(32)
    D, K = 33, 3
    a, b = random_twin(engine, "euclidean", D, K, F32, 10, rng)
    try:
        for frame in range(2):
            stored = [int(i) for i in a.order()]
            on, n_obs = [stored[0], None, stored[4], stored[5], None], [3, 2, 1, 2, 0]
            q_ids = np.arange(300 + 10 * frame, 305 + 10 * frame, dtype=u64)
            feats = TA.queries_on(rng, a, on, n_obs)
            quality = [rng.uniform(0, 1, m).astype(f32) for m in n_obs]
            got = a.absorb_keep_raw(q_ids, feats, 2, CUT["euclidean"], "latest", quality=quality, capacity=2)
            st, plain = a.retain_stats(), a.absorb_stats()
            want = b.absorb_raw(q_ids, feats, 2, CUT["euclidean"], quality=quality, capacity=2)
            TA.same_out(got, want)
            TA.same_stores(rng, a, b)
            other = b.absorb_stats()
            assert st["keep"] == SA_KEEP_LATEST and st["qual_upload_bytes"] == 0 and st["launches"] == other["launches"] == 3
            assert all(st[k] == plain[k] for k in plain)
            assert (st["matched"], st["created"], st["rows_moved"], st["host_waits"]) == tuple(other[k] for k in ("matched", "created", "rows_moved", "host_waits"))
        # the plain entry point reports through sa_store_retain_last as well
        assert b.retain_stats()["keep"] == SA_KEEP_LATEST and b.retain_stats()["launches"] == 3
    finally:
        a.close()
        b.close()


# ---- 6. edges, stats, reruns ---------------------------------------------------------------------
def test_an_empty_store_and_an_empty_frame(engine):
    rng = np.random.default_rng(33)
    D, K = 33, 3
    a, b = twin(engine, "euclidean", D, K, F32)
    try:
        q_ids = np.arange(10, 16, dtype=u64)
        n_obs = [1, 0, 3, 2, 3, 3]
        quality = [rng.uniform(0, 1, m).astype(f32) for m in n_obs]
        dest, st = step(rng, a, b, q_ids, TA.queries_on(rng, a, [None] * 6, n_obs), 2, CUT["euclidean"], quality, 2)
        assert np.array_equal(dest, q_ids) and st["created"] == 6 and st["launches"] == 2 and st["host_waits"] == 1
        assert st["qual_upload_bytes"] == 0   # nothing stored, nothing to upload
        assert list(a.fetch_raw(q_ids)[0]) == [1, 0, 2, 2, 2, 2]
        for t in q_ids:
            q = bank_quality(a, t)
            assert q == sorted(q, reverse=True)
        before = TA.state(a)
        dest, st = step(rng, a, b, np.zeros(0, u64), [], 2, CUT["euclidean"])
        assert TA.state(a) == before and st["launches"] == 0 and st["qual_upload_bytes"] == 0 and st["step_ms"] == 0.0
        # the created banks were written by the step, mirror included: matched next, without an upload
        dest, st = step(rng, a, b, [20, 21], TA.queries_on(rng, a, [12, 14], [2, 3]), 1, CUT["euclidean"],
                        [np.array([0.99, 0.01], f32), np.array([0.5, 0.5, 0.5], f32)])
        assert [int(d) for d in dest] == [12, 14] and st["qual_upload_bytes"] == 0 and st["launches"] == 3
    finally:
        a.close()
        b.close()


def test_launches_do_not_depend_on_the_number_of_queries(engine):
    """Q = 1 here; Q = 1025 is asserted in test_frames_of_many_queries_against_700_tracks."""
    rng = np.random.default_rng(34)
    D, K = 64, 5
    a, b = random_twin(engine, "cosine", D, K, BF16, 30, rng)
    try:
        stored = [int(i) for i in a.order()]
        _, one = step(rng, a, b, [700], TA.queries_on(rng, a, [stored[0]], [2]), 1, CUT["cosine"], [np.array([0.4, 0.6], f32)])
        on = [stored[k] if k % 2 else None for k in range(24)]
        n_obs = [1 + k % K for k in range(24)]
        _, many = step(rng, a, b, np.arange(800, 824, dtype=u64), TA.queries_on(rng, a, on, n_obs), 1, CUT["cosine"],
                       [rng.uniform(0, 1, m).astype(f32) for m in n_obs])
        assert one["launches"] == many["launches"] == 3 and one["host_waits"] == many["host_waits"] == 2
        assert one["matched"] == 1 and many["matched"] + many["created"] == 24 and one["step_ms"] > 0 and many["step_ms"] > 0
    finally:
        a.close()
        b.close()


def test_a_pool_rerun_applies_the_step_once(engine):
    """As tests/test_gpu_absorb.py: 24 x 21 groups outgrow a fresh pool, the search runs twice, the step rides behind the second run."""
    rng = np.random.default_rng(35)
    D, K, T, Q = 33, 3, 21, 24
    ids = np.arange(1, T + 1, dtype=u64)
    banks = [rng.uniform(-1, 1, (K, D)).astype(f32) for _ in range(T)]
    a, b = twin(engine, "euclidean", D, K, F16, ids, banks, [rng.uniform(0, 1, K).astype(f32) for _ in range(T)])
    try:
        feats = [rng.uniform(-1, 1, (K, D)).astype(f32) for _ in range(Q)]
        dest, st = step(rng, a, b, np.arange(500, 500 + Q, dtype=u64), feats, 3, FAR, [rng.uniform(0, 1, K).astype(f32) for _ in range(Q)], 2)
        assert st["groups"] == Q * T and st["reruns"] == 1 and st["launches"] == 3 and st["host_waits"] == 3
        assert st["matched"] >= 1 and st["created"] >= Q - T and st["qual_upload_bytes"] == T * kp(a.K) * 4
    finally:
        a.close()
        b.close()


def test_under_a_rule_matched_and_created_tracks_get_their_attributes(engine):
    rng = np.random.default_rng(36)
    D, K, T = 33, 3, 12
    a, b = random_twin(engine, "cosine", D, K, F32, T, rng)
    try:
        ids = np.arange(1, T + 1, dtype=u64)
        for s in (a, b):
            s.set_attrs(ids, ids % 3, np.arange(T) * 10, np.arange(T) * 10 + 5)
        rule = AT.compat(same_key=True, disjoint=True)
        on = [1, 2, 3, 4, None, 5]   # 0, 1: matched; 2: another key; 3: overlapping span; 4: far; 5: no observation
        n_obs = [2, 1, 1, 3, 1, 0]
        q_ids = np.arange(100, 106, dtype=u64)
        q_attrs = AT.pack_attrs([1, 2, 1, 1, 0, 2], [1000, 1000, 1000, 32, 1000, 1000], [1005, 1007, 1005, 40, 1001, 1001])
        quality = [rng.uniform(0, 1, m).astype(f32) for m in n_obs]
        dest, st = step(rng, a, b, q_ids, TA.queries_on(rng, a, on, n_obs), 2, CUT["cosine"], quality, 3, rule=rule, q_attrs=q_attrs)
        assert [int(d) for d in dest] == [1, 2, 102, 103, 104, 105]
        got = a.get_attrs(list(ids) + list(q_ids))
        assert got[1] == (1, 0, 1005) and got[2] == (2, 10, 1007) and got[3] == (0, 20, 25)
        assert got[102] == (1, 1000, 1005) and got[103] == (1, 32, 40) and got[104] == (0, 1000, 1001) and got[105] == (2, 1000, 1001)
        q_attrs = AT.pack_attrs([1, 2], [500, 2000], [600, 2001])
        dest, st = step(rng, a, b, [110, 111], TA.queries_on(rng, a, [1, 2], [1, 1]), 2, CUT["cosine"],
                        [np.array([0.5], f32), np.array([0.5], f32)], rule=rule, q_attrs=q_attrs)
        assert [int(d) for d in dest] == [110, 2] and st["qual_upload_bytes"] == 0
    finally:
        a.close()
        b.close()


# ---- 7. rows from device memory ------------------------------------------------------------------
def test_absorb_keep_rows_from_device_memory(engine):
    """Strided f16 rows gathered through an index into an f16 store: absorb_keep_rows against search_rows (BestFit) + append_rows."""
    rng = np.random.default_rng(37)
    D, K, T = 33, 3, 10
    a, b = random_twin(engine, "euclidean", D, K, F16, T, rng)
    try:
        next_id = 300
        for frame in range(2):
            stored = [int(i) for i in a.order()]
            on = [stored[0], stored[0], None, stored[3], stored[4], None, stored[5]]
            n_obs = np.array([1, 2, 3, 3, 1, 0, 2], u32)
            q_ids = np.arange(next_id, next_id + len(on), dtype=u64)
            next_id += len(on)
            total = int(n_obs.sum())
            rows = np.concatenate(TA.queries_on(rng, a, on, n_obs))
            index = rng.permutation(total + 2)[:total].astype(u32)
            bits = np.zeros((total + 2, D), u16)
            bits[index] = TA.to_bits(rows, F16)
            stride = D + 3
            img = np.full((total + 1) * stride + D, 0x7FFF, u16)   # NaN patterns between the rows
            for r in range(total + 2):
                img[r * stride: r * stride + D] = bits[r]
            quality = rng.uniform(0, 1, total).astype(f32)
            with TA.device_block(engine, img) as ptr:
                dr = DeviceRows(ptr, total + 2, stride, F16, index)
                got = a.absorb_keep_rows_raw(q_ids, n_obs, dr, 2, CUT["euclidean"], quality=quality, capacity=2)
                st = a.retain_stats()
                out_n, win, trk, wt, _ = b.search_rows_raw(q_ids, n_obs, dr, 2, CUT["euclidean"], vote="bestfit")
                dest = TA.dest_of(q_ids, out_n, win)
                b.append_rows(dest, n_obs, dr, quality, 2, "best")
            TA.same_out(got, (out_n, win, trk, wt, dest))
            TA.same_stores(rng, a, b)
            assert a.devrows_stats()["rows"] == total and st["matched"] >= 2 and st["created"] >= 2 and st["keep"] == SA_KEEP_BEST
            assert (st["qual_upload_bytes"] == 0) == (frame == 1)
    finally:
        a.close()
        b.close()


# ---- 8. refusals ---------------------------------------------------------------------------------
def test_refusals_leave_the_store_and_the_mirror_as_they_were(engine):
    rng = np.random.default_rng(38)
    D, K, T = 33, 3, 8
    a, b = random_twin(engine, "cosine", D, K, F32, T, rng)
    try:
        stored = [int(i) for i in a.order()]
        step(rng, a, b, [40, 41], TA.queries_on(rng, a, [stored[0], None], [2, 1]), 1, CUT["cosine"],
             [np.array([0.2, 0.7], f32), np.array([0.4], f32)])   # the mirror is valid from here on
        before = TA.state(a)
        ok_ids = np.array([50, 51], u64)
        ok = [rng.uniform(-1, 1, (2, D)).astype(f32), rng.uniform(-1, 1, (1, D)).astype(f32)]
        rule = AT.compat(same_key=True)
        qa = AT.pack_attrs([0, 1], [0, 0], [5, 5])
        nan_q = [np.array([0.5, np.nan], f32), np.array([0.5], f32)]
        k = a.absorb_keep_raw
        cases = [
            (abi.SA_ERR_BAD_ARG, "unknown keep", lambda: k(ok_ids, ok, 1, 0.5, 2)),
            (abi.SA_ERR_BAD_ARG, "unknown keep", lambda: k(np.zeros(0, u64), [], 1, 0.5, 7)),                  # ahead of n_queries == 0, as append
            (abi.SA_ERR_BAD_ARG, "stored", lambda: k([50, 3], ok, 1, 0.5)),                                    # a query id the store holds
            (abi.SA_ERR_BAD_ARG, "id 0", lambda: k([0, 51], ok, 1, 0.5)),
            (abi.SA_ERR_BAD_ARG, "twice", lambda: k([50, 50], ok, 1, 0.5)),
            (abi.SA_ERR_BAD_ARG, "observations", lambda: k(ok_ids, [rng.uniform(-1, 1, (K + 1, D)).astype(f32), ok[1]], 1, 0.5)),
            (abi.SA_ERR_BAD_ARG, "topn", lambda: k(ok_ids, ok, 0, 0.5)),
            (abi.SA_ERR_UNSUPPORTED, "topn", lambda: k(ok_ids, ok, 65, 0.5)),
            (abi.SA_ERR_BAD_ARG, "NaN", lambda: k(ok_ids, ok, 1, math.nan)),
            (abi.SA_ERR_BAD_ARG, "capacity", lambda: k(ok_ids, ok, 1, 0.5, capacity=[1, 0])),
            (abi.SA_ERR_BAD_ARG, "capacity", lambda: k(ok_ids, ok, 1, 0.5, capacity=[K + 1, 1])),
            (abi.SA_ERR_BAD_ARG, "NaN quality", lambda: k(ok_ids, ok, 1, 0.5, quality=nan_q)),
            (abi.SA_ERR_BAD_ARG, "q_attrs without a rule", lambda: k(ok_ids, ok, 1, 0.5, attrs=qa)),
            (abi.SA_ERR_BAD_ARG, "null argument", lambda: k(ok_ids, ok, 1, 0.5, compat=rule)),                 # a rule without q_attrs
            (abi.SA_ERR_BAD_ARG, "starts after", lambda: k(ok_ids, ok, 1, 0.5, compat=rule, attrs=AT.pack_attrs([0, 1], [9, 0], [5, 5]))),
            (abi.SA_ERR_BAD_ARG, "unknown rule bits", lambda: k(ok_ids, ok, 1, 0.5, compat=AT.Compat(0x100), attrs=qa)),
            (abi.SA_ERR_BAD_ARG, "null rows", lambda: a.absorb_keep_rows_raw(ok_ids, [2, 1], None, 1, 0.5)),
        ]
        zero = {"step_ms": 0.0, "matched": 0, "created": 0, "rows_moved": 0, "launches": 0, "host_waits": 0, "keep": 0, "qual_upload_bytes": 0}
        for code, word, call in cases:
            with pytest.raises(EngineError) as ex:
                call()
            assert ex.value.code == code and word in str(ex.value), (word, ex.value.code, str(ex.value))
            assert TA.state(a) == before, word
            assert a.retain_stats() == zero, word
        # null out_dest, null q_feats with observations: through the C call itself
        import ctypes as C

        from similari_amd.search import _p, pack_tracks, sa_topn_params

        prm = sa_topn_params(1, 1, 0.5, math.inf)
        ids, n_obs, feats = pack_tracks(ok_ids, ok, D)
        out_n, win, wt, dest = np.zeros(2, u32), np.zeros((2, 1), u64), np.zeros((2, 1), np.float64), np.zeros(2, u64)
        for word, f, d in [("null argument", feats, None), ("null q_feats", None, dest)]:
            rc = a.lib.sa_store_absorb_keep(a.h, SA_KEEP_BEST, C.byref(prm), None, 2, _p(ids, C.c_uint64), _p(n_obs, C.c_uint32), _p(f, C.c_float),
                                            None, None, None, _p(out_n, C.c_uint32), _p(win, C.c_uint64), None, _p(wt, C.c_double),
                                            _p(d, C.c_uint64))
            assert rc == abi.SA_ERR_BAD_ARG and word in a.lib.sa_last_error(a.engine.h).decode(), word
            assert TA.state(a) == before, word
        # the mirror is as it was — valid —, and the next frame equals the twin without an upload
        dest, st = step(rng, a, b, [60, 61, 62], TA.queries_on(rng, a, [stored[0], stored[1], None], [1, 2, 3]), 1, CUT["cosine"],
                        [np.array([0.5], f32), np.array([0.9, 0.1], f32), np.array([0.3, 0.2, 0.8], f32)], 3)
        assert [int(d) for d in dest[:2]] == stored[:2] and st["qual_upload_bytes"] == 0
    finally:
        a.close()
        b.close()
