"""f16 feature stores on the MI355X (similari_amd.f16.F16Store over include/similari_f16.h), for both metrics.

An f16 store is an f32 store fed with f16(x) for every feature value, contracted with f32 accumulation.  So every statement the suite
makes about an f32 store is made here against rounded rows (tests/f16_ref.py), with the tolerances the suite already has: none for
winners, weights, fetched rows and the three forms of a search; for a cell against f64 of the rounded rows the bounds of
test_gpu_search.assert_close — 1e-5 absolute for cosine, 1e-5 relative (floor 1e-30) for euclidean.  Products of f16 values are exact
in f32; what differs from f64 is the order of the f32 additions and, for euclidean, the cancellation of |a|^2 + |b|^2 - 2ab, which the
store answers by recomputing the cells it flags (d^2 < rho s) directly.  sa_store_expand_last proves which route a cell took."""
import math

import numpy as np
import pytest

import bestfit_ref as BF
import compat_ref as X
import f16_ref as F
import gallery_ref as G
import topn_ref as R
from similari_amd import abi, attrs as A
from similari_amd.bestfit import BestFitStore
from similari_amd.bf16 import Bf16Store
from similari_amd.engine import Engine, EngineError
from similari_amd.f16 import SA_ELEM_F16, SA_ELEM_F32, F16Store, expand_stats, store_info

pytestmark = pytest.mark.gpu
INF = math.inf
u32, u64 = np.uint32, np.uint64
KINDS = ["cosine", "euclidean"]


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


def jitter(rng, rows, rel):
    """rows plus a random vector of `rel` times each row's norm"""
    rows = np.asarray(rows, np.float32)
    d = rng.normal(0, 1, rows.shape)
    d *= (rel * np.linalg.norm(rows, axis=-1, keepdims=True)) / np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-30)
    return (rows + d).astype(np.float32)


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


def cell_error(kind, got, want):
    """got f32 cells, want f64 cells (same shape, same NaN pattern) -> the error per cell in the gate's measure: absolute for cosine,
    relative with the 1e-30 floor of tests/test_gpu_search.py for euclidean (NaN where want is)"""
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    err = np.abs(got.astype(np.float64) - want)
    return err if kind == "cosine" else err / np.maximum(np.abs(want), 1e-30)


def assert_cells(kind, got, want, tol=1e-5):
    err = cell_error(kind, got, want)
    worst = float(np.nanmax(err))
    print("%s: max error against f64 of the rounded rows = %.3g over %d cells" % (kind, worst, int((~np.isnan(want)).sum())))
    assert worst <= tol
    return worst


# ---- 1. fetch returns the rounded rows ------------------------------------------------------------------------------------------
def fetched_equal(store, ids, feats):
    n_obs, got, _ = store.fetch_raw(ids)
    for k, f in enumerate(feats):
        assert n_obs[k] == len(f)
        same_rows(got[k, : len(f)], F.round_f16(f))
        assert not got[k, len(f):].view(u32).any()   # unfilled rows: +0.0
    return n_obs, got


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [5, 33, 100])   # an odd length inside one 32-element chunk, one past it, one that ends inside the fourth
def test_fetch_returns_the_rounded_rows(engine, kind, D):
    rng = np.random.default_rng(300 + D)
    K, T = 3, 21
    ids = np.arange(1, T + 1)
    feats = bank(rng, T, K, D)
    feats[0] = (rng.normal(0, 100, (K, D))).astype(np.float32)                      # both signs, other binades
    feats[1] = rng.uniform(-6.2e-5, 6.2e-5, (K, D)).astype(np.float32)               # the f16 subnormal range
    feats[2] = np.array([[65504.0, 65519.0, 65520.0, -1e9, 2.0**-24] + [2.0**-25] * (D - 5)] * K, np.float32)   # the top, overflow to inf, the bottom
    store = F16Store(engine, kind, D, K)
    try:
        store.upsert(ids, feats)
        n_obs, got = fetched_equal(store, ids, feats)
        assert np.isinf(got[2, 0, 2]) and got[2, 0, 3] == -np.inf and got[2, 0, 4] == np.float32(2.0**-24) and got[1].any()
        store.upsert(ids, [got[k, : n_obs[k]] for k in range(T)])   # rounding is idempotent: feeding back changes no bit
        fetched_equal(store, ids, feats)
        more = [rng.uniform(0, 1, (1, D)).astype(np.float32) if len(f) < K else np.zeros((0, D), np.float32) for f in feats]
        store.append(ids, more)                                       # the append rounds as the upsert does
        fetched_equal(store, ids, [np.concatenate([f, m]) for f, m in zip(feats, more)])
        rep = [F.round_f16(f) for f in bank(rng, T, K, D, ragged=False)]   # f16-representable rows are stored without loss
        store.upsert(ids, rep)
        for k in range(T):
            same_rows(store.fetch_raw(ids)[1][k], rep[k])
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


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", [1, 3, 8, 32])
@pytest.mark.parametrize("D", [33, 100, 288])   # 2 and 4 chunks of 32: one guarded turn; 9: one steady turn, then 5 chunks in two guarded turns
def test_winners_equal_the_restatement_on_the_engines_cells(engine, kind, K, D):
    winners_case(engine, kind, K, D)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", RING_D)
def test_winners_equal_the_restatement_at_every_chunk_count_of_the_ring(engine, kind, D):
    winners_case(engine, kind, 3, D)


def winners_case(engine, kind, K, D):
    rng = np.random.default_rng(1000 * K + D + 1)
    T, Q = 37, 6   # ragged banks; 37 K stored rows and 6 K query rows cross both edges of the 64 x 64 tiles
    s_ids = rng.choice(np.arange(1, 500), T, replace=False)
    q_ids = np.concatenate([s_ids[:3], rng.choice(np.arange(500, 900), Q - 3, replace=False)])   # three queries are stored too
    store = F16Store(engine, kind, D, K)
    try:
        s_feats = bank(rng, T, K, D, zero_frac=0.15)
        s_feats[5] = rng.uniform(0.1, 1, (K, D)).astype(np.float32)
        store.upsert(s_ids, s_feats)
        q_feats = bank(rng, Q, K, D, zero_frac=0.15)
        q_feats[1] = np.zeros((0, D), np.float32)   # a query without observations: no pairs
        q_feats[4] = jitter(rng, s_feats[5], 1e-2)  # the twin of a stored track under another id: a whole group of near-duplicates
        _, cells, _ = check_exact(store, q_ids, q_feats, 5, INF)
        if kind == "euclidean":
            assert 0 < store.expand_stats()["cells"] < cells.size   # both routes fed the vote
        lo, mid = distance_quantile(cells, 0.05), distance_quantile(cells, 0.5)
        for topn, md, mv, kb in ((1, mid, 1, INF), (5, lo, 0, INF), (64, mid, 3, distance_quantile(cells, 0.9)), (64, INF, 1, INF),
                                 (5, mid, 1, distance_quantile(cells, 0.3))):
            check_exact(store, q_ids, q_feats, topn, md, mv, kb)
    finally:
        store.close()


# ---- 3. cells against f64 on the rounded inputs ---------------------------------------------------------------------------------
def tap_cells(engine, kind, K, D, s_feats, q_feats):
    """-> the tapped cells and the expansion's counters of that search"""
    store = F16Store(engine, kind, D, K)
    try:
        store.upsert(np.arange(1, len(s_feats) + 1), s_feats)
        cells = store.search_raw(np.arange(10**6, 10**6 + len(q_feats)), q_feats, 5, 0.5, tap=True)[3]
        return cells, store.expand_stats()
    finally:
        store.close()


def flag_bracket(q_feats, s_feats, K, D):
    """How many cells the expansion must, and may, have flagged: those whose d^2 / s (f64, rounded rows) lies below rho / 2, and below
    2 rho.  The engine evaluates d^2 / s in f32 with a relative error of some D eps, 1e-5 of rho at most, so a factor of two either
    way leaves no cell in doubt."""
    r = F.flag_ratio(F.round_banks(q_feats), F.round_banks(s_feats), K)
    rho = float(F.rho(D))
    return int((r < rho / 2).sum()), int((r < 2 * rho).sum())


@pytest.mark.parametrize("kind", KINDS)
# the smallest odd two-chunk row; four chunks; nine: the steady state and 5 chunks left; then every other count of RING_D
@pytest.mark.parametrize("K,D", [(2, 33), (3, 100), (4, 288)] + [(2 + n % 3, D) for n, D in enumerate(RING_D)])
def test_cells_against_f64_of_the_rounded_rows(engine, kind, K, D):
    rng = np.random.default_rng(K * 7 + D)
    s_feats = bank(rng, 9, K, D, zero_frac=0.1)
    s_feats[0] = rng.uniform(0.1, 1, (K, D)).astype(np.float32)
    s_feats[1] = rng.uniform(-1, 1, (K, D)).astype(np.float32)
    s_feats[2] = rng.uniform(-6.2e-5, 6.2e-5, (K, D)).astype(np.float32)   # every value in the f16 subnormal range
    s_feats[3] = np.zeros((K, D), np.float32)                               # zero rows that are present
    s_feats[3][0, ::3] = 3e-5                                               # and one of subnormals among zeros
    q_feats = bank(rng, 6, K, D, zero_frac=0.1)
    q_feats[0] = s_feats[0].copy()                                          # exact duplicates
    q_feats[1] = np.stack([jitter(rng, s_feats[1][k], rel) for k, rel in zip(range(K), (1e-3, 1e-2, 1e-1, 3e-2))])   # near-duplicates
    q_feats[2] = jitter(rng, s_feats[2], 1e-1)                              # near-duplicates among the subnormals
    q_feats[3] = np.zeros((K, D), np.float32)
    cells, st = tap_cells(engine, kind, K, D, s_feats, q_feats)
    want = F.cells_f64(kind, F.round_banks(q_feats), F.round_banks(s_feats), K)
    assert np.isfinite(want).any()
    assert_cells(kind, cells, want)
    if kind == "euclidean":
        for k in range(K):
            assert cells[0, k, 0, k].view(u32) == 0   # an exact duplicate pair: exactly +0.0
        assert not cells[3, :, 3, 1:].view(u32).any()   # zero row against zero row
        lo, hi = flag_bracket(q_feats, s_feats, K, D)
        print("flagged %d cells in %d tiles (between %d and %d expected) of %d" % (st["cells"], st["tiles"], lo, hi, cells.size))
        assert 0 < st["cells"] < cells.size and lo <= st["cells"] <= hi and st["tiles"] >= 1
        assert lo >= 3 * K   # each twin row and its original, at the least
    else:
        assert st == {"cells": 0, "tiles": 0}
        assert np.isfinite(cells[2, :, 2, :]).all() and (cells[2, :, 2, :] != 0).all()   # subnormal rows have a cosine: nothing was flushed


# ---- 4. the rho sweep -------------------------------------------------------------------------------------------------------------
def sweep_rows(rng, D, n):
    """One query row a and n stored rows whose d^2 / (|a|^2 + |b|^2) is spread geometrically from 1e-4 to 1: b = alpha a + beta v with
    v orthogonal to a and as long — alpha = 1, beta^2 = 2 r / (1 - r) up to r = 1/3, from there beta = 1 and alpha falls to 0."""
    a = np.abs(rng.normal(0, 1, D))
    a /= np.linalg.norm(a)
    r = np.geomspace(1e-4, 1.0, n)
    v = rng.normal(0, 1, (n, D))
    v -= (v @ a)[:, None] * a[None, :]
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    e = r - 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        alpha = np.where(r <= 1 / 3, 1.0, np.where(e < 0, (-1.0 + np.sqrt(np.maximum(1.0 - 2.0 * e * e, 0.0))) / e, 0.0))
    beta = np.where(r <= 1 / 3, np.sqrt(2 * r / (1 - np.minimum(r, 0.5))), 1.0)
    b = alpha[:, None] * a[None, :] + beta[:, None] * v
    return F.round_f16(a[None, :]), F.round_f16(b)


@pytest.mark.parametrize("D", [32, 512])   # one chunk; the re-ID width
def test_the_rho_sweep(engine, D):
    """2048 cells across the flag boundary, every one within 1e-5 relative: the unflagged side is the expansion at its worst
    cancellation (d^2 just above rho s), the flagged side the direct sum.  Measured on the MI355X (printed by the test),
    largest relative error on the flagged / the unflagged side: D = 32 (rho 0.0283) 7.9e-8 / 2.2e-6, D = 512 (rho 0.1131) 1.4e-7 / 1.1e-6;
    the unflagged maximum lies within a factor 2 above rho both times, and the engine flagged exactly the cells f64 puts below rho."""
    rng = np.random.default_rng(4000 + D)
    n = 2048
    a, b = sweep_rows(rng, D, n)
    store = F16Store(engine, "euclidean", D, 1)
    try:
        store.upsert(np.arange(1, n + 1), [row[None, :] for row in b])
        assert np.array_equal(store.order(), np.arange(1, n + 1))   # cell t is stored row t
        cells = store.search_raw([10**6], [a], 5, INF, tap=True)[3].reshape(n)
        st = store.expand_stats()
    finally:
        store.close()
    stored = [row[None, :] for row in b]
    ratio = F.flag_ratio([a], stored, 1).reshape(n)
    assert ratio.min() < 2e-4 and ratio.max() > 0.9 and np.all(np.diff(np.log(ratio)) < 0.2)   # the spread the sweep is about
    err = cell_error("euclidean", cells, F.cells_f64("euclidean", [a], stored, 1).reshape(n))
    rho = float(F.rho(D))
    below, above = ratio < rho, ratio >= rho
    print("D = %d, rho = %.4g: %d cells flagged by the engine (%d below rho in f64); max relative error %.3g flagged side, %.3g unflagged side,"
          " %.3g within a factor 2 above rho" % (D, rho, st["cells"], int(below.sum()), err[below].max(), err[above].max(),
                                                  err[above & (ratio < 2 * rho)].max()))
    assert abs(st["cells"] - int(below.sum())) <= 2 and 0 < st["cells"] < n   # the boundary lies where the rule puts it
    assert err.max() <= 1e-5


# ---- 5. a tile that flags everything ------------------------------------------------------------------------------------------------
def test_a_tile_that_flags_everything(engine):
    """64 near-identical rows against 64 (K = 32, D = 64: two query tracks, two stored tracks, one 64 x 64 tile): all 4096 cells are
    recomputed.  A second, far-away identity in the store adds a tile that recomputes nothing."""
    rng = np.random.default_rng(55)
    K, D = 32, 64
    base = rng.uniform(0.1, 1, D).astype(np.float32)
    near = lambda: jitter(rng, np.tile(base, (K, 1)), 1e-2)
    s_feats, q_feats = [near(), near()], [near(), near()]
    far = rng.uniform(0.1, 1, D).astype(np.float32)[::-1].copy()
    store = F16Store(engine, "euclidean", D, K)
    try:
        store.upsert([1, 2], s_feats)
        cells = store.search_raw([11, 12], q_feats, 5, INF, tap=True)[3]
        assert store.expand_stats() == {"cells": 4096, "tiles": 1}
        assert_cells("euclidean", cells, F.cells_f64("euclidean", F.round_banks(q_feats), F.round_banks(s_feats), K))
        s_feats += [jitter(rng, np.tile(far, (K, 1)), 1e-2) for _ in range(2)]
        store.upsert([3, 4], s_feats[2:])
        raw = store.search_raw([11, 12], q_feats, 5, INF, tap=True)
        assert store.expand_stats() == {"cells": 4096, "tiles": 1} and store.last_stats()["groups"] == 8   # of the two tiles that ran
        assert_cells("euclidean", raw[3], F.cells_f64("euclidean", F.round_banks(q_feats), F.round_banks(s_feats), K))
        j = store.join_raw(5, INF, tap=True)   # 128 x 128: three tiles on or above the diagonal, two of them all twins
        st = store.expand_stats()
        assert st["tiles"] == 2 and st["cells"] == 2 * 4096
        assert_cells("euclidean", j[3], F.cells_f64("euclidean", F.round_banks(s_feats), F.round_banks(s_feats), K))
    finally:
        store.close()


# ---- 6. join == stored == host-fed ----------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("kind", KINDS)
def test_join_equals_stored_equals_host_fed(engine, kind):
    T, K, D = 37, 3, 100   # 111 rows: two tile columns, the second ragged; a four-chunk row
    rng = np.random.default_rng(100000 * T + 1000 * K + D)
    ids = rng.choice(np.arange(1, 5000), T, replace=False)
    feats = bank(rng, T, K, D, zero_frac=0.15)
    feats[1] = np.zeros((0, D), np.float32)
    feats[0], feats[2] = (rng.uniform(0.1, 1, (K, D)).astype(np.float32) for _ in range(2))
    feats[30] = feats[0].copy()                 # an exact twin, in the other tile column
    feats[7] = jitter(rng, feats[2], 1e-2)      # a near twin, in the same tile
    feats[33] = jitter(rng, feats[2], 1e-3)     # and one across
    store = F16Store(engine, kind, D, K)
    try:
        store.upsert(ids, feats)
        order = store.order()
        assert np.array_equal(order, ids)   # slot t holds feats[t]
        cells = three_ways(store, 5, INF)[3]
        assert cells.shape == (T, K, T, K)
        if kind == "euclidean":
            st = store.expand_stats()
            assert 3 * K <= st["cells"] < cells.size   # each twin row and its original, at the least
            assert not cells[0, :, 30, :][np.eye(K, dtype=bool)].view(u32).any()   # the exact twin: +0.0
        flat = cells.reshape(T * K, T * K)
        m = ~np.isnan(flat)
        assert np.array_equal(m, m.T) and np.array_equal(flat[m].view(u32), flat.T[m].view(u32))   # symmetric to the bit
        assert_cells(kind, cells, F.cells_f64(kind, F.round_banks(feats), F.round_banks(feats), K))
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


# ---- 7. a search after append + merge returns the bits of a freshly upserted store ---------------------------------------------
def check_against_fresh(engine, kind, store, model, rng):
    assert [int(i) for i in store.order()] == model.order
    n_obs, feats, qual = store.fetch_raw(model.order)
    for k, i in enumerate(model.order):
        m = len(model.feats(i))
        assert n_obs[k] == m
        same_rows(feats[k, :m], model.feats(i))
        assert np.array_equal(qual[k, :m].view(u32), model.quality(i).view(u32))
    q_ids = [10**6 + k for k in range(4)] + model.order[:2]
    q_feats = [rng.uniform(0, 1, (int(rng.integers(0, model.K + 1)), model.D)).astype(np.float32) - np.float32(0.5) for _ in q_ids]
    q_feats[3] = model.feats(model.order[4])[:1].copy()   # a stored row as a query: the flagged route, in both stores
    ref = F16Store(engine, kind, model.D, model.K)
    try:
        ref.upsert(model.order, [model.feats(i) for i in model.order])
        a = store.search_raw(q_ids, q_feats, 5, INF, tap=True)
        same_bits(a, ref.search_raw(q_ids, q_feats, 5, INF, tap=True))
        assert store.expand_stats() == ref.expand_stats()
        md = distance_quantile(a[3], 0.3)
        same_bits(store.search_raw(q_ids, q_feats, 64, md, 2, tap=True), ref.search_raw(q_ids, q_feats, 64, md, 2, tap=True))
        assert a[0].any()
    finally:
        ref.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("keep", ["latest", "best"])
def test_append_and_merge_leave_what_a_fresh_store_holds(engine, kind, keep):
    rng = np.random.default_rng(77 + (keep == "best"))
    K, D, T = 4, 100, 20
    store, model = F16Store(engine, kind, D, K), F.Model(K, D)
    try:
        ids = list(range(1, T + 1))
        feats = [rng.uniform(0, 1, (int(rng.integers(2, K + 1)), D)).astype(np.float32) - np.float32(0.5) for _ in ids]
        qual = [rng.integers(0, 4, len(f)).astype(np.float32) for f in feats]
        for m in (store, model):
            m.append(ids, feats, qual, keep=keep)
        check_against_fresh(engine, kind, store, model, rng)
        more = [rng.uniform(0, 1, (int(rng.integers(0, K + 1)), D)).astype(np.float32) - np.float32(0.5) for _ in ids[:8]]
        mq = [rng.integers(0, 4, len(f)).astype(np.float32) for f in more]
        new = rng.uniform(0, 1, (1, D)).astype(np.float32)
        for m in (store, model):   # known ids (some get no row) and a new one, under a capacity below K
            m.append(ids[:8] + [100], more + [new], mq + [np.ones(1, np.float32)], keep=keep, capacity=3)
        check_against_fresh(engine, kind, store, model, rng)
        pairs = {2: [19, 7], 11: [3], 5: []}
        merged = sum(len(model.feats(i)) for i in (2, 19, 7))
        assert merged > 3   # a capacity below the merged count: the rule drops rows
        for m in (store, model):
            m.merge(pairs, keep=keep, capacity={2: 3, 11: 2, 5: 1})
        assert store.merge_stats()["tracks_moved"] > 0
        check_against_fresh(engine, kind, store, model, rng)
    finally:
        store.close()


# ---- 8. compat and BestFit -------------------------------------------------------------------------------------------------------
def attr_case(engine, kind, seed):
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
    store = F16Store(engine, kind, D, K)
    store.upsert(ids, feats)
    store.set_attrs_raw(ids, packed(s_attrs))
    return store, ids, s_attrs, q_ids, q_feats, q_attrs, packed


@pytest.mark.parametrize("kind", KINDS)
def test_compat_on_an_f16_store(engine, kind):
    store, ids, s_attrs, q_ids, q_feats, q_attrs, packed = attr_case(engine, kind, 61)
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


@pytest.mark.parametrize("kind", KINDS)
def test_bestfit_on_an_f16_store(engine, kind):
    store, ids, s_attrs, q_ids, q_feats, q_attrs, packed = attr_case(engine, kind, 62)
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


# ---- 9. an f32 store and an f16 store fed f16-representable rows ---------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_an_f32_and_an_f16_store_fed_f16_rows(engine, kind):
    """Both stores then hold the same values, so both are held against the same f64 cells with the gate's tolerance, and against
    each other with twice that.  The f16 store keeps the rows in exactly half the bytes."""
    rng = np.random.default_rng(81)
    K, D, T, Q = 3, 100, 70, 6   # past the first capacity of 64
    ids, feats = np.arange(1, T + 1), F.round_banks(bank(rng, T, K, D))
    q_ids, q_feats = np.arange(1000, 1000 + Q), F.round_banks(bank(rng, Q, K, D, ragged=False))
    q_feats[2] = F.round_f16(jitter(rng, np.concatenate([feats[4], np.ones((K, D), np.float32)])[:K], 1e-2))   # near-duplicates for both routes
    f32, h16 = BestFitStore(engine, kind, D, K), F16Store(engine, kind, D, K)
    try:
        for s in (f32, h16):
            s.upsert(ids, feats)
        a, b = (s.search_raw(q_ids, q_feats, 5, INF, tap=True) for s in (f32, h16))
        want = F.cells_f64(kind, q_feats, feats, K)
        assert_cells(kind, a[3], want)
        assert_cells(kind, b[3], want)
        assert float(np.nanmax(cell_error(kind, b[3], a[3].astype(np.float64)))) <= 2e-5
        same_bits(b, h16.search_raw(q_ids, q_feats, 5, INF, tap=True))   # and again: the same bits
        assert expand_stats(f32) == {"cells": 0, "tiles": 0}
        assert (h16.expand_stats()["cells"] > 0) == (kind == "euclidean")
        for s in (f32, h16):   # without loss: both return the rows as given
            same_rows(s.fetch_raw(ids)[1], np.stack([np.concatenate([f, np.zeros((K - len(f), D), np.float32)]) for f in feats]))
        assert 2 * h16.info()["feature_bytes"] == store_info(f32)["feature_bytes"] > 0
    finally:
        f32.close()
        h16.close()


# ---- 10. info and refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K,D", [(3, 100), (1, 2)])
def test_info(engine, kind, K, D):
    rng = np.random.default_rng(91)
    T = 70   # past the first capacity of 64
    f32, h16 = BestFitStore(engine, kind, D, K), F16Store(engine, kind, D, K)
    try:
        assert h16.info()["feature_bytes"] == 0 and h16.expand_stats() == {"cells": 0, "tiles": 0}
        for s in (f32, h16):
            s.upsert(np.arange(1, T + 1), bank(rng, T, K, D, ragged=False))
        a, b = store_info(f32), h16.info()
        kp = 1 << (K - 1).bit_length()
        assert (a["elem"], b["elem"]) == (SA_ELEM_F32, SA_ELEM_F16) and b["elem"] == 2
        for i in (a, b):
            assert i["struct_size"] == 24 and i["Dp"] == -(-D // 32) * 32 and i["Kp"] == kp
        assert a["feature_bytes"] == 128 * kp * a["Dp"] * 4 and 2 * b["feature_bytes"] == a["feature_bytes"]
    finally:
        f32.close()
        h16.close()


def test_refusals_come_with_a_message(engine):
    with pytest.raises(EngineError, match=r"unknown element type 3 \(SA_ELEM_F32, SA_ELEM_BF16, SA_ELEM_F16\)") as ei:
        F16Store(engine, "euclidean", 16, 2, elem=3)
    assert ei.value.code == abi.SA_ERR_BAD_ARG
    with pytest.raises(EngineError, match="cosine only") as ei:   # the bf16 store's refusal stands
        Bf16Store(engine, "euclidean", 16, 2)
    assert ei.value.code == abi.SA_ERR_UNSUPPORTED
    with pytest.raises(EngineError) as ei:   # what sa_store_create refuses is refused here too
        F16Store(engine, "euclidean", 16, 33)
    assert ei.value.code == abi.SA_ERR_UNSUPPORTED
    for kind in KINDS:   # and nothing else is
        F16Store(engine, kind, 16, 2).close()
