"""A store's mutual best pairs merged in one call on the MI355X (similari_amd.consolidate over include/similari_consolidate.h).

The contract admits no tolerance: sa_store_consolidate returns, and leaves in the store, exactly the bits of sa_store_order,
sa_store_join_bestfit, the pairs of step 2 (tests/consolidate_ref.py) and one sa_store_merge / sa_store_merge_compat.  So every case
runs twin stores in one engine fed the same calls — A through the one call, B through the existing ones — and compares as raw bytes the
call's six outputs, order(), fetch rows, counts and qualities, the attributes, and a tapped join of both stores (the cells carry the
norms, the groups need d_ids / d_nobs to agree).  A second round on the result must again equal the twin's.

Inputs.  Tracklet pairs: track i (id i + 1) observes sign_i * ident[i // 2] + normal(0, 0.02): euclidean ident = uniform(0, 1), sign
+1; cosine ident = normal(0, 1), the sign alternating — the engine's cosine is the similarity and the vote prefers the smaller value,
so a pair is antipodal.  Rows of a pair lie 0.02 sqrt(2 D) apart and idents sqrt(D / 6), so the euclidean cut 0.08 sqrt(2 D) keeps
every pair and no stranger; the cosine cut is -0.9 against -0.9996 and, among 40 random directions in 24-d, nothing below -0.8.  Every
tracklet case asserts pairs == T // 2 as a condition, so none can pass with nothing merged.

Shapes are the smallest at which the kernels can go wrong: K 1, 3 (Kp 4, ragged banks), 32 (64 combined observations, every lane);
D 24, 33 (padded row), 1040 (a second turn of the 64-lane piece loop); T 2 and 40 (several workgroups of four waves)."""
import ctypes as C
import math

import numpy as np
import pytest

import consolidate_ref as CR
import test_gpu_absorb as TA
from similari_amd import abi, attrs as AT, consolidate as CO
from similari_amd.engine import Engine, EngineError
from similari_amd.f16 import SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_F32
from similari_amd.i8 import SA_ELEM_I8, I8Store
from similari_amd.merge import SA_KEEP_BEST, SA_KEEP_LATEST
from similari_amd.retain import RetainStore
from similari_amd.search import sa_topn_params

pytestmark = pytest.mark.gpu
u32, u64, f32 = np.uint32, np.uint64, np.float32
F32, BF16, F16, I8 = SA_ELEM_F32, SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_I8
NAME = {F32: "f32", BF16: "bf16", F16: "f16", I8: "i8"}
FAR = TA.FAR
FORMS = [(F32, "cosine"), (F32, "euclidean"), (F16, "cosine"), (F16, "euclidean"), (BF16, "cosine"), (I8, "cosine")]
KEEPS = {"latest": SA_KEEP_LATEST, "best": SA_KEEP_BEST}
ZERO = {"step_ms": 0.0, "compact_ms": 0.0, "pairs": 0, "rows_moved": 0, "tracks_moved": 0, "launches": 0, "host_waits": 0, "keep": 0,
        "qual_upload_bytes": 0}


def form_id(v):
    return NAME.get(v, v) if isinstance(v, int) else str(v)


@pytest.fixture(scope="module")
def engine():
    eng = Engine(abi.make_config(device=0))
    yield eng
    eng.close()


# ---- stores and inputs ---------------------------------------------------------------------------
class Twin:
    """A for the one call, B for the existing ones."""

    def __init__(self, engine, elem, kind, D, K):
        self.stores = []
        for _ in range(2):   # one at a time: a failed creation leaves the earlier one to close()
            self.stores.append(I8Store(engine, "cosine", D, K) if elem == I8 else RetainStore(engine, kind, D, K, elem))
        self.a, self.b = self.stores
        self.kind, self.D, self.K = kind, D, K

    def each(self, f):
        for s in self.stores:
            f(s)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for s in self.stores:
            s.close()


def cut_of(kind, D):
    return -0.9 if kind == "cosine" else 0.08 * math.sqrt(2 * D)


def tracklets(seed, T, D, kind, n_obs):
    """-> (rng, ids 1..T, banks): the tracklet pairs of the module docstring, n_obs[i] observations for track i."""
    rng = np.random.default_rng(seed)
    ident = rng.normal(0, 1, (T // 2 + 1, D)) if kind == "cosine" else rng.uniform(0, 1, (T // 2 + 1, D))
    banks = []
    for i in range(T):
        sign = -1.0 if kind == "cosine" and i % 2 else 1.0
        banks.append((sign * ident[i // 2] + rng.normal(0, 0.02, (int(n_obs[i]), D))).astype(f32))
    return rng, np.arange(1, T + 1, dtype=u64), banks


def sources_first(ids):
    """An upsert order that puts every source (the even ids) ahead of every destination: the destinations lie in the last slots and
    each merged bank is then moved into a hole."""
    return np.concatenate([np.flatnonzero(ids % 2 == 0), np.flatnonzero(ids % 2 == 1)])


# ---- the two routes ------------------------------------------------------------------------------
def same(a, b, rule=None):
    assert TA.state(a) == TA.state(b)
    if len(a):
        TA.same_bits(a.join_raw(3, FAR, tap=True), b.join_raw(3, FAR, tap=True))
        if rule is not None:
            TA.same_bits(a.join_raw(3, FAR, tap=True, compat=rule), b.join_raw(3, FAR, tap=True, compat=rule))


def two_calls(b, topn, cut, keep, capacity=None, rule=None, **kw):
    """Steps 1 to 3 of the header through the calls that were there before; -> (the six outputs, pairs, search stats after the join)."""
    ids = b.order()
    out_n, win, trk, wt, _ = b.join_bestfit_raw(topn, cut, compat=rule, **kw)
    stats = dict(b.last_stats(), **{"fit_" + k: v for k, v in b.bestfit_stats().items()})
    found, dest = CR.pairs(ids, out_n, win)
    if found:
        pairs = {d: [s] for d, s in found}
        if rule is None:
            b.merge(pairs, keep, capacity)
        else:   # merge refuses SA_COMPAT_ONLY_READY: both tracks of a pair were ready, or they would not be a pair
            b.merge(pairs, keep, capacity, compat=AT.Compat(AT._rule(rule).flags & ~AT.SA_COMPAT_ONLY_READY, AT._rule(rule).ready_at))
    return (out_n, win, trk, wt, ids, dest), found, stats


def both(tw, topn, cut, keep="latest", capacity=None, rule=None, **kw):
    """One consolidation through both routes, everything compared; -> (pairs [(dst, src)], the stats of A)."""
    a, b = tw.a, tw.b
    before = TA.state(a)
    got = CO.consolidate_raw(a, topn, cut, keep, capacity, rule, **kw)
    st = CO.last(a)
    mine = dict(a.last_stats(), **{"fit_" + k: v for k, v in a.bestfit_stats().items()})
    want, found, theirs = two_calls(b, topn, cut, keep, capacity, rule, **kw)
    TA.same_out(got, want)
    same(a, b, rule)
    for k in ("groups", "reruns", "fit_groups", "fit_claimed"):   # filled as after sa_store_join_bestfit
        assert mine[k] == theirs[k], k
    if found:
        assert st["pairs"] == len(found) == int((got[5] != got[4]).sum()) and st["keep"] == KEEPS[keep]
        assert st["launches"] == 2 + (1 if st["tracks_moved"] else 0) and st["host_waits"] == mine["reruns"] + 3
        assert st["step_ms"] > 0 and (st["compact_ms"] > 0) == (st["tracks_moved"] > 0)
    else:
        assert st == ZERO and TA.state(a) == before
    return found, st


def expect_pairs(found, T):
    """Every tracklet pair merged, the lower id the destination, destinations in the order of the store."""
    assert found == [(2 * i + 1, 2 * i + 2) for i in range(T // 2)] and len(found) == T // 2


# ---- 1. store types and metrics ------------------------------------------------------------------
@pytest.mark.parametrize("seed", [64, 65, 66])
@pytest.mark.parametrize("elem,kind", FORMS, ids=form_id)
def test_tracklet_pairs_leave_the_bits_of_join_then_merge(engine, elem, kind, seed):
    """T = 40, D = 24, K = 2 with capacity 3 below the combined count of 4: every pair merges, the bank shifts onto itself, and the
    second round finds nothing mutual below the cut and leaves the store as it is."""
    T, D, K = 40, 24, 2
    rng, ids, banks = tracklets(seed, T, D, kind, [K] * T)
    with Twin(engine, elem, kind, D, K + 1) as tw:
        tw.each(lambda s: s.upsert(ids, banks))
        found, st = both(tw, 2, cut_of(kind, D), "latest", 3)
        expect_pairs(found, T)
        assert st["rows_moved"] == 3 * (T // 2) and len(tw.a) == T // 2
        found, st = both(tw, 2, cut_of(kind, D), "latest", 3)
        assert found == []
        # above every distance the merged tracks pair up again, whoever they are: the twin says which
        found, st = both(tw, 1, FAR if kind == "euclidean" else 1.0, "latest")
        assert len(found) >= 1


# ---- 2. and 3. bank depths and row widths --------------------------------------------------------
@pytest.mark.parametrize("keep", ["latest", "best"])
@pytest.mark.parametrize("K,D,T", [(1, 24, 10), (3, 33, 14), (32, 24, 6), (3, 1040, 6)], ids=str)
@pytest.mark.parametrize("elem,kind", [(F32, "euclidean"), (F16, "cosine"), (I8, "cosine")], ids=form_id)
def test_bank_depths_and_row_widths(engine, elem, kind, K, D, T, keep):
    """K = 1 (Kp = 1); K = 3 (Kp = 4): counts 1..3, unfilled slots; K = 32: full banks, 64 combined observations; D = 33: a padded
    row; D = 1040: a second turn of the piece loop.  Random qualities, so SA_KEEP_BEST permutes."""
    n_obs = [K if K in (1, 32) else 1 + (i * 2 + i // 2) % K for i in range(T)]
    rng, ids, banks = tracklets(100 * K + D, T, D, kind, n_obs)
    qual = [rng.uniform(0, 1, len(x)).astype(f32) for x in banks]
    with Twin(engine, elem, kind, D, K) as tw:
        tw.each(lambda s: s.append(ids, banks, qual, "latest"))
        found, st = both(tw, 1, cut_of(kind, D), keep)
        expect_pairs(found, T)
        assert all(n == min(K, n_obs[d - 1] + n_obs[s - 1]) for (d, s), n in zip(found, tw.a.fetch_raw([d for d, _ in found])[0]))
        both(tw, 1, cut_of(kind, D), keep)


# ---- 4. retention --------------------------------------------------------------------------------
def retention_case(engine, qualities, keep, capacity, K=3, T=8, upsert=()):
    """f32 euclidean, D = 24, full banks of K; qualities(i, k) -> the quality of observation k of track i."""
    D = 24
    rng, ids, banks = tracklets(4, T, D, "euclidean", [K] * T)
    qual = [np.array([qualities(i, k) for k in range(K)], f32) for i in range(T)]
    with Twin(engine, F32, "euclidean", D, K) as tw:
        tw.each(lambda s: s.append(ids, banks, qual, "latest"))
        for i in upsert:
            tw.each(lambda s: s.upsert([ids[i]], [banks[i][::-1]]))
        found, st = both(tw, 1, cut_of("euclidean", D), keep, capacity)
        expect_pairs(found, T)
        return st, tw.a.fetch_raw(tw.a.order()), banks


def test_keep_latest_below_the_combined_count_shifts_the_bank_onto_itself(engine):
    st, (n_obs, feats, qual), banks = retention_case(engine, lambda i, k: 0.1 * k, "latest", 2)
    assert n_obs.tolist() == [2] * 4 and st["rows_moved"] == 4 * (2 + 1)   # two rows arrive, one slot is zeroed
    st, (n_obs, feats, qual), banks = retention_case(engine, lambda i, k: 0.1 * k, "latest", None)
    assert n_obs.tolist() == [3] * 4 and st["rows_moved"] == 4 * 3         # drop = 3: nothing of the bank stays
    assert np.array_equal(feats[0], banks[1])


def test_keep_best_is_stable_among_equal_qualities(engine):
    st, (n_obs, feats, qual), banks = retention_case(engine, lambda i, k: 0.5, "best", None)
    assert st["rows_moved"] == 0 and np.array_equal(feats[0], banks[0])    # the destination's own rows rank first and stay
    st, (n_obs, feats, qual), banks = retention_case(engine, lambda i, k: 0.0 if (i + k) % 2 else -0.0, "best", None)
    assert st["rows_moved"] == 0 and np.array_equal(feats[0], banks[0])    # -0.0 == 0.0
    assert np.array_equal(np.signbit(qual[0]), [True, False, True])        # and the sign travels with the observation


def test_keep_best_on_unsorted_banks_and_at_capacity_one(engine):
    """Qualities ascending inside each bank (an append under "latest" stores them as they come), two banks then rewritten by an
    upsert: qualities 0, rows reversed, the mirror stale."""
    q = lambda i, k: 0.1 + 0.2 * k + 0.05 * i
    st, (n_obs, feats, qual), banks = retention_case(engine, q, "best", None, upsert=(2, 5))
    assert np.array_equal(feats[0], np.stack([banks[1][2], banks[0][2], banks[1][1]]))
    assert st["qual_upload_bytes"] == 8 * 4 * 4
    st, (n_obs, feats, qual), banks = retention_case(engine, q, "best", 1)
    assert n_obs.tolist() == [1] * 4 and np.array_equal(feats[0, 0], banks[1][2]) and st["rows_moved"] == 4 * 3


def test_the_quality_mirror_goes_up_only_when_stale(engine):
    """After a keep-best absorb the mirror is valid: nothing is uploaded.  A call that merged a pair leaves it stale, and so does an
    upsert."""
    T, D, K = 8, 24, 3
    rng, ids, banks = tracklets(9, T, D, "euclidean", [2] * T)
    qual = [rng.uniform(0, 1, 2).astype(f32) for _ in range(T)]
    far = [np.full((1, D), 9.0, f32)]
    with Twin(engine, F32, "euclidean", D, K) as tw:
        tw.each(lambda s: s.append(ids[:6], banks[:6], qual[:6], "latest"))
        tw.each(lambda s: s.absorb_keep_raw(ids[6:], banks[6:], 1, 0.01, "best", quality=qual[6:]))
        assert tw.a.retain_stats()["created"] == 2 and tw.a.retain_stats()["qual_upload_bytes"] > 0
        found, st = both(tw, 1, cut_of("euclidean", D), "best")
        expect_pairs(found, T)
        assert st["qual_upload_bytes"] == 0
        tw.each(lambda s: s.absorb_keep_raw([77], far, 1, 0.01, "best", quality=[[0.5]]))
        assert tw.a.retain_stats()["qual_upload_bytes"] == 4 * 4 * 4      # the consolidation left the mirror stale
        tw.each(lambda s: s.upsert([78], far))
        found, st = both(tw, 1, FAR, "best")
        assert len(found) >= 1 and st["qual_upload_bytes"] == 6 * 4 * 4


# ---- 5. compaction -------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", ["latest", "best"])
@pytest.mark.parametrize("T", [2, 40])
def test_destinations_in_the_last_slots_move_into_the_holes(engine, T, keep):
    D, K = 24, 2
    rng, ids, banks = tracklets(64, T, D, "euclidean", [1 + i % 2 for i in range(T)])
    qual = [rng.uniform(0, 1, len(x)).astype(f32) for x in banks]
    order = sources_first(ids)
    with Twin(engine, F32, "euclidean", D, K) as tw:
        tw.each(lambda s: s.append(ids[order], [banks[i] for i in order], [qual[i] for i in order], "latest"))
        found, st = both(tw, 1, cut_of("euclidean", D), keep)
        expect_pairs(found, T)
        assert st["tracks_moved"] == T // 2 and st["launches"] == 3
        assert sorted(tw.a.order().tolist()) == list(range(1, T + 1, 2))


def test_sources_at_the_last_slot_need_no_move(engine):
    D, K = 24, 2
    rng, ids, banks = tracklets(65, 2, D, "euclidean", [2, 2])
    with Twin(engine, F32, "euclidean", D, K) as tw:
        tw.each(lambda s: s.upsert(ids, banks))
        found, st = both(tw, 1, cut_of("euclidean", D), "latest")
        assert found == [(1, 2)] and st["tracks_moved"] == 0 and st["launches"] == 2 and st["compact_ms"] == 0.0
        assert tw.a.order().tolist() == [1]


# ---- 6. nothing to do ----------------------------------------------------------------------------
@pytest.mark.parametrize("keep", ["latest", "best"])
def test_nothing_to_do_leaves_the_store_and_the_stats_alone(engine, keep):
    D, K = 24, 2
    rng, ids, banks = tracklets(66, 6, D, "euclidean", [2] * 6)
    with Twin(engine, F32, "euclidean", D, K) as tw:
        found, st = both(tw, 1, 1.0, keep)                       # an empty store
        assert found == [] and len(tw.a) == 0
        tw.each(lambda s: s.upsert(ids[:1], banks[:1]))
        found, st = both(tw, 1, FAR, keep)                       # one track
        assert found == [] and len(tw.a) == 1
        tw.each(lambda s: s.upsert(ids, banks))
        found, st = both(tw, 1, 1e-6, keep)                      # below every distance
        assert found == [] and len(tw.a) == 6
        found, st = both(tw, 1, cut_of("euclidean", D), keep)    # and the mirror's state is as it was: stale
        assert len(found) == 3 and st["qual_upload_bytes"] == (6 * 2 * 4 if keep == "best" else 0)


# ---- the triple ----------------------------------------------------------------------------------
def test_a_third_track_near_a_pair_stays_under_its_own_id(engine):
    D = 24
    rng = np.random.default_rng(7)
    c = rng.uniform(0, 1, D)
    banks = [(c + rng.normal(0, 0.02, (1, D))).astype(f32), (c + rng.normal(0, 0.02, (1, D))).astype(f32),
             (c + 0.3 + rng.normal(0, 0.02, (1, D))).astype(f32)]
    with Twin(engine, F32, "euclidean", D, 2) as tw:
        tw.each(lambda s: s.upsert([5, 3, 9], banks))
        found, st = both(tw, 2, FAR, "latest")
        assert found == [(3, 5)] and tw.a.order().tolist() == [9, 3]


# ---- 7. the pool's rerun -------------------------------------------------------------------------
def test_a_pool_rerun_applies_the_step_once(engine):
    """Fresh stores (a first pool holds 256 blocks): 40 tracks joined above every distance leave 780 groups, so the join runs twice.
    The step rides behind the second run alone."""
    T, D, K = 40, 24, 2
    rng, ids, banks = tracklets(64, T, D, "euclidean", [K] * T)
    with Twin(engine, F16, "euclidean", D, K) as tw:
        tw.each(lambda s: s.upsert(ids, banks))
        found, st = both(tw, 1, FAR, "latest")
        expect_pairs(found, T)
        assert st["host_waits"] == 4 and st["launches"] == 3   # both() held host_waits against reruns + 3: the join ran twice


# ---- 8. rules ------------------------------------------------------------------------------------
def test_same_key_and_disjoint_refuse_some_geometric_pairs(engine):
    T, D, K = 16, 24, 2
    rng, ids, banks = tracklets(64, T, D, "cosine", [K] * T)
    # pair j: 0 one camera, disjoint spans; 1 two cameras; 2 one camera, overlapping spans; 3 one camera, disjoint, the source first
    keys = [j % 2 if (i // 2) % 4 != 1 else i % 2 for i, j in ((i, i // 2) for i in range(T))]
    starts = [{0: 100 * (i % 2), 1: 100 * (i % 2), 2: 50 * (i % 2), 3: 100 * (1 - i % 2)}[(i // 2) % 4] for i in range(T)]
    ends = [s + 80 for s in starts]
    rule = AT.compat(same_key=True, disjoint=True)
    with Twin(engine, F32, "cosine", D, K) as tw:
        tw.each(lambda s: s.upsert(ids, banks))
        tw.each(lambda s: s.set_attrs(ids, keys, starts, ends))
        found, st = both(tw, 1, cut_of("cosine", D), "latest", rule=rule)
        assert found == [(2 * j + 1, 2 * j + 2) for j in range(T // 2) if j % 4 in (0, 3)]
        got = tw.a.get_attrs([d for d, _ in found])
        assert all(got[d] == (keys[d - 1], 0, 180) for d, _ in found)          # the union
        assert tw.a.get_attrs([3])[3] == (keys[2], starts[2], ends[2])         # a refused pair keeps its own


def test_only_ready_pairs_ready_tracks_alone(engine):
    T, D, K = 16, 24, 1
    rng, ids, banks = tracklets(65, T, D, "euclidean", [K] * T)
    ends = [50 if (i // 2) % 2 == 0 or i % 2 == 0 else 500 for i in range(T)]   # every second pair has a track that is not ready
    rule = AT.compat(ready_at=100)
    with Twin(engine, F32, "euclidean", D, K) as tw:
        tw.each(lambda s: s.upsert(ids, banks))
        tw.each(lambda s: s.set_attrs(ids, [0] * T, [0] * T, ends))
        found, st = both(tw, 1, cut_of("euclidean", D), "latest", rule=rule)
        assert found == [(2 * j + 1, 2 * j + 2) for j in range(T // 2) if j % 2 == 0]


def test_without_a_rule_no_attribute_is_touched_and_query_first_is_refused(engine):
    T, D, K = 6, 24, 1
    rng, ids, banks = tracklets(66, T, D, "euclidean", [K] * T)
    with Twin(engine, F32, "euclidean", D, K) as tw:
        tw.each(lambda s: s.upsert(ids, banks))
        tw.each(lambda s: s.set_attrs(ids, ids, 10 * ids, 10 * ids + 5))
        before = TA.state(tw.a)
        with pytest.raises(EngineError) as ex:
            CO.consolidate_raw(tw.a, 1, 1.0, compat=AT.compat(query_first=True))
        assert ex.value.code == abi.SA_ERR_BAD_ARG and "SA_COMPAT_QUERY_FIRST" in str(ex.value)
        assert TA.state(tw.a) == before and CO.last(tw.a) == ZERO
        found, st = both(tw, 1, cut_of("euclidean", D), "latest")
        expect_pairs(found, T)
        assert tw.a.get_attrs([1, 3, 5]) == {i: (i, 10 * i, 10 * i + 5) for i in (1, 3, 5)}


# ---- 9. refusals ---------------------------------------------------------------------------------
def test_refusals_leave_the_store_and_the_mirror_as_they_were(engine):
    T, D, K = 8, 24, 3
    rng, ids, banks = tracklets(64, T, D, "euclidean", [2] * T)
    qual = [rng.uniform(0, 1, 2).astype(f32) for _ in range(T)]
    with Twin(engine, F32, "euclidean", D, K) as tw:
        tw.each(lambda s: s.absorb_keep_raw(ids, banks, 1, 1e-6, "best", quality=qual))   # every track created, the mirror valid
        a = tw.a
        before = TA.state(a)
        cut = cut_of("euclidean", D)
        for word, kw in [("unknown keep", dict(topn=1, max_distance=cut, keep=7)), ("capacity", dict(topn=1, max_distance=cut, capacity=K + 1)),
                         ("NaN", dict(topn=1, max_distance=math.nan)), ("topn must be", dict(topn=0, max_distance=cut)),
                         ("unknown rule bits", dict(topn=1, max_distance=cut, compat=AT.Compat(0x100)))]:
            with pytest.raises(EngineError) as ex:
                CO.consolidate_raw(a, **kw)
            assert ex.value.code == abi.SA_ERR_BAD_ARG and word in str(ex.value), (word, str(ex.value))
            assert TA.state(a) == before and CO.last(a) == ZERO, word
        # what the join refuses is refused with the join's code
        for kw in (dict(topn=1, max_distance=math.nan), dict(topn=0, max_distance=cut), dict(topn=1, max_distance=cut, compat=AT.Compat(0x100))):
            with pytest.raises(EngineError) as ex:
                a.join_bestfit_raw(**kw)
            assert ex.value.code == abi.SA_ERR_BAD_ARG
        # null outputs through the C call itself: out_dest may not be null, out_track and out_ids may
        prm = sa_topn_params(1, 1, cut, math.inf)
        out_n, win, wt, dest = np.zeros(T, u32), np.zeros((T, 1), u64), np.zeros((T, 1), np.float64), np.zeros(T, u64)
        p64, p32, pd = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_double)
        full = [out_n.ctypes.data_as(p32), win.ctypes.data_as(p64), None, wt.ctypes.data_as(pd), None, dest.ctypes.data_as(p64)]
        lib = CO._lib(a)
        for hole in (0, 1, 3, 5):
            args = list(full)
            args[hole] = None
            rc = lib.sa_store_consolidate(a.h, 0, C.byref(prm), None, 0, *args)
            assert rc == abi.SA_ERR_BAD_ARG and "null argument" in lib.sa_last_error(a.engine.h).decode(), hole
            assert TA.state(a) == before and CO.last(a) == ZERO, hole
        # the mirror is as it was — valid —: the call that follows equals the twin without an upload
        found, st = both(tw, 1, cut, "best")
        expect_pairs(found, T)
        assert st["qual_upload_bytes"] == 0


# ---- 10. stats and the repeated call -------------------------------------------------------------
def test_the_launches_do_not_depend_on_the_number_of_tracks(engine):
    """Sources first, so that the compaction has a track to move at T = 2 as well as at T = 40 (a source that already lies behind
    every track that stays needs no launch: test_sources_at_the_last_slot_need_no_move)."""
    D, K = 24, 1
    seen = {}
    for T in (2, 40):
        rng, ids, banks = tracklets(64, T, D, "euclidean", [K] * T)
        order = sources_first(ids)
        with Twin(engine, F32, "euclidean", D, K) as tw:
            tw.each(lambda s: s.upsert(ids[order], [banks[i] for i in order]))
            found, st = both(tw, 1, cut_of("euclidean", D), "latest")
            expect_pairs(found, T)
            assert st["pairs"] == T // 2 and st["host_waits"] == 3
            seen[T] = st["launches"]
    assert seen[2] == seen[40] == 3


def test_consolidate_all_takes_two_rounds_for_four_tracklets_per_identity(engine):
    """One call merges pairs, not clusters.  Tracks 4j .. 4j + 3 observe identity j; 4j, 4j + 1 lie 0.005 sqrt(2 D) = 0.035 apart
    and so do 4j + 2, 4j + 3, the two halves 0.05 sqrt(2 D) = 0.35, all below the cut of 0.55: the halves are mutual in the first
    round, the merged halves in the second, and a third finds nothing."""
    n, D, K = 5, 24, 4
    rng = np.random.default_rng(11)
    ident = rng.uniform(0, 1, (n, D))
    half = rng.normal(0, 0.05, (2 * n, D))
    ids = np.arange(1, 4 * n + 1, dtype=u64)
    banks = [(ident[i // 4] + half[i // 2] + rng.normal(0, 0.005, (1, D))).astype(f32) for i in range(4 * n)]
    with Twin(engine, F32, "euclidean", D, K) as tw:
        tw.each(lambda s: s.upsert(ids, banks))
        cut = cut_of("euclidean", D)
        rounds = 0
        while True:   # the twin, round by round
            found, st = both(tw, 1, cut, "latest")
            if not found:
                break
            rounds += 1
        assert rounds == 2 and len(tw.a) == n
        assert sorted((int(i) - 1) // 4 for i in tw.a.order()) == list(range(n))
        assert all(m == 4 for m in tw.a.fetch_raw(tw.a.order())[0])
    with Twin(engine, F32, "euclidean", D, K) as tw:
        tw.a.upsert(ids, banks)
        final = CO.consolidate_all(tw.a, 1, cut, max_rounds=8)
        left = set(int(i) for i in tw.a.order())
        assert len(left) == n and len(final) == 3 * n and set(final.values()) == left
        assert all((s - 1) // 4 == (d - 1) // 4 for s, d in final.items())
        winners, merged = CO.consolidate(tw.a, 1, cut)
        assert merged == {} and CO.last(tw.a) == ZERO
