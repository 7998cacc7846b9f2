"""The OKS metric on the MI355X (similari_amd.pose_oks over include/similari_pose_oks.h) against the numpy model tests/oks_ref.py: the tap
carries the model's bits, the vote reaches the total of the oracle's kuhn_munkres and the model's matches on scenes whose optimum
tests/test_oks_scenes_ref.py proves unique on the CPU, the batch, the frame loop and the tracker do under OKS what they do under the
Mahalanobis metric, and a bank that switched back leaves the bits of one that never switched.  "Bits" is the comparison of
tests/test_gpu_points.py.

Shapes: P in {2, 17, 65} (65 crosses the 64-point LDS chunk) with (m, T) in {(1, 1), (3, 5), (17, 70), (70, 17)} (below, at and across
the 16 x 64 tile edges); P = 1, where no pair has a body size; a crowd of 150 x 150 for the dense search; 2048 x 2048 for the limits."""
import ctypes as C

import numpy as np
import pytest

import devrows_ref as dref
import oks_ref as OR
import points_ref as R
import pose_ref as PR
import pose_sort_ref as SR
from similari_amd import abi
from similari_amd import pose as PS
from similari_amd import pose_oks as K
from similari_amd.devrows import DeviceRows
from similari_amd.engine import Engine, EngineError
from similari_amd.f16 import SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_F32
from similari_amd.points import SA_ROW_NONE
from similari_amd.pose import PoseBank
from similari_amd.pose_oks import COCO_SIGMAS, OksMetric, get_metric, set_metric
from similari_amd.pose_sort import KeypointSort
from similari_amd.pose_track import PoseTrackBank
from test_gpu_points import bits, device_block, to_source
from test_gpu_pose_sort import call_of, records_equal, same_as_model, wasted_equal

pytestmark = pytest.mark.gpu
f32, u8, u32, u64 = np.float32, np.uint8, np.uint32, np.uint64
SHAPES = [(1, 1), (3, 5), (17, 70), (70, 17)]


@pytest.fixture(scope="module")
def eng():
    e = Engine(abi.make_config(positional="iou", positional_threshold=0.3, device=0))
    yield e
    e.close()


def bank_of(eng, sc, cls=PoseBank, metric=True):
    b = cls(eng, sc.P, metric=OksMetric(sc.sigmas) if metric else None)
    for z, pres in sc.rounds:
        b.step(sc.ids, z, present=pres)
    return b


# ---- 1. the matrix -----------------------------------------------------------------------------------
@pytest.mark.parametrize("min_common", [1, 3])
@pytest.mark.parametrize("m,T", SHAPES)
@pytest.mark.parametrize("P", [2, 17, 65])
def test_the_tap_matrix_carries_the_models_bits(eng, P, m, T, min_common):
    sc = OR.scene(m, T, P)
    want = sc.weights(min_common)
    with bank_of(eng, sc) as bank:
        ids, w, tap = bank.associate(sc.poses, present=sc.pres, min_common=min_common, matrix=True)
        st = bank.last_associate()
    assert bits(tap, want)
    assert (st["launches"], st["poses"], st["tracks"]) == (4, m, T)   # extents, factor, tile, assign
    assert st["bytes_h2d"] == sc.poses.nbytes + m * P and st["bytes_d2h"] == 8 * m + 4 + 4 * m * T
    real = want[~np.isnan(want)]
    assert ((real >= 0) & (real <= 1)).all()
    if P > 2 and m > 1:
        assert (real > 0.5).any() and (real == 0).any()   # somebody continues a track; pairs beyond the cut of exp


@pytest.mark.parametrize("comps", [2, 3])
@pytest.mark.parametrize("elem", [SA_ELEM_F32, SA_ELEM_F16, SA_ELEM_BF16])
def test_poses_read_from_device_memory(eng, elem, comps):
    """Rows in f32, f16 and bf16, a column slice of a wider block (strided), gathered by an index with SA_ROW_NONE and a row named twice."""
    sc = OR.scene(17, 70, 17, grid=True)
    P, m, T, B, off = sc.P, sc.m, sc.T, 40, 4
    L = P * comps
    W = L + 11
    eb = 4 if elem == SA_ELEM_F32 else 2
    rng = np.random.default_rng(7 + elem)
    index = rng.permutation(B)[:m].astype(u32)
    index[3] = index[9] = SA_ROW_NONE
    index[5] = index[2]
    vals = rng.uniform(-300, 300, (B, W)).astype(f32)
    block = np.zeros((B, P, comps), f32)
    got = index != SA_ROW_NONE
    block[index[got], :, :2] = sc.poses[got]
    if comps == 3:
        block[..., 2] = rng.uniform(0, 1, (B, P))
    vals[:, off: off + L] = block.reshape(B, L)
    vals[index[0], off] = np.nan
    src = to_source(vals, elem)
    wide = dref.widen(src, elem)[:, off: off + L].reshape(B, P, comps)
    z = np.zeros((m, P, comps), f32)
    z[got] = wide[index[got]]
    mask = sc.pres & got[:, None]
    with bank_of(eng, sc) as bank, device_block(eng, src) as ptr:
        rows = DeviceRows(ptr + off * eb, B, W, elem, index)
        ids_d, w_d, tap_d = bank.associate(rows=rows, present=sc.pres, comps=comps, min_score=0.4, matrix=True)
        st = bank.last_associate()
        ids_h, w_h, tap_h = bank.associate(z, present=mask, min_score=0.4, matrix=True)
        assert (ids_d == ids_h).all() and bits(w_d, w_h) and bits(tap_d, tap_h)
        assert np.isnan(tap_d[[3, 9]]).all() and ids_d[3] == 0 and ids_d[9] == 0 and (ids_d != 0).sum() >= 3
        assert st["launches"] == 4 and st["bytes_h2d"] == m * 4 + m * P and st["src_bytes"] == int(got.sum()) * L * eb
        pres = R.present_of(z, 0.4, mask)
        assert bits(tap_d, OR.weights(z[..., :2], pres, sc.model.has, sc.model.mean, sc.sigmas))
        ids_d, w_d, tap_d = bank.associate(rows=DeviceRows(ptr + off * eb, B, W, elem), comps=comps, matrix=True)   # no index, no mask
        ids_h, w_h, tap_h = bank.associate(np.ascontiguousarray(wide), matrix=True)
        assert tap_d.shape == (B, T) and (ids_d == ids_h).all() and bits(w_d, w_h) and bits(tap_d, tap_h)


def test_one_point_has_no_body_size(eng):
    """P = 1: every side is a single point, s2 = 0, every pair is refused — every cell NaN, every pose creates a track."""
    rng = np.random.default_rng(4)
    centres = PR.people(rng, 9, 1, False)
    rounds = PR.track_rounds(rng, centres, absent=0.0, never=0.0)
    ids = np.arange(1, 10, dtype=u64)
    z = (centres[:6] + rng.normal(0, 0.01, (6, 1, 2))).astype(f32)
    with PoseTrackBank(eng, 1, metric=OksMetric([0.05])) as bank:
        for zz, pres in rounds:
            bank.step(ids, zz, present=pres)
        got, w, tap = bank.associate(z, matrix=True)
        assert np.isnan(tap).all() and tap.shape == (6, 9) and (got == 0).all() and np.isnan(w).all()
        set_metric(bank, None)   # the Mahalanobis vote finds them
        assert (bank.associate(z)[0] == ids[:6]).all()
        set_metric(bank, OksMetric([0.05]))
        out = bank.track(z, 100)
        assert out.tolist() == list(range(100, 106)) and bank.last_track()["created"] == 6 and len(bank) == 15


# ---- 2. the vote -------------------------------------------------------------------------------------
def check_vote(sc, ids, w, st, min_common=1, threshold=OR.THRESHOLD):
    total, ref, wq, thr_q = sc.vote(min_common, threshold)
    want_w = sc.weights(min_common)
    col_of = {int(t): j for j, t in enumerate(sc.ids)}
    got = np.array([col_of[int(t)] if t else -1 for t in ids], np.int64)
    hit = got >= 0
    assert len(set(ids[hit].tolist())) == int(hit.sum())
    assert PR.total_of(got, wq, thr_q) == total                    # kuhn_munkres's total
    assert (got == ref).all()                                      # and its matches: every row is forced (test_oks_scenes_ref.py)
    assert bits(w[hit], want_w[np.flatnonzero(hit), got[hit]]) and np.isnan(w[~hit]).all()
    assert st["matched"] == int(hit.sum()) and st["launches"] == 4
    assert st["roots"] == PR.greedy_roots(wq, thr_q)
    return st["roots"]


@pytest.mark.parametrize("m,T", OR.VOTE_SHAPES)
@pytest.mark.parametrize("P", [2, 17])
def test_the_vote_equals_the_models_in_every_row(eng, P, m, T):
    sc = OR.scene(m, T, P, crowd=True)
    with bank_of(eng, sc) as bank:
        ids, w = bank.associate(sc.poses, present=sc.pres)   # no threshold given: 0.3 under an OksMetric
        st = bank.last_associate()
        check_vote(sc, ids, w, st)
        assert st["bytes_d2h"] == 8 * m + 4
        none, _ = bank.associate(sc.poses, present=sc.pres, threshold=1.0)   # the diagonal of the Mahalanobis vote matches nothing: w <= 1
        assert (none == 0).all()


def test_the_vote_in_a_crowd_runs_the_dense_search(eng):
    m, T, P = OR.CROWD
    sc = OR.scene(m, T, P, crowd=True)
    total, ref, wq, thr_q = sc.vote()
    lost = PR.greedy_roots(wq, thr_q)
    assert lost >= 1
    with bank_of(eng, sc) as bank:
        ids, w = bank.associate(sc.poses, present=sc.pres)
        st = bank.last_associate()
    assert check_vote(sc, ids, w, st) == lost


def test_2048_by_2048_and_one_beyond(eng):
    P, n = 2, PS.SA_POSE_MAX
    sc = OR.Scene(n, n + 1, P, crowd=False)
    with PoseBank(eng, P, metric=OksMetric(sc.sigmas)) as bank:
        for z, pres in sc.rounds:
            bank.step(sc.ids, z, present=pres)
        ids_t = sc.ids[:n]
        w = OR.weights(sc.poses, sc.pres, sc.model.has[:n], sc.model.mean[:n], sc.sigmas)
        usable = np.nan_to_num(w, nan=0.0) > f32(OR.THRESHOLD)
        # people far apart: a row has at most one usable pair and no two rows the same: that assignment is the optimum, no solver needed
        assert usable.sum(1).max() == 1 and usable.sum(0).max() == 1 and usable.sum() > 500
        want = np.where(usable.any(1), ids_t[np.argmax(usable, 1)], 0).astype(u64)
        ids, got_w = bank.associate(sc.poses, present=sc.pres, ids=ids_t)
        st = bank.last_associate()
        assert (ids == want).all() and st["roots"] == 0 and st["launches"] == 4 and st["matched"] == int(usable.any(1).sum())
        rows = np.flatnonzero(usable.any(1))
        assert bits(got_w[rows], w[rows, np.argmax(usable, 1)[rows]]) and np.isnan(got_w[~usable.any(1)]).all()
        for kw in (dict(ids=None), dict(ids=sc.ids)):   # 2049 tracks
            with pytest.raises(EngineError) as ei:
                bank.associate(sc.poses, present=sc.pres, **kw)
            assert ei.value.code == abi.SA_ERR_UNSUPPORTED and bank.last_associate()["launches"] == 0
        with pytest.raises(EngineError) as ei:   # 2049 poses
            bank.associate(np.concatenate([sc.poses, sc.poses[:1]]), ids=ids_t)
        assert ei.value.code == abi.SA_ERR_UNSUPPORTED and bank.last_associate()["launches"] == 0
        assert (bank.associate(sc.poses, present=sc.pres, ids=ids_t)[0] == want).all()


# ---- 3. a batch --------------------------------------------------------------------------------------
def test_a_batch_returns_what_associate_returns_per_scene(eng):
    """Four scenes in one bank: 17 x 70, one without tracks, 70 x 17, one without poses."""
    P = 17
    parts = [OR.scene(17, 70, P, crowd=True), OR.scene(3, 5, P, crowd=True), OR.scene(70, 17, P, crowd=True), OR.scene(1, 1, P)]
    sig = parts[0].sigmas
    with PoseBank(eng, P, metric=OksMetric(sig)) as bank:
        scenes, base = [], 0
        for k, sc in enumerate(parts):
            ids = sc.ids + u64(base)
            base += 1000
            for z, pres in sc.rounds:
                bank.step(ids, z + f32(500 * k), present=pres)
            scenes.append((ids, (sc.poses + f32(500 * k)).astype(f32), sc.pres))
        scenes[1] = (np.zeros(0, u64), scenes[1][1], scenes[1][2])                                           # no tracks
        scenes[3] = (scenes[3][0], np.zeros((0, P, 2), f32), np.zeros((0, P), bool))                         # no poses
        got = bank.associate_batch(scenes, matrix=True)
        st = bank.last_associate_batch()
        assert st["launches"] == 4 and st["scenes"] == 4
        matched = 0
        for k, (ids, z, pres) in enumerate(scenes):
            if len(z) == 0:
                assert len(got[k][0]) == 0
                continue
            one = bank.associate(z, present=pres, ids=ids, matrix=True)
            assert (got[k][0] == one[0]).all() and bits(got[k][1], one[1]) and bits(got[k][2], one[2]), k
            assert st["scene_roots"][k] == bank.last_associate()["roots"]
            matched += int((one[0] != 0).sum())
        assert st["matched"] == matched and matched >= 20 and (got[1][0] == 0).all()


# ---- 4. the frame loop -------------------------------------------------------------------------------
def states_equal(a, b):
    assert a.order().tolist() == b.order().tolist()
    for t in a.order():
        x, y = a.state(t), b.state(t)
        assert (x[0] == y[0]).all() and bits(x[1], y[1]) and bits(x[2], y[2]), t


def test_track_leaves_the_bits_of_the_plain_calls(eng):
    """Five frames: PoseTrackBank.track (one call) against PoseBank.track (associate, step, predict) on a twin, both under OKS."""
    P = 17
    rng = np.random.default_rng(11)
    centres = PR.people(rng, 12, P, False)
    metric = OksMetric(COCO_SIGMAS)
    with PoseTrackBank(eng, P, metric=metric) as a, PoseBank(eng, P, metric=metric) as b:
        next_id, coasted = 100, 0
        for k in range(5):
            shown = np.arange(8) if k == 0 else np.arange(12) if k < 3 else np.delete(np.arange(12), 4)
            z = (centres[shown] + rng.normal(0, 0.03, (len(shown), P, 2))).astype(f32)
            pres = rng.random((len(shown), P)) >= 0.2
            new = np.arange(next_id, next_id + len(shown), dtype=u64)
            next_id += len(shown)
            got = a.track(z, new, present=pres)
            st = a.last_track()
            want = PoseBank.track(b, z, new, present=pres)
            assert (got == want).all(), k
            assert st["vote_launches"] == (4 if k else 0), k   # the extents launch is one of the vote's under OKS
            coasted += st["coasted"]
            states_equal(a, b)
        assert len(a) == 12 and coasted == 2


def test_track_batch_leaves_the_bits_of_the_plain_calls(eng):
    P = 17
    rng = np.random.default_rng(12)
    cams = [PR.people(rng, n, P, False) + 400.0 * k for k, n in enumerate((9, 20, 3))]
    metric = OksMetric(COCO_SIGMAS)
    with PoseTrackBank(eng, P, metric=metric) as a, PoseBank(eng, P, metric=metric) as b:
        lists = [np.zeros(0, u64) for _ in cams]
        next_id = 1
        for k in range(5):
            scenes = []
            for c, centres in enumerate(cams):
                shown = rng.permutation(len(centres))[: len(centres) - (k + c) % 3]
                z = (centres[shown] + rng.normal(0, 0.03, (len(shown), P, 2))).astype(f32)
                scenes.append((lists[c], z, rng.random((len(shown), P)) >= 0.2))
            m = sum(len(s[1]) for s in scenes)
            new = np.arange(next_id, next_id + m, dtype=u64)
            next_id += m
            got = a.track_batch(scenes, new)
            st = a.last_track()
            want = PoseBank.track_batch(b, scenes, new)
            for c in range(len(cams)):
                assert (got[c] == want[c]).all(), (k, c)
                lists[c] = np.union1d(lists[c], got[c]).astype(u64)
            assert st["vote_launches"] == (4 if k else 0) and (k == 0 or st["matched"] >= 20), k
            states_equal(a, b)


# ---- 5. the tracker ----------------------------------------------------------------------------------
@pytest.mark.parametrize("gated", [False, True], ids=["no constraints", "(1, 1.0)"])
def test_eight_frames_of_the_tracker_against_the_model(eng, gated):
    P = 17
    mdl = OR.sort_model(gated, P)
    cons = OR.SORT_CONS if gated else []
    expired = refused_seen = 0
    with KeypointSort(eng, P, max_idle_epochs=OR.SORT_IDLE, constraints=cons, metric=OksMetric(OR.sort_sigmas(P))) as trk:
        assert get_metric(trk.bank()) == OksMetric(OR.sort_sigmas(P))
        for e, fr in enumerate(OR.sort_frames(P)):
            if e in (3, 5, 7):   # the vote alone, cell by cell: peek's tap, the refused pairs
                pl = mdl.plan([f[0] for f in fr])
                got = trk.peek(call_of(fr), matrix=True)
                st = trk.last()
                refused = 0
                for k, f in enumerate(SR.present_of(fr)):
                    w, no, raw = mdl.weights(pl, k, f[1], f[2])
                    assert bits(got[f[0]][2], w), (e, k)
                    refused += int(no.sum())
                    tracks = np.array(pl["tracks"][k] + [0], u64)
                    assert (got[f[0]][0] == tracks[PR.vote(w, mdl.threshold)[1]]).all(), (e, k)
                assert (st["gate_launches"], st["vote_launches"], st["refused_pairs"], st["expired"]) == (1, 3, refused, len(pl["expired"])), e
                assert bool(refused) == gated
                refused_seen += refused
            want = mdl.predict(fr)
            records_equal(trk.predict(call_of(fr)), fr, want)
            st = trk.last()
            assert st["gate_launches"] == (1 if e else 0) and st["vote_launches"] == (3 if e else 0), e   # ONE extents launch, gate or no gate
            assert e == 0 or st["gate_ms"] > 0
            expired += wasted_equal(trk, mdl)
            same_as_model(trk, mdl)
        assert expired >= 2 and (refused_seen > 0) == gated


# ---- 6. switching ------------------------------------------------------------------------------------
def test_a_bank_that_switched_back_is_a_bank_that_never_switched(eng):
    sc = OR.scene(17, 70, 17, crowd=True)
    oks = OksMetric(sc.sigmas)
    rng = np.random.default_rng(5)
    with bank_of(eng, sc, PoseTrackBank, metric=False) as a, bank_of(eng, sc, PoseTrackBank, metric=False) as b:
        assert get_metric(b) is None
        set_metric(b, oks)
        assert get_metric(b) == oks and b.metric == oks
        _, _, tap = b.associate(sc.poses, present=sc.pres, matrix=True)
        assert b.last_associate()["launches"] == 4 and bits(tap, sc.weights())
        set_metric(b, None)
        assert get_metric(b) is None
        states_equal(a, b)   # the metric changed no state
        ra, rb = a.associate(sc.poses, present=sc.pres, matrix=True), b.associate(sc.poses, present=sc.pres, matrix=True)
        assert (ra[0] == rb[0]).all() and bits(ra[1], rb[1]) and bits(ra[2], rb[2]) and (ra[0] != 0).sum() >= 5
        assert bits(ra[2], sc.mahalanobis())
        assert a.last_associate()["launches"] == b.last_associate()["launches"] == 3
        for k in range(3):
            z = (sc.poses + rng.normal(0, 0.02, sc.poses.shape)).astype(f32)
            ia, ib = a.track(z, 5000 + 100 * k, present=sc.pres), b.track(z, 5000 + 100 * k, present=sc.pres)
            assert (ia == ib).all() and a.last_track()["vote_launches"] == b.last_track()["vote_launches"] == 3
            states_equal(a, b)


# ---- 7. refusals -------------------------------------------------------------------------------------
def test_every_refusal_of_set_metric_leaves_the_previous_metric(eng):
    P = 5
    lib = eng.lib
    with PoseBank(eng, P, metric=OksMetric([0.1, 0.2, 0.3, 0.4, 0.5])) as bank:
        K.bind(lib)
        good = np.array([0.5, 0.4, 0.3, 0.2, 0.1], f32)

        def metric(size=24, kind=K.SA_POSE_METRIC_OKS, n=P, reserved=0, sig=good):
            sig = np.ascontiguousarray(sig, f32)
            m = K.sa_pose_metric(size, kind, n, reserved, sig.ctypes.data_as(C.POINTER(C.c_float)) if len(sig) else None)
            m._keep = sig
            return m

        cases = [
            lambda: lib.sa_points_set_metric(bank.h, None),
            lambda: lib.sa_points_set_metric(None, C.byref(metric())),
            lambda: lib.sa_points_set_metric(bank.h, C.byref(metric(size=20))),
            lambda: lib.sa_points_set_metric(bank.h, C.byref(metric(size=32))),
            lambda: lib.sa_points_set_metric(bank.h, C.byref(metric(kind=2))),
            lambda: lib.sa_points_set_metric(bank.h, C.byref(metric(n=P - 1))),
            lambda: lib.sa_points_set_metric(bank.h, C.byref(metric(n=P + 1, sig=np.ones(P + 1)))),
            lambda: lib.sa_points_set_metric(bank.h, C.byref(metric(n=0, sig=[]))),
            lambda: lib.sa_points_set_metric(bank.h, C.byref(metric(sig=[]))),                                    # null sigmas
            lambda: lib.sa_points_set_metric(bank.h, C.byref(metric(kind=K.SA_POSE_METRIC_MAHALANOBIS))),        # sigmas for a metric that takes none
            lambda: lib.sa_points_set_metric(bank.h, C.byref(metric(reserved=1))),
            lambda: lib.sa_points_set_metric(bank.h, C.byref(metric(kind=K.SA_POSE_METRIC_MAHALANOBIS, n=0, reserved=1))),
        ] + [lambda bad=bad, at=at: lib.sa_points_set_metric(bank.h, C.byref(metric(sig=np.where(np.arange(P) == at, bad, good))))
             for at in (0, P - 1) for bad in (0.0, -0.1, np.nan, np.inf, -np.inf)]
        for k, call in enumerate(cases):
            assert call() == abi.SA_ERR_BAD_ARG, k
            assert get_metric(bank) == OksMetric([0.1, 0.2, 0.3, 0.4, 0.5]), k   # the previous metric stays
        assert lib.sa_points_set_metric(bank.h, C.byref(metric())) == 0 and get_metric(bank) == OksMetric(good)
        kind = C.c_uint32(7)
        assert lib.sa_points_get_metric(bank.h, C.byref(kind), None) == 0 and kind.value == K.SA_POSE_METRIC_OKS
        set_metric(bank, OksMetric(good))
        with pytest.raises(EngineError):
            set_metric(bank, OksMetric([0.1] * 4))
        assert bank.metric == OksMetric(good) and get_metric(bank) == OksMetric(good)   # the Python face keeps the previous metric, too
