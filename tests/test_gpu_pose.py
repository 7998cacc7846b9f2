"""Keypoint association on the MI355X (similari_amd.pose over include/similari_pose.h) against the numpy model tests/pose_ref.py: the
tap matrix carries the model's bits, the vote reaches the total of the oracle's kuhn_munkres on SortVoting's dense matrix and its
matches wherever the optimum is unique.  "Bits" is the comparison of tests/test_gpu_points.py.

Shapes: P in {1, 17, 65} (65 crosses the 64-point LDS chunk of k_pose_tile) with (m, T) in {(1, 1), (3, 5), (17, 70), (70, 17)} (below,
at and across the 16 x 64 tile edges); a crowd of 300 x 300 for the dense search; 2048 x 2048 for the limits.  A scene's model is
computed once and shared by the tests that need it."""
import ctypes as C
import functools

import numpy as np
import pytest

import devrows_ref as dref
import points_ref as R
import pose_ref as PR
from similari_amd import abi
from similari_amd import pose as PS
from similari_amd.devrows import DeviceRows
from similari_amd.engine import Engine, EngineError
from similari_amd.f16 import SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_F32
from similari_amd.points import SA_ROW_NONE, sa_point_rows
from similari_amd.pose import PoseBank
from test_gpu_points import bits, device_block, to_source

pytestmark = pytest.mark.gpu
f32, u8, u32, u64 = np.float32, np.uint8, np.uint32, np.uint64
SHAPES = [(1, 1), (3, 5), (17, 70), (70, 17), (33, 130)]   # (33, 130): a block's tile row and tile column both beyond 1, both edges partial


@pytest.fixture(scope="module")
def eng():
    e = Engine(abi.make_config(positional="iou", positional_threshold=0.3, device=0))
    yield e
    e.close()


class Scene:
    """Tracks from four rounds of step (30 % of the points absent, a tenth never sighted), one state seeded indefinite; the poses of
    the next frame with 30 % of the points absent.  Read-only once built."""

    def __init__(self, m, T, P, crowd, indefinite=True, grid=False):
        rng = np.random.default_rng(1000 * P + 10 * m + T)
        self.m, self.T, self.P = m, T, P
        self.ids = (np.arange(T, dtype=u64) * 3 + 5)
        centres = PR.people(rng, T, P, crowd)
        if grid:   # multiples of 4 below 1024: exact in f16 and in bf16, so a 16-bit source shows the poses where the tracks are
            centres = np.round(centres / 4.0) * 4.0
        self.rounds = PR.track_rounds(rng, centres)
        self.model = PR.model_bank(self.rounds)
        self.seeded = (T // 2, int(np.argmax(self.model.has[T // 2])))   # this state gets a negative definite covariance: its pivots fail
        if indefinite:
            self.model.cov[self.seeded] = -np.abs(self.model.cov[self.seeded]) - f32(1)
        self.poses, self.pres = PR.poses_of(rng, centres, m, noise=0.0 if grid else 0.05)
        for a in (self.poses, self.pres):
            a.setflags(write=False)

    @functools.lru_cache(maxsize=None)
    def weights(self, min_common=1):
        w = PR.weights(self.poses, self.pres, self.model.has, self.model.mean, self.model.cov, R.PW, min_common)
        w.setflags(write=False)
        return w

    @functools.lru_cache(maxsize=None)
    def vote(self, min_common=1, threshold=1.0):
        return PR.vote(self.weights(min_common), threshold)

    def bank(self, eng):
        b = PoseBank(eng, self.P)
        for z, pres in self.rounds:
            b.step(self.ids, z, present=pres)
        s = self.seeded[0]
        has = self.model.has[s]
        b.set_state(self.ids[s], has, np.where(has[:, None], self.model.mean[s], 0), np.where(has[:, None, None], self.model.cov[s], 0))
        return b


@functools.lru_cache(maxsize=None)
def scene(m, T, P, crowd=False, grid=False):
    return Scene(m, T, P, crowd, grid=grid)


# ---- 1. the matrix -----------------------------------------------------------------------------------
@pytest.mark.parametrize("min_common", [1, 3])
@pytest.mark.parametrize("m,T", SHAPES)
@pytest.mark.parametrize("P", [1, 17, 65])
def test_the_tap_matrix_carries_the_models_bits(eng, P, m, T, min_common):
    sc = scene(m, T, P)
    want = sc.weights(min_common)
    with sc.bank(eng) as bank:
        ids, w, tap = bank.associate(sc.poses, present=sc.pres, min_common=min_common, matrix=True)
        st = bank.last_associate()
    assert bits(tap, want)
    assert (st["launches"], st["poses"], st["tracks"]) == (3, m, T)
    assert st["bytes_h2d"] == sc.poses.nbytes + m * P and st["bytes_d2h"] == 8 * m + 4 + 4 * m * T and st["src_bytes"] == 0
    if P > 1 and m > 1:
        assert (want[~np.isnan(want)] > 50).any()   # somebody continues a track
    if P == 17 and T > 1:
        assert sc.model.has[sc.seeded] and not sc.model.has.all()   # the indefinite state is there; some points were never sighted
        assert np.isnan(R.distance(sc.model.mean[sc.seeded], sc.model.cov[sc.seeded], np.zeros(2, f32)))


# ---- 2. the vote -------------------------------------------------------------------------------------
def check_vote(sc, ids, w, st, min_common=1, threshold=1.0):
    total, ref, wq, thr_q = sc.vote(min_common, threshold)
    want_w = sc.weights(min_common)
    col_of = {int(t): j for j, t in enumerate(sc.ids)}
    got = np.array([col_of[int(t)] if t else -1 for t in ids], np.int64)
    hit = got >= 0
    assert len(set(ids[hit].tolist())) == int(hit.sum())          # no track twice
    assert PR.total_of(got, wq, thr_q) == total                    # kuhn_munkres's total
    assert (wq[np.flatnonzero(hit), sc.m + got[hit]] > thr_q).all()
    assert bits(w[hit], want_w[np.flatnonzero(hit), got[hit]]) and np.isnan(w[~hit]).all()
    differ = np.flatnonzero(got != ref)
    if len(differ):   # only where the model finds that the optimum is not unique
        assert not PR.forced_rows(wq, total, ref, rows=differ)[differ].any()
    assert st["matched"] == int(hit.sum()) and st["launches"] == 3
    assert st["roots"] == PR.greedy_roots(wq, thr_q)
    return st["roots"]


@pytest.mark.parametrize("min_common", [1, 3])
@pytest.mark.parametrize("m,T", SHAPES)
@pytest.mark.parametrize("P", [1, 17, 65])
def test_the_vote_reaches_the_models_total(eng, P, m, T, min_common):
    sc = scene(m, T, P, crowd=True)
    with sc.bank(eng) as bank:
        ids, w = bank.associate(sc.poses, present=sc.pres, min_common=min_common)
        st = bank.last_associate()
    check_vote(sc, ids, w, st, min_common)
    assert st["bytes_d2h"] == 8 * m + 4   # without the tap only the results come back


def test_the_vote_in_a_crowd_runs_the_dense_search(eng):
    sc = scene(300, 300, 2, crowd=True)
    total, ref, wq, thr_q = sc.vote()
    lost = PR.greedy_roots(wq, thr_q)   # on the CPU, from the model alone: is this a crowd at all?
    assert lost >= 1, "the scene is no crowd: every row keeps its greedy bid and the dense search would not run"
    with sc.bank(eng) as bank:
        ids, w = bank.associate(sc.poses, present=sc.pres)
        st = bank.last_associate()
    roots = check_vote(sc, ids, w, st)
    assert roots >= 1 and roots == lost
    assert (ref >= 0).sum() > 100


# ---- 3. the limits -----------------------------------------------------------------------------------
def test_2048_by_2048_and_one_beyond(eng):
    P, n = 2, PS.SA_POSE_MAX
    sc = Scene(n, n + 1, P, crowd=False, indefinite=False)   # one track more than a call takes
    with PoseBank(eng, P) as bank:
        for z, pres in sc.rounds:
            bank.step(sc.ids, z, present=pres)
        ids_t = sc.ids[:n]
        w = PR.weights(sc.poses, sc.pres, sc.model.has[:n], sc.model.mean[:n], sc.model.cov[:n])
        # People far apart: a row has at most one usable pair, and no two rows have the same: that assignment is the optimum, no solver needed
        usable = np.nan_to_num(w, nan=0.0) > 1.0
        assert usable.sum(1).max() == 1 and usable.sum(0).max() == 1 and usable.sum() > 1000
        want = np.where(usable.any(1), ids_t[np.argmax(usable, 1)], 0).astype(u64)
        ids, got_w = bank.associate(sc.poses, present=sc.pres, ids=ids_t)
        st = bank.last_associate()
        assert (ids == want).all() and st["roots"] == 0 and st["launches"] == 3 and st["matched"] == int(usable.any(1).sum())
        rows = np.flatnonzero(usable.any(1))
        assert bits(got_w[rows], w[rows, np.argmax(usable, 1)[rows]]) and np.isnan(got_w[~usable.any(1)]).all()
        # one beyond, either way
        for kw in (dict(ids=None), dict(ids=sc.ids)):
            with pytest.raises(EngineError) as ei:
                bank.associate(sc.poses, present=sc.pres, **kw)
            assert ei.value.code == abi.SA_ERR_UNSUPPORTED and bank.last_associate()["launches"] == 0
        more = np.concatenate([sc.poses, sc.poses[:1]])
        with pytest.raises(EngineError) as ei:
            bank.associate(more, ids=ids_t)
        assert ei.value.code == abi.SA_ERR_UNSUPPORTED and bank.last_associate()["launches"] == 0
        assert (bank.associate(sc.poses, present=sc.pres, ids=ids_t)[0] == want).all()   # the next good call works


# ---- 4. poses in device memory -----------------------------------------------------------------------
@pytest.mark.parametrize("comps", [2, 3])
@pytest.mark.parametrize("elem", [SA_ELEM_F32, SA_ELEM_F16, SA_ELEM_BF16])
def test_poses_read_from_device_memory(eng, elem, comps):
    sc = scene(17, 70, 17, grid=True)
    P, m, T, B, off = sc.P, sc.m, sc.T, 40, 4
    L = P * comps
    W = L + 11   # a column slice of a wider output
    eb = 4 if elem == SA_ELEM_F32 else 2
    rng = np.random.default_rng(7 + elem)
    index = rng.permutation(B)[:m].astype(u32)
    index[3] = index[9] = SA_ROW_NONE
    index[5] = index[2]   # a row named twice: two poses of one person
    vals = rng.uniform(-300, 300, (B, W)).astype(f32)
    block = np.zeros((B, P, comps), f32)
    got = index != SA_ROW_NONE
    block[index[got], :, :2] = sc.poses[got]
    if comps == 3:
        block[..., 2] = rng.uniform(0, 1, (B, P))
    vals[:, off: off + L] = block.reshape(B, L)
    vals[index[0], off] = np.nan   # a point that is not finite in the source
    src = to_source(vals, elem)
    wide = dref.widen(src, elem)[:, off: off + L].reshape(B, P, comps)
    z = np.zeros((m, P, comps), f32)
    z[got] = wide[index[got]]
    mask = sc.pres & got[:, None]   # the host twin: a pose without a row has every point absent
    with sc.bank(eng) as bank, device_block(eng, src) as ptr:
        rows = DeviceRows(ptr + off * eb, B, W, elem, index)
        ids_d, w_d, tap_d = bank.associate(rows=rows, present=sc.pres, comps=comps, min_score=0.4, matrix=True)
        st = bank.last_associate()
        ids_h, w_h, tap_h = bank.associate(z, present=mask, min_score=0.4, matrix=True)
        assert (ids_d == ids_h).all() and bits(w_d, w_h) and bits(tap_d, tap_h)
        assert np.isnan(tap_d[[3, 9]]).all() and ids_d[3] == 0 and ids_d[9] == 0 and (ids_d != 0).sum() >= 3
        assert st["launches"] == 3 and st["bytes_h2d"] == m * 4 + m * P and st["src_bytes"] == int(got.sum()) * L * eb
        pres = R.present_of(z, 0.4, mask)
        assert bits(tap_d, PR.weights(z[..., :2], pres, sc.model.has, sc.model.mean, sc.model.cov))
        # without an index and without a mask: pose i is row i
        ids_d, w_d, tap_d = bank.associate(rows=DeviceRows(ptr + off * eb, B, W, elem), comps=comps, matrix=True)
        assert bank.last_associate()["bytes_h2d"] == 0 and tap_d.shape == (B, T)
        ids_h, w_h, tap_h = bank.associate(np.ascontiguousarray(wide), matrix=True)
        assert (ids_d == ids_h).all() and bits(w_d, w_h) and bits(tap_d, tap_h)


# ---- 5. no state changes -----------------------------------------------------------------------------
def test_associate_changes_no_state_and_ids_permute_the_columns(eng):
    sc = scene(17, 70, 17, crowd=True)
    with sc.bank(eng) as bank:
        order = bank.order().tolist()
        before = [bank.state(i) for i in sc.ids]
        ids0, w0, tap0 = bank.associate(sc.poses, present=sc.pres, matrix=True)
        assert bank.last_associate()["bytes_h2d"] == sc.poses.nbytes + sc.m * sc.P   # every track: no slot table
        ids1, w1, tap1 = bank.associate(sc.poses, present=sc.pres, ids=bank.order(), matrix=True)
        assert (ids0 == ids1).all() and bits(w0, w1) and bits(tap0, tap1)
        perm = np.random.default_rng(3).permutation(sc.T)
        ids2, w2, tap2 = bank.associate(sc.poses, present=sc.pres, ids=sc.ids[perm], matrix=True)
        assert bits(tap2, tap0[:, perm])
        total, ref, wq, thr_q = sc.vote()
        assert PR.forced_rows(wq, total, ref).all()    # the model finds the optimum unique, so no order of the columns may change an id
        assert (ids2 == ids0).all() and bits(w2, w0)
        assert bank.last_associate()["bytes_h2d"] == sc.poses.nbytes + sc.m * sc.P + sc.T * 4
        sub = sc.ids[::2]
        ids3, w3, tap3 = bank.associate(sc.poses, present=sc.pres, ids=sub, matrix=True)
        assert bits(tap3, tap0[:, ::2]) and set(ids3.tolist()) <= set(sub.tolist()) | {0}
        assert bank.order().tolist() == order
        for x, i in zip(before, sc.ids):
            y = bank.state(i)
            assert (x[0] == y[0]).all() and bits(x[1], y[1]) and bits(x[2], y[2])
        assert bank.last()["launches"] == 1 and bank.last()["tracks"] == sc.T   # sa_points_last still speaks of the last step


# ---- 6. the frame loop -------------------------------------------------------------------------------
def test_track_equals_the_plain_calls(eng):
    P = 17
    rng = np.random.default_rng(11)
    centres = PR.people(rng, 12, P, False)
    next_id = [100]

    def fresh(n):
        out = np.arange(next_id[0], next_id[0] + n, dtype=u64)
        next_id[0] += n
        return out

    with PoseBank(eng, P) as a, PoseBank(eng, P) as b:
        births = coasted = 0
        id_of = {}   # person -> the id of the track that follows them
        for k in range(5):
            shown = np.arange(8) if k == 0 else np.arange(12) if k < 3 else np.delete(np.arange(12), 4)   # births at k = 1; one person gone from k = 3
            z = (centres[shown] + rng.normal(0, 0.03, (len(shown), P, 2))).astype(f32)
            pres = rng.random((len(shown), P)) >= 0.2
            new = fresh(len(shown))
            got = a.track(z, new, present=pres)
            # the plain calls on the twin
            ids, _ = b.associate(z, present=pres)
            idle = [t for t in b.order().tolist() if t not in set(ids.tolist())]
            unmatched = np.flatnonzero(ids == 0)
            ids[unmatched] = new[: len(unmatched)]
            b.step(ids, z, present=pres)
            if idle:
                b.predict(np.array(idle, u64))
            assert (got == ids).all(), k
            births += len(unmatched) if k else 0
            coasted += len(idle)
            for person, t in zip(shown, got):
                assert id_of.setdefault(int(person), int(t)) == int(t), (k, person)   # everybody keeps their id
            assert a.order().tolist() == b.order().tolist()
            for t in a.order():
                x, y = a.state(t), b.state(t)
                assert (x[0] == y[0]).all() and bits(x[1], y[1]) and bits(x[2], y[2]), (k, t)
        assert births == 4 and coasted == 2 and len(a) == 12
        # coast=False leaves the unmatched track as it is
        before = a.state(id_of[4])
        a.track(z, fresh(len(z)), present=pres, coast=False)
        after = a.state(id_of[4])
        assert bits(before[1], after[1]) and bits(before[2], after[2])


# ---- 7. refusals -------------------------------------------------------------------------------------
def test_every_refusal_leaves_everything_as_it_was(eng):
    sc = scene(3, 5, 17, crowd=True)
    lib = eng.lib
    with sc.bank(eng) as bank:
        m, T = sc.m, sc.T
        want = bank.associate(sc.poses, present=sc.pres)
        before = [bank.state(i) for i in sc.ids]
        z = np.ascontiguousarray(sc.poses)
        zp = z.ctypes.data_as(C.POINTER(C.c_float))
        out_t, out_w = np.full(m, 77, u64), np.full(m, 5.0, f32)
        tp, wp = out_t.ctypes.data_as(C.POINTER(C.c_uint64)), out_w.ctypes.data_as(C.POINTER(C.c_float))

        def rows(size=40, comps=2, host=zp, dev=None):
            return C.byref(sa_point_rows(size, comps, 0.0, 0, host, None, dev))

        def opts(size=16, min_common=1, threshold=1.0):
            return C.byref(PS.sa_pose_options(size, min_common, threshold, 0))

        def arr(*v):
            a = np.array(v, u64)
            return a.ctypes.data_as(C.POINTER(C.c_uint64)), a

        good = arr(*sc.ids)
        zero, twice, unknown = arr(5, 0, 11), arr(5, 8, 5), arr(5, 8, 9999)
        d = DeviceRows(0x1000, 3, sc.P * 2, SA_ELEM_F32).struct()
        B, NF = abi.SA_ERR_BAD_ARG, abi.SA_ERR_NOT_FOUND
        f = lib.sa_points_associate
        cases = [
            (B, lambda: f(bank.h, T, good[0], m, None, opts(), tp, wp, None)),
            (B, lambda: f(bank.h, T, good[0], m, rows(), None, tp, wp, None)),
            (B, lambda: f(bank.h, T, good[0], m, rows(), opts(), None, wp, None)),
            (B, lambda: f(bank.h, T, good[0], m, rows(), opts(), tp, None, None)),
            (B, lambda: f(bank.h, 3, zero[0], m, rows(), opts(), tp, wp, None)),
            (B, lambda: f(bank.h, 3, twice[0], m, rows(), opts(), tp, wp, None)),
            (NF, lambda: f(bank.h, 3, unknown[0], m, rows(), opts(), tp, wp, None)),
            (B, lambda: f(bank.h, T, good[0], m, rows(), opts(size=12), tp, wp, None)),
            (B, lambda: f(bank.h, T, good[0], m, rows(size=32), opts(), tp, wp, None)),
            (B, lambda: f(bank.h, T, good[0], m, rows(comps=4), opts(), tp, wp, None)),
            (B, lambda: f(bank.h, T, good[0], m, rows(host=None), opts(), tp, wp, None)),
            (B, lambda: f(bank.h, T, good[0], m, rows(dev=C.pointer(d)), opts(), tp, wp, None)),
            (B, lambda: f(bank.h, T, good[0], m, rows(host=None, dev=C.pointer(d)), opts(), tp, wp, None)),   # a span in no registered block
            (B, lambda: f(bank.h, T, good[0], m, rows(), opts(min_common=0), tp, wp, None)),
            (B, lambda: f(bank.h, T, good[0], m, rows(), opts(threshold=float("nan")), tp, wp, None)),
            (B, lambda: f(bank.h, T, good[0], m, rows(), opts(threshold=float("inf")), tp, wp, None)),
            (B, lambda: f(bank.h, T, good[0], m, rows(), opts(threshold=-0.5), tp, wp, None)),
        ]
        for k, (code, call) in enumerate(cases):
            assert call() == code, k
            assert lib.sa_last_error(eng.h), k
            assert bank.last_associate()["launches"] == 0, k
            assert (out_t == 77).all() and (out_w == 5.0).all(), k
            got = bank.associate(sc.poses, present=sc.pres)   # the next good call works
            assert (got[0] == want[0]).all() and bits(got[1], want[1]), k
        for x, i in zip(before, sc.ids):
            y = bank.state(i)
            assert (x[0] == y[0]).all() and bits(x[1], y[1]) and bits(x[2], y[2])
        # nothing to match: SA_OK without a launch
        assert f(bank.h, T, good[0], 0, None, opts(), None, None, None) == 0 and bank.last_associate()["launches"] == 0
        assert f(bank.h, 0, good[0], m, rows(), opts(), tp, wp, None) == 0 and bank.last_associate()["launches"] == 0
        assert (out_t == 0).all() and np.isnan(out_w).all()
    with PoseBank(eng, sc.P) as empty:   # a bank without tracks
        ids, w = empty.associate(sc.poses)
        assert (ids == 0).all() and np.isnan(w).all() and empty.last_associate()["launches"] == 0
