"""Keypoint association for a batch of scenes on the MI355X (PoseBank.associate_batch over include/similari_pose_batch.h): every scene of
a call returns what the single call returns for it — the tap bit for bit tests/pose_ref.py's weights and the single call's, the matches
and weights the single call's, the vote under the conditions of tests/test_gpu_pose.py's check_vote — and no pose is given a track of
another scene.

ONE bank holds the tracks of all scenes of a call, a scene's ids offset by OFF * (its number + 1); the single calls it is compared with
run on the same bank with `ids=` the scene's tracks.  The scenes are test_gpu_pose's (computed once, shared through its cache).

Shapes: (m, T) = (1, 1), (3, 5), (0, 4), (17, 70), (4, 0), (70, 17), (17, 65) in that order in one call: first tracks 0, 1, 6, 10, 80, 80, 97
and gain offsets 0, 1, 16, 16, 1206, 1206, 2396 — no multiples of the tile or of a 16-byte piece —, a scene without poses, one without
tracks, two of several tiles, and one column into a second tile.  P in {1, 17, 65} (65 crosses the 64-point LDS chunk)."""
import ctypes as C

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
from test_gpu_points import device_block, to_source
from test_gpu_pose import Scene, bits, check_vote, scene

pytestmark = pytest.mark.gpu
f32, u8, u32, u64 = np.float32, np.uint8, np.uint32, np.uint64
SHAPES = [(1, 1), (3, 5), (0, 4), (17, 70), (4, 0), (70, 17), (17, 65)]
OFF = 100000


@pytest.fixture(scope="module")
def eng():
    e = Engine(abi.make_config(positional="iou", positional_threshold=0.3, device=0))
    yield e
    e.close()


class NoTracks:
    """m poses and no track to continue."""

    def __init__(self, m, P):
        rng = np.random.default_rng(77 + m + P)
        self.m, self.T, self.P = m, 0, P
        self.ids = np.zeros(0, u64)
        self.rounds = []
        self.poses = rng.uniform(0, 100, (m, P, 2)).astype(f32)
        self.pres = rng.random((m, P)) >= 0.3

    def weights(self, min_common=1):
        return np.full((self.m, 0), np.nan, f32)


class SeededScene(Scene):
    """A Scene from a seed of its own: Scene seeds by its shape, so two of one shape would be the same people."""

    def __init__(self, m, T, P, crowd, seed):
        rng = np.random.default_rng(seed)
        self.m, self.T, self.P = m, T, P
        self.ids = (np.arange(T, dtype=u64) * 3 + 5)
        centres = PR.people(rng, T, P, crowd)
        self.rounds = PR.track_rounds(rng, centres)
        self.model = PR.model_bank(self.rounds)
        self.seeded = (T // 2, int(np.argmax(self.model.has[T // 2])))
        self.model.cov[self.seeded] = -np.abs(self.model.cov[self.seeded]) - f32(1)
        self.poses, self.pres = PR.poses_of(rng, centres, m)
        for a in (self.poses, self.pres):
            a.setflags(write=False)


def scenes_of(P, crowd=False, grid=False, shapes=SHAPES):
    kw = dict(grid=True) if grid else dict(crowd=True) if crowd else {}   # (as test_gpu_pose names them: one cache entry for both files)
    return [NoTracks(m, P) if T == 0 else scene(m, T, P, **kw) for m, T in shapes]


def ids_of(scs):
    return [sc.ids + u64(OFF * (s + 1)) for s, sc in enumerate(scs)]


def fill(bank, scs, seed_state=True):
    """The tracks of every scene into one bank, as Scene.bank builds a scene's own."""
    for sc, t in zip(scs, ids_of(scs)):
        for z, pres in sc.rounds:
            bank.step(t, z, present=pres)
        if sc.T and seed_state:
            s = sc.seeded[0]
            has = sc.model.has[s]
            bank.set_state(t[s], has, np.where(has[:, None], sc.model.mean[s], 0), np.where(has[:, None, None], sc.model.cov[s], 0))
    return bank


def call_of(scs):
    return [(t, sc.poses, sc.pres) for sc, t in zip(scs, ids_of(scs))]


def local(ids, s):
    """a scene's answers in the scene's own ids; every match lies inside the scene"""
    hit = ids != 0
    assert ((ids[hit] > OFF * (s + 1)) & (ids[hit] < OFF * (s + 2))).all(), s
    return np.where(hit, ids - u64(OFF * (s + 1)), u64(0)).astype(u64)


def tiles_of(scs):
    return sum((sc.m + 15) // 16 * ((sc.T + 63) // 64) for sc in scs if sc.m and sc.T)


def equal_to_single_calls(bank, scs, got, **kw):
    for s, (sc, t) in enumerate(zip(scs, ids_of(scs))):
        one = bank.associate(sc.poses, present=sc.pres, ids=t, matrix=len(got[s]) > 2, **kw)
        assert (got[s][0] == one[0]).all() and bits(got[s][1], one[1]), s
        if len(one) > 2:
            assert bits(got[s][2], one[2]), s


# ---- 1. the matrix -----------------------------------------------------------------------------------
@pytest.mark.parametrize("min_common", [1, 3])
@pytest.mark.parametrize("P", [1, 17, 65])
def test_every_scenes_tap_carries_the_models_bits(eng, P, min_common):
    scs = scenes_of(P)
    assert [(sc.m, sc.T) for sc in scs] == SHAPES
    with fill(PoseBank(eng, P), scs) as bank:
        got = bank.associate_batch(call_of(scs), min_common=min_common, matrix=True)
        st = bank.last_associate_batch()
        for s, sc in enumerate(scs):
            assert got[s][2].shape == (sc.m, sc.T) and bits(got[s][2], sc.weights(min_common)), s
            local(got[s][0], s)
        equal_to_single_calls(bank, scs, got, min_common=min_common)
    m, T, cells = sum(sc.m for sc in scs), sum(sc.T for sc in scs), sum(sc.m * sc.T for sc in scs)
    assert (st["launches"], st["scenes"], st["poses"], st["tracks"], st["tiles"]) == (3, len(scs), m, T, tiles_of(scs))
    assert st["bytes_h2d"] == 32 * len(scs) + 4 * T + m * P * 2 * 4 + m * P and st["src_bytes"] == 0
    assert st["bytes_d2h"] == 8 * m + 4 * len(scs) + 4 * cells
    assert st["matched"] == sum(int((g[0] != 0).sum()) for g in got) and st["roots"] == int(st["scene_roots"].sum())
    assert (got[4][0] == 0).all() and np.isnan(got[4][1]).all() and st["scene_roots"][4] == 0   # the scene without tracks
    assert len(got[2][0]) == 0 and st["scene_roots"][2] == 0                                      # the scene without poses


# ---- 2. the vote -------------------------------------------------------------------------------------
def check_votes(bank, scs, got, st, min_common=1):
    roots = st["scene_roots"]
    for s, sc in enumerate(scs):
        ids, w = got[s][0], got[s][1]
        if sc.m == 0 or sc.T == 0:
            assert (ids == 0).all() and np.isnan(w).all() and roots[s] == 0, s
            continue
        check_vote(sc, local(ids, s), w, {"matched": int((ids != 0).sum()), "launches": st["launches"], "roots": int(roots[s])}, min_common)
    equal_to_single_calls(bank, scs, got, min_common=min_common)
    assert st["roots"] == int(roots.sum()) and st["launches"] == 3


@pytest.mark.parametrize("min_common", [1, 3])
@pytest.mark.parametrize("P", [1, 17, 65])
def test_every_scenes_vote_reaches_the_models_total(eng, P, min_common):
    scs = scenes_of(P, crowd=True)
    with fill(PoseBank(eng, P), scs) as bank:
        got = bank.associate_batch(call_of(scs), min_common=min_common)
        st = bank.last_associate_batch()
        check_votes(bank, scs, got, st, min_common)
    m = sum(sc.m for sc in scs)
    assert st["bytes_d2h"] == 8 * m + 4 * len(scs)   # without the tap only the results and the roots come back


def test_three_crowds_run_their_dense_searches_side_by_side(eng):
    P = 2
    crowds = [SeededScene(150, 150, P, True, seed) for seed in (31, 32, 33)]
    scs = [crowds[0], scene(3, 5, P), crowds[1], scene(17, 70, P), crowds[2]]
    for sc in crowds:   # on the CPU, from the model alone: is this a crowd at all?
        total, ref, wq, thr_q = sc.vote()
        assert PR.greedy_roots(wq, thr_q) >= 1, "the scene is no crowd: every row keeps its greedy bid and the dense search would not run"
    with fill(PoseBank(eng, P), scs) as bank:
        got = bank.associate_batch(call_of(scs))
        st = bank.last_associate_batch()
        check_votes(bank, scs, got, st)
    assert all(st["scene_roots"][s] >= 1 for s in (0, 2, 4))
    assert not np.array_equal(crowds[0].poses, crowds[1].poses)


# ---- 3. isolation ------------------------------------------------------------------------------------
def test_no_pose_is_given_a_track_of_another_scene(eng):
    sc, other = scene(17, 70, 17, crowd=True), scene(3, 5, 17)
    far = [(z + f32(50000), pres) for z, pres in other.rounds]   # tracks nowhere near anybody's poses
    with PoseBank(eng, sc.P) as bank:
        a, b, c = sc.ids + u64(OFF), sc.ids + u64(2 * OFF), other.ids + u64(3 * OFF)
        for z, pres in sc.rounds:
            bank.step(a, z, present=pres)
            bank.step(b, z, present=pres)   # the same coordinates under other ids
        for z, pres in far:
            bank.step(c, z, present=pres)
        one = bank.associate(sc.poses, present=sc.pres, ids=a)
        assert (one[0] != 0).sum() >= 5
        # two scenes of the same tracks and the same poses: each finds its own
        (ia, wa), (ib, wb) = bank.associate_batch([(a, sc.poses, sc.pres), (b, sc.poses, sc.pres)])
        assert (ia == one[0]).all() and bits(wa, one[1])
        assert (local(ia, 0) == local(ib, 1)).all() and bits(wa, wb)
        # poses that stand only where another scene's tracks are: nobody to continue
        (ia, wa), (ic, wc) = bank.associate_batch([(a, sc.poses, sc.pres), (c, sc.poses, sc.pres)])
        assert (ia == one[0]).all() and (ic == 0).all() and np.isnan(wc).all()
        (ic, wc), (ia, wa) = bank.associate_batch([(c, sc.poses, sc.pres), (a, sc.poses, sc.pres)])
        assert (ia == one[0]).all() and (ic == 0).all() and np.isnan(wc).all()
        # in ONE scene over both sets of tracks they would be matched: the scenes are what keeps them apart
        both = bank.associate(sc.poses, present=sc.pres, ids=np.concatenate([c, a]))
        assert (both[0] == one[0]).all()


# ---- 4. more scenes than compute units ---------------------------------------------------------------
def test_300_small_scenes_equal_their_single_calls(eng):
    P, S = 3, 300
    rng = np.random.default_rng(300)
    ms, ns = rng.integers(1, 6, S), rng.integers(1, 6, S)
    centres = [PR.people(rng, int(n), P, bool(s % 2)) + 20.0 * s for s, n in enumerate(ns)]
    ids = [np.arange(1, n + 1, dtype=u64) + u64(OFF * (s + 1)) for s, n in enumerate(ns)]
    rounds = PR.track_rounds(rng, np.concatenate(centres))
    poses = [PR.poses_of(rng, c, int(m)) for c, m in zip(centres, ms)]
    with PoseBank(eng, P) as bank:
        for z, pres in rounds:
            bank.step(np.concatenate(ids), z, present=pres)
        call = [(t, z, pres) for t, (z, pres) in zip(ids, poses)]
        got = bank.associate_batch(call, matrix=True)
        st = bank.last_associate_batch()
        assert (st["launches"], st["scenes"], st["tiles"], st["poses"], st["tracks"]) == (3, S, S, int(ms.sum()), int(ns.sum()))
        roots = 0
        for s, (t, z, pres) in enumerate(call):
            one = bank.associate(z, present=pres, ids=t, matrix=True)
            assert (got[s][0] == one[0]).all() and bits(got[s][1], one[1]) and bits(got[s][2], one[2]), s
            assert st["scene_roots"][s] == bank.last_associate()["roots"], s
            local(got[s][0], s)
            roots += bank.last_associate()["roots"]
        assert st["roots"] == roots and st["matched"] > S // 2


# ---- 5. the limits -----------------------------------------------------------------------------------
def test_a_2048_by_2048_scene_beside_a_small_one_and_one_beyond(eng):
    P, n = 2, PS.SA_POSE_MAX
    sc = Scene(n, n + 1, P, crowd=False, indefinite=False)   # one track more than a scene takes
    small = scene(1, 1, P)
    with PoseBank(eng, P) as bank:
        big_ids, small_ids = sc.ids + u64(OFF), small.ids + u64(2 * OFF)
        for z, pres in sc.rounds:
            bank.step(big_ids, z, present=pres)
        for z, pres in small.rounds:
            bank.step(small_ids, z, present=pres)
        ids_t = big_ids[:n]
        w = PR.weights(sc.poses, sc.pres, sc.model.has[:n], sc.model.mean[:n], sc.model.cov[:n])
        # People far apart: a row has at most one usable pair, and no two rows have the same: that assignment is the optimum, no solver needed
        usable = np.nan_to_num(w, nan=0.0) > 1.0
        assert usable.sum(1).max() == 1 and usable.sum(0).max() == 1 and usable.sum() > 1000
        want = np.where(usable.any(1), ids_t[np.argmax(usable, 1)], 0).astype(u64)
        one_small = bank.associate(small.poses, present=small.pres, ids=small_ids)
        good = [(small_ids, small.poses, small.pres), (ids_t, sc.poses, sc.pres)]
        (i1, w1), (ids, got_w) = bank.associate_batch(good)
        st = bank.last_associate_batch()
        assert (ids == want).all() and st["roots"] == 0 and st["launches"] == 3 and st["tiles"] == 1 + 128 * 32
        assert st["matched"] == int(usable.any(1).sum()) + int((i1 != 0).sum())
        rows = np.flatnonzero(usable.any(1))
        assert bits(got_w[rows], w[rows, np.argmax(usable, 1)[rows]]) and np.isnan(got_w[~usable.any(1)]).all()
        assert (i1 == one_small[0]).all() and bits(w1, one_small[1])
        # one beyond, either way, in one scene
        more = np.concatenate([sc.poses, sc.poses[:1]])
        for bad in ([good[0], (big_ids, sc.poses, sc.pres)], [good[0], (ids_t, more, np.ones((n + 1, P), bool))], [(big_ids, sc.poses, sc.pres), good[0]]):
            with pytest.raises(EngineError) as ei:
                bank.associate_batch(bad)
            assert ei.value.code == abi.SA_ERR_UNSUPPORTED and "scene %d" % (0 if bad[0][0] is big_ids else 1) in str(ei.value)
            assert bank.last_associate_batch()["launches"] == 0
        (i1, w1), (ids, got_w) = bank.associate_batch(good)   # the next good call works
        assert (ids == want).all() and (i1 == one_small[0]).all() and bank.last_associate_batch()["launches"] == 3


# ---- 6. poses in device memory -----------------------------------------------------------------------
@pytest.mark.parametrize("comps", [2, 3])
@pytest.mark.parametrize("elem", [SA_ELEM_F32, SA_ELEM_F16, SA_ELEM_BF16])
def test_poses_read_from_device_memory(eng, elem, comps):
    P = 17
    scs = scenes_of(P, grid=True, shapes=[(17, 70), (3, 5), (70, 17)])
    tids = ids_of(scs)
    poses, pres = np.concatenate([sc.poses for sc in scs]), np.concatenate([sc.pres for sc in scs])
    counts = [sc.m for sc in scs]
    m, B, off = len(poses), 120, 4
    L = P * comps
    W = L + 11   # a column slice of a wider output
    eb = 4 if elem == SA_ELEM_F32 else 2
    rng = np.random.default_rng(70 + elem)
    index = rng.permutation(B)[:m].astype(u32)
    index[[3, 9, 18, 89]] = SA_ROW_NONE   # in the first scene, the second and the last
    index[5] = index[2]                   # a row named twice: two poses of one person
    vals = rng.uniform(-300, 300, (B, W)).astype(f32)
    block = np.zeros((B, P, comps), f32)
    got = index != SA_ROW_NONE
    block[index[got], :, :2] = poses[got]
    if comps == 3:
        block[..., 2] = rng.uniform(0, 1, (B, P))
    vals[:, off: off + L] = block.reshape(B, L)
    vals[index[0], off] = np.nan   # a point that is not finite in the source
    src = to_source(vals, elem)
    wide = dref.widen(src, elem)[:, off: off + L].reshape(B, P, comps)
    z = np.zeros((m, P, comps), f32)
    z[got] = wide[index[got]]
    mask = pres & got[:, None]   # the host twin: a pose without a row has every point absent
    ends = np.cumsum(counts)[:-1]
    with fill(PoseBank(eng, P), scs) as bank, fill(PoseBank(eng, P), scs) as twin, device_block(eng, src) as ptr:
        rows = DeviceRows(ptr + off * eb, B, W, elem, index)
        dev = bank.associate_batch(rows=rows, track_ids=tids, pose_counts=counts, present=pres, comps=comps, min_score=0.4, matrix=True)
        st = bank.last_associate_batch()
        host = twin.associate_batch([(t, zs, ms) for t, zs, ms in zip(tids, np.split(z, ends), np.split(mask, ends))], min_score=0.4, matrix=True)
        present = R.present_of(z, 0.4, mask)
        for s, sc in enumerate(scs):
            assert (dev[s][0] == host[s][0]).all() and bits(dev[s][1], host[s][1]) and bits(dev[s][2], host[s][2]), s
            lo = sum(counts[:s])
            assert bits(dev[s][2], PR.weights(z[lo: lo + sc.m, :, :2], present[lo: lo + sc.m], sc.model.has, sc.model.mean, sc.model.cov)), s
            local(dev[s][0], s)
        assert np.isnan(dev[0][2][[3, 9]]).all() and np.isnan(dev[1][2][1]).all() and np.isnan(dev[2][2][69]).all()
        assert sum(int((d[0] != 0).sum()) for d in dev) >= 10
        T = sum(sc.T for sc in scs)
        assert st["launches"] == 3 and st["bytes_h2d"] == 32 * 3 + 4 * T + m * 4 + m * P and st["src_bytes"] == int(got.sum()) * L * eb
        # without an index and without a mask: pose i of the call is row i; the flat form of the ids
        counts_b = [17, 3, 100]
        dev = bank.associate_batch(rows=DeviceRows(ptr + off * eb, B, W, elem), track_ids=np.concatenate(tids), track_counts=[sc.T for sc in scs],
                                   pose_counts=counts_b, comps=comps, matrix=True)
        assert bank.last_associate_batch()["bytes_h2d"] == 32 * 3 + 4 * T and dev[2][2].shape == (100, 17)
        host = twin.associate_batch([(t, zs) for t, zs in zip(tids, np.split(np.ascontiguousarray(wide), np.cumsum(counts_b)[:-1]))], matrix=True)
        for s in range(3):
            assert (dev[s][0] == host[s][0]).all() and bits(dev[s][1], host[s][1]) and bits(dev[s][2], host[s][2]), s


# ---- 7. no state changes, no record of the single call changes -----------------------------------------
def test_the_batch_changes_no_state_and_not_the_single_calls_records(eng):
    P = 17
    scs = scenes_of(P, crowd=True)
    with fill(PoseBank(eng, P), scs) as bank:
        every = np.concatenate(ids_of(scs))
        order = bank.order().tolist()
        before = [bank.state(i) for i in every]
        bank.associate(scs[3].poses, present=scs[3].pres, ids=ids_of(scs)[3])
        rec, rec_points = bank.last_associate(), bank.last()
        assert rec["launches"] == 3
        bank.associate_batch(call_of(scs), matrix=True)
        assert bank.last_associate_batch()["launches"] == 3
        assert bank.last_associate() == rec and bank.last() == rec_points
        with pytest.raises(EngineError):
            bank.associate_batch(call_of(scs), min_common=0)
        assert bank.last_associate() == rec and bank.last() == rec_points   # nor does a refused one
        assert bank.order().tolist() == order
        for x, i in zip(before, every):
            y = bank.state(i)
            assert (x[0] == y[0]).all() and bits(x[1], y[1]) and bits(x[2], y[2])


# ---- 8. the frame loop -------------------------------------------------------------------------------
def test_track_batch_equals_three_banks_that_track(eng):
    P, S = 17, 3
    rng = np.random.default_rng(12)
    centres = [PR.people(rng, 12, P, False) + 300.0 * s for s in range(S)]
    next_id = [100]

    def fresh(n):
        out = np.arange(next_id[0], next_id[0] + n, dtype=u64)
        next_id[0] += n
        return out

    def shown_in(k, s):   # births at k = 1 + s; one person gone from k = 3 in scene 1
        n = np.arange(8) if k <= s else np.arange(12)
        return np.delete(n, 4) if k >= 3 and s == 1 else n

    with PoseBank(eng, P) as a, PoseBank(eng, P) as b0, PoseBank(eng, P) as b1, PoseBank(eng, P) as b2:
        twins = [b0, b1, b2]
        listed = []
        for s in range(S):   # everybody's first sighting: the loop starts with tracks to match
            z = (centres[s][:6] + rng.normal(0, 0.03, (6, P, 2))).astype(f32)
            t = fresh(6)
            a.step(t, z)
            twins[s].step(t, z)
            listed.append(t)
        births = coasted = 0
        for k in range(5):
            frame = []
            for s in range(S):
                shown = shown_in(k, s)
                z = (centres[s][shown] + rng.normal(0, 0.03, (len(shown), P, 2))).astype(f32)
                frame.append((listed[s], z, rng.random((len(shown), P)) >= 0.2))
            new = fresh(sum(len(f[1]) for f in frame))
            got = a.track_batch(frame, new)
            assert a.last_associate_batch()["launches"] == 3, k
            used = 0
            for s in range(S):
                assert twins[s].order().tolist() == listed[s].tolist(), (k, s)
                want = twins[s].track(frame[s][1], new[used:], present=frame[s][2])
                assert (got[s] == want).all(), (k, s)
                born = want[np.isin(want, new)]
                coasted += len(np.setdiff1d(listed[s], want))
                used += len(born)
                births += len(born)
                listed[s] = np.concatenate([listed[s], born])
                for t in listed[s]:
                    x, y = a.state(t), twins[s].state(t)
                    assert (x[0] == y[0]).all() and bits(x[1], y[1]) and bits(x[2], y[2]), (k, s, t)
        assert births >= 12 and coasted >= 2 and len(a) == sum(len(t) for t in listed)
        assert a.order().tolist() == sorted(a.order().tolist(), key=lambda t: int(t))   # new ids went out in scene order, then pose order


# ---- 9. refusals -------------------------------------------------------------------------------------
def test_every_refusal_leaves_everything_as_it_was(eng):
    P = 17
    scs = scenes_of(P, crowd=True, shapes=[(3, 5), (17, 70)])
    lib = eng.lib
    with fill(PoseBank(eng, P), scs) as bank:
        tids = ids_of(scs)
        every = np.concatenate(tids)
        want = bank.associate_batch(call_of(scs))
        before = [bank.state(i) for i in every]
        m = sum(sc.m for sc in scs)
        z = np.ascontiguousarray(np.concatenate([sc.poses for sc in scs]))
        zp = z.ctypes.data_as(C.POINTER(C.c_float))
        out_t, out_w, out_r = np.full(m, 77, u64), np.full(m, 5.0, f32), np.full(2, 9, u32)
        tp, wp, rp = out_t.ctypes.data_as(C.POINTER(C.c_uint64)), out_w.ctypes.data_as(C.POINTER(C.c_float)), out_r.ctypes.data_as(C.POINTER(C.c_uint32))

        def rows(size=40, comps=2, host=zp, dev=None):
            return C.byref(sa_point_rows(size, comps, 0.0, 0, host, None, dev))

        def opts(size=16, min_common=1, threshold=1.0):
            return C.byref(PS.sa_pose_options(size, min_common, threshold, 0))

        def arr(v, t=u64):
            a = np.array(v, t)
            return a.ctypes.data_as(C.POINTER(C.c_uint64 if t is u64 else C.c_uint32)), a

        good = arr(every)
        tc, pc = arr([5, 70], u32), arr([3, 17], u32)
        in_two = arr(np.concatenate([tids[0], tids[1][:69], tids[0][:1]]))       # the first scene's first track again in the second
        zero = arr(np.concatenate([tids[0], np.zeros(1, u64), tids[1][1:]]))
        unknown = arr(np.concatenate([tids[0], tids[1][:69], np.full(1, 9999, u64)]))
        many_c = arr(np.zeros(65536, u32), u32)
        big_tc = arr([5, 2049], u32)
        d = DeviceRows(0x1000, m, P * 2, SA_ELEM_F32).struct()
        B, NF, U = abi.SA_ERR_BAD_ARG, abi.SA_ERR_NOT_FOUND, abi.SA_ERR_UNSUPPORTED
        f = lib.sa_points_associate_batch
        cases = [
            (B, "twice", lambda: f(bank.h, 2, tc[0], in_two[0], pc[0], rows(), opts(), tp, wp, rp, None)),
            (B, "id 0", lambda: f(bank.h, 2, tc[0], zero[0], pc[0], rows(), opts(), tp, wp, rp, None)),
            (NF, "unknown", lambda: f(bank.h, 2, tc[0], unknown[0], pc[0], rows(), opts(), tp, wp, rp, None)),
            (B, "null", lambda: f(bank.h, 2, None, good[0], pc[0], rows(), opts(), tp, wp, rp, None)),
            (B, "null", lambda: f(bank.h, 2, tc[0], good[0], None, rows(), opts(), tp, wp, rp, None)),
            (B, "null", lambda: f(bank.h, 2, tc[0], None, pc[0], rows(), opts(), tp, wp, rp, None)),
            (B, "min_common", lambda: f(bank.h, 2, tc[0], good[0], pc[0], rows(), opts(min_common=0), tp, wp, rp, None)),
            (B, "threshold", lambda: f(bank.h, 2, tc[0], good[0], pc[0], rows(), opts(threshold=float("nan")), tp, wp, rp, None)),
            (B, "threshold", lambda: f(bank.h, 2, tc[0], good[0], pc[0], rows(), opts(threshold=float("inf")), tp, wp, rp, None)),
            (B, "threshold", lambda: f(bank.h, 2, tc[0], good[0], pc[0], rows(), opts(threshold=-0.5), tp, wp, rp, None)),
            (B, "struct_size", lambda: f(bank.h, 2, tc[0], good[0], pc[0], rows(), opts(size=12), tp, wp, rp, None)),
            (B, "struct_size", lambda: f(bank.h, 2, tc[0], good[0], pc[0], rows(size=32), opts(), tp, wp, rp, None)),
            (B, "null options", lambda: f(bank.h, 2, tc[0], good[0], pc[0], rows(), None, tp, wp, rp, None)),
            (B, "null rows", lambda: f(bank.h, 2, tc[0], good[0], pc[0], None, opts(), tp, wp, rp, None)),
            (B, "null", lambda: f(bank.h, 2, tc[0], good[0], pc[0], rows(), opts(), None, wp, rp, None)),
            (B, "null", lambda: f(bank.h, 2, tc[0], good[0], pc[0], rows(), opts(), tp, None, rp, None)),
            (B, "comps", lambda: f(bank.h, 2, tc[0], good[0], pc[0], rows(comps=4), opts(), tp, wp, rp, None)),
            (B, "exactly one", lambda: f(bank.h, 2, tc[0], good[0], pc[0], rows(host=None), opts(), tp, wp, rp, None)),
            (B, "", lambda: f(bank.h, 2, tc[0], good[0], pc[0], rows(host=None, dev=C.pointer(d)), opts(), tp, wp, rp, None)),   # a span in no registered block
            (U, "scenes", lambda: f(bank.h, 65536, many_c[0], good[0], many_c[0], rows(), opts(), tp, wp, rp, None)),
            (U, "scene 1", lambda: f(bank.h, 2, big_tc[0], good[0], pc[0], rows(), opts(), tp, wp, rp, None)),
        ]
        for k, (code, word, call) in enumerate(cases):
            assert call() == code, k
            assert word in lib.sa_last_error(eng.h).decode(), k
            st = bank.last_associate_batch()
            assert st["launches"] == 0 and st["scenes"] == 0 and st["poses"] == 0, k   # zeros after a refused call
            assert (out_t == 77).all() and (out_w == 5.0).all() and (out_r == 9).all(), k
            got = bank.associate_batch(call_of(scs))   # the next good call works
            assert bank.last_associate_batch()["launches"] == 3, k
            for s in range(2):
                assert (got[s][0] == want[s][0]).all() and bits(got[s][1], want[s][1]), (k, s)
        for x, i in zip(before, every):
            y = bank.state(i)
            assert (x[0] == y[0]).all() and bits(x[1], y[1]) and bits(x[2], y[2])
        # nothing to match: SA_OK without a launch
        last = bank.last_associate_batch
        assert f(bank.h, 0, tc[0], good[0], pc[0], rows(), opts(), tp, wp, None, None) == 0 and last()["launches"] == 0
        assert f(bank.h, 0, None, None, None, None, opts(), None, None, None, None) == 0 and last()["launches"] == 0
        no_pose = arr([0, 0], u32)
        assert f(bank.h, 2, tc[0], good[0], no_pose[0], None, opts(), None, None, rp, None) == 0 and last()["launches"] == 0
        assert (out_t == 77).all() and (out_w == 5.0).all() and (out_r == 0).all()
        no_track = arr([0, 0], u32)
        assert f(bank.h, 2, no_track[0], good[0], pc[0], rows(), opts(), tp, wp, None, None) == 0
        assert (last()["launches"], last()["scenes"], last()["poses"], last()["tracks"]) == (0, 2, m, 0)
        assert (out_t == 0).all() and np.isnan(out_w).all()
    with PoseBank(eng, P) as empty:   # a bank without tracks
        got = empty.associate_batch([([], scs[0].poses), ([], scs[1].poses)])
        assert all((g[0] == 0).all() and np.isnan(g[1]).all() for g in got) and empty.last_associate_batch()["launches"] == 0
