"""The keypoint frame loop in one call on the MI355X (PoseTrackBank.track / track_batch over include/similari_pose_track.h): the call
returns, and leaves in the bank, the bits of the sequence it replaces — PoseBank.track / track_batch: one associate, one step, one
predict —, which a twin bank on the same engine runs on the same frames.  Equal means equal: ids, the order of the bank, and every
state bit for bit (two NaNs count as the same bits, as everywhere in these tests); the route of the vote is deterministic, so no tie is
excluded.  One test compares with the numpy models alone (tests/points_ref.py stepped by the matches of tests/pose_ref.py's
kuhn_munkres) on a frame where the CPU first shows that every row of the optimum is forced.

Shapes: the scenes of tests/test_gpu_pose_batch.py, (m, T) = (1, 1), (3, 5), (0, 4), (17, 70), (4, 0), (70, 17), (17, 65), with
P in {1, 17, 65}: a scene without poses, one without tracks, several tiles, the 64-point chunk crossed; 150 x 150 crowds for the dense
search; 300 scenes for the scan over more scenes than threads; 2048 x 2048 for the limits."""
import ctypes as C

import numpy as np
import pytest

import devrows_ref as dref
import points_ref as R
import pose_ref as PR
from similari_amd import abi
from similari_amd import pose as PS
from similari_amd import pose_track as PT
from similari_amd.devrows import DeviceRows
from similari_amd.engine import Engine, EngineError
from similari_amd.f16 import SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_F32
from similari_amd.points import SA_ROW_NONE, sa_point_rows
from similari_amd.pose import PoseBank
from similari_amd.pose_track import PoseTrackBank
from test_gpu_points import Model, bits, check_states, device_block, to_source
from test_gpu_pose import scene
from test_gpu_pose_batch import OFF, SHAPES, SeededScene, call_of, fill, ids_of, scenes_of

pytestmark = pytest.mark.gpu
f32, u8, u32, u64 = np.float32, np.uint8, np.uint32, np.uint64


@pytest.fixture(scope="module")
def eng():
    e = Engine(abi.make_config(positional="iou", positional_threshold=0.3, device=0))
    yield e
    e.close()


def same_states(a, b, ids=None):
    """the two banks hold the same tracks in the same order, and the listed (None: all) states are equal bit for bit"""
    assert a.order().tolist() == b.order().tolist()
    for t in a.order() if ids is None else ids:
        x, y = a.state(t), b.state(t)
        assert (x[0] == y[0]).all() and bits(x[1], y[1]) and bits(x[2], y[2]), t


def sequence(bank, ids, pts, new_ids, present=None, coast=True, **kw):
    """The sequence the call replaces, for a list of tracks of the caller's: associate, step, predict -> (ids, weights)"""
    got, w = bank.associate(pts, present=present, ids=ids, **kw)
    fresh = np.flatnonzero(got == 0)
    listed = bank.order() if ids is None else np.asarray(ids, u64)
    idle = np.setdiff1d(listed, got[got != 0]) if coast else np.zeros(0, u64)
    got[fresh] = np.asarray(new_ids, u64)[: len(fresh)]
    if len(got):
        bank.step(got, pts, present=present, min_score=kw.get("min_score", 0.0))
    if len(idle):
        bank.predict(idle)
    return got, w


def twin_track_batch(b, frame, new):
    """PoseBank.track_batch for the twin.  It takes no scene without poses (it reshapes the scene's empty array with an open dimension),
    and all such a scene adds to the sequence is that its tracks coast: they get a predict of their own, which leaves the same bits,
    because no state is in both predicts."""
    full = [f for f in frame if len(f[1])]
    got = iter(b.track_batch(full, new) if full else [])
    idle = [f[0] for f in frame if not len(f[1]) and len(f[0])]
    if idle:
        b.predict(np.concatenate(idle))
    return [next(got) if len(f[1]) else np.zeros(0, u64) for f in frame]


class Crowd:
    """People of one camera and what the tracker is shown of them frame after frame: scene s of SHAPES starts with T tracks and
    shows m poses per frame, drawn from max(m, T) + 3 people, so every frame some are born, some are missed and coast, some left."""

    def __init__(self, rng, s, m, T, P):
        self.m, self.P = m, P
        n = max(m, T) + 3
        self.centres = PR.people(rng, n, P, bool(s % 2)) + 400.0 * s
        self.listed = np.arange(1, T + 1, dtype=u64) + u64(OFF * (s + 1))
        self.first = [((self.centres[:T] + rng.normal(0, 0.03, (T, P, 2))).astype(f32), rng.random((T, P)) >= 0.3) for _ in range(2)]

    def frame(self, rng):
        shown = rng.permutation(len(self.centres))[: self.m]
        z = (self.centres[shown] + rng.normal(0, 0.04, (self.m, self.P, 2))).astype(f32)
        return (self.listed, z, rng.random((self.m, self.P)) >= 0.25)

    def born(self, ids, new):
        self.listed = np.concatenate([self.listed, ids[np.isin(ids, new)]])


# ---- 1. twin banks over five frames --------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 17, 65])
def test_track_batch_leaves_the_bits_of_the_three_calls(eng, P):
    rng = np.random.default_rng(500 + P)
    cams = [Crowd(rng, s, m, T, P) for s, (m, T) in enumerate(SHAPES)]
    with PoseTrackBank(eng, P) as a, PoseBank(eng, P) as b:
        for cam in cams:
            for z, pres in cam.first:
                if len(cam.listed):
                    a.step(cam.listed, z, present=pres)
                    b.step(cam.listed, z, present=pres)
        next_id, created, coasted = 7, 0, 0
        for k in range(5):
            if k == 3:   # somebody leaves for good: the caller drops the track
                gone = cams[3].listed[:2]
                a.remove(gone)
                b.remove(gone)
                cams[3].listed = cams[3].listed[2:]
            frame = [cam.frame(rng) for cam in cams]
            m = sum(cam.m for cam in cams)
            new = np.arange(next_id, next_id + m, dtype=u64)
            want_w = np.concatenate([g[1] for g in b.associate_batch(frame)])
            roots = b.last_associate_batch()["scene_roots"].copy()
            want = twin_track_batch(b, frame, new)
            got = a.track_batch(frame, next_id)   # a first id: m consecutive ones are offered
            st = a.last_track()
            for s, cam in enumerate(cams):
                assert (got[s] == want[s]).all() and got[s].dtype == u64 and (got[s] != 0).all(), (k, s)
                cam.born(got[s], new)
            assert bits(a.last_weights(), want_w), k
            same_states(a, b)
            n = sum(len(f[0]) for f in frame)
            assert (st["scenes"], st["poses"], st["tracks"], st["vote_launches"], st["step_launches"]) == (len(cams), m, n, 3, 2), k
            assert (st["scene_roots"] == roots).all() and st["roots"] == int(roots.sum())
            assert st["matched"] + st["created"] == m and st["coasted"] == n - st["matched"]
            assert st["created"] == int(np.isin(np.concatenate(got), new).sum())
            assert st["bytes_h2d"] == 32 * len(cams) + 4 * n + m * P * 2 * 4 + m * P and st["bytes_d2h"] == 8 * m + 4 * len(cams)
            next_id += st["created"]
            created += st["created"]
            coasted += st["coasted"]
        assert created >= 20 and coasted >= 20 and len(a) == sum(len(cam.listed) for cam in cams)


@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("m,T", [(3, 5), (17, 70), (70, 17)])
@pytest.mark.parametrize("P", [1, 17, 65])
def test_track_leaves_the_bits_of_the_three_calls(eng, P, m, T, permuted):
    rng = np.random.default_rng(900 + 7 * P + m)
    cam = Crowd(rng, int(permuted), m, T, P)   # people apart for the bank's own order, a crowd for the caller's list
    with PoseTrackBank(eng, P) as a, PoseBank(eng, P) as b:
        for z, pres in cam.first:
            a.step(cam.listed, z, present=pres)
            b.step(cam.listed, z, present=pres)
        next_id = 3
        for k in range(5):
            _, z, pres = cam.frame(rng)
            new = np.arange(next_id, next_id + m, dtype=u64)
            if permuted:   # the caller's own list, in an order of the caller's: all but one track of the bank
                ids = rng.permutation(a.order())[1:]
                want, want_w = sequence(b, ids, z, new, present=pres)
                got, xy = a.track(z, new, present=pres, track_ids=ids, xy=True)
                assert bits(xy, np.stack([b.state(t)[1][:, :2] for t in got])), k   # the step's out_xy: the means it left
            else:
                want_w = b.associate(z, present=pres)[1]
                want = b.track(z, new, present=pres)
                got = a.track(z, next_id, present=pres)
            st = a.last_track()
            assert (got == want).all() and bits(a.last_weights(), want_w), k
            same_states(a, b)
            assert (st["vote_launches"], st["step_launches"], st["scenes"], st["poses"]) == (3, 1, 1, m), k
            assert st["created"] == int(np.isin(got, new).sum()) and st["matched"] == m - st["created"]
            next_id += st["created"]
        assert len(a) > T or permuted   # people apart: whoever is shown first is born (in a crowd a pose may find a neighbour's track)


# ---- 2. against the model, independent of the code under test ------------------------------------------
def forced_scenes(P):
    """Three sparse scenes in which every row of kuhn_munkres's optimum is forced (forbidding its cell lowers the total), the seed
    found on the CPU from the model alone."""
    for seed in range(20, 40):
        scs = [SeededScene(m, T, P, False, seed * 10 + k) for k, (m, T) in enumerate([(3, 5), (17, 70), (70, 17)])]
        votes = [PR.vote(PR.weights(sc.poses, sc.pres, sc.model.has, sc.model.mean, sc.model.cov)) for sc in scs]
        if all(PR.forced_rows(wq, total, ref.copy()).all() for total, ref, wq, thr_q in votes):
            return scs, [v[1] for v in votes]
    raise AssertionError("no seed gives three scenes whose optimum is unique")


def test_states_against_the_models(eng):
    P = 17
    scs, refs = forced_scenes(P)   # (asserted on the CPU, before any GPU call: 100 % of the rows are compared)
    assert sum(int((r >= 0).sum()) for r in refs) >= 20 and sum(int((r < 0).sum()) for r in refs) >= 5
    tids = ids_of(scs)
    mdl = Model(P, cap=256)
    for sc, t in zip(scs, tids):
        for z, pres in sc.rounds:
            mdl.call("step", t, z, pres, create=True)
        mdl.b.cov[mdl.row[int(t[sc.seeded[0]])], sc.seeded[1]] = sc.model.cov[sc.seeded]
    new = np.arange(1, 1 + sum(sc.m for sc in scs), dtype=u64)
    want, used = [], 0
    for sc, t, ref in zip(scs, tids, refs):
        ids = np.where(ref >= 0, t[np.maximum(ref, 0)], 0).astype(u64)
        fresh = np.flatnonzero(ids == 0)
        ids[fresh] = new[used: used + len(fresh)]
        used += len(fresh)
        want.append(ids)
    every = np.concatenate(want)
    mdl.call("step", every, np.concatenate([sc.poses for sc in scs]), np.concatenate([sc.pres for sc in scs]), create=True)
    mdl.call("predict", np.setdiff1d(np.concatenate(tids), every))
    with fill(PoseTrackBank(eng, P), scs) as bank:
        got = bank.track_batch(call_of(scs), new)
        for s in range(len(scs)):
            assert (got[s] == want[s]).all(), s
        check_states(bank, mdl)
        assert bank.last_track()["created"] == used


# ---- 3. a crowd ----------------------------------------------------------------------------------------
def test_three_crowds_beside_two_sparse_scenes(eng):
    P = 2
    crowds = [SeededScene(150, 150, P, True, seed) for seed in (31, 32, 33)]
    scs = [crowds[0], scene(3, 5, P), crowds[1], scene(17, 70, P), crowds[2]]
    for sc in crowds:   # on the CPU, from the model alone: is this a crowd at all?
        total, ref, wq, thr_q = sc.vote()
        assert PR.greedy_roots(wq, thr_q) >= 1, "the scene is no crowd: the dense search would not run"
    m = sum(sc.m for sc in scs)
    with fill(PoseTrackBank(eng, P), scs) as a, fill(PoseBank(eng, P), scs) as b:
        b.associate_batch(call_of(scs))
        roots = b.last_associate_batch()["scene_roots"].copy()
        want = b.track_batch(call_of(scs), np.arange(1, m + 1, dtype=u64))
        got = a.track_batch(call_of(scs), 1)
        st = a.last_track()
        assert (st["scene_roots"] == roots).all() and all(roots[s] >= 1 for s in (0, 2, 4))
        assert all((g == w).all() for g, w in zip(got, want))
        same_states(a, b)


# ---- 4. growth inside the call -------------------------------------------------------------------------
def test_the_planes_grow_inside_the_call(eng):
    P = 17
    rng = np.random.default_rng(4)
    centres = PR.people(rng, 60, P, False)
    ids = np.arange(1, 61, dtype=u64)
    poses = (9000.0 + 20.0 * np.arange(10)[:, None, None] + rng.uniform(-3, 3, (10, P, 2))).astype(f32)   # nobody the bank knows
    with PoseTrackBank(eng, P) as a, PoseBank(eng, P) as b:
        for bank in (a, b):
            for z, pres in PR.track_rounds(np.random.default_rng(5), centres, rounds=2):
                bank.step(ids, z, present=pres)
            assert bank.last()["capacity"] == 64
        want = b.track(poses, np.arange(100, 110, dtype=u64))
        got = a.track(poses, 100)
        assert got.tolist() == want.tolist() == list(range(100, 110))   # the created ids in pose order
        assert a.last_track()["created"] == 10 and a.last_track()["matched"] == 0 and a.last_track()["coasted"] == 60
        a.distance(ids[:1], poses[:1])   # (changes no state; its record shows the capacity)
        assert a.last()["capacity"] == 128
        same_states(a, b)
        assert len(a) == 70


# ---- 5. the edges --------------------------------------------------------------------------------------
def test_the_edges(eng):
    P = 17
    sc = scene(17, 70, P)
    with PoseTrackBank(eng, P) as a, PoseBank(eng, P) as b:
        # an empty bank: every pose creates a track, nothing votes
        poses = sc.poses.copy()
        poses[4] = np.nan                      # a pose whose points are all absent: a track without a state
        pres = sc.pres.copy()
        pres[6] = False                        # the same through the mask
        new = np.arange(1, 18, dtype=u64)
        assert (a.track(poses, new, present=pres) == new).all() and (b.track(poses, new, present=pres) == new).all()
        st = a.last_track()
        assert (st["vote_launches"], st["step_launches"], st["created"], st["matched"], st["coasted"], st["tracks"]) == (0, 1, 17, 0, 0, 0)
        assert np.isnan(a.last_weights()).all() and st["bytes_d2h"] == 0
        assert not a.state(5)[0].any() and not a.state(7)[0].any() and a.state(1)[0].any()
        same_states(a, b)
        # m == 0 with coast: a predict over the listed tracks, and only those
        listed = new[:9]
        got = a.track(np.zeros((0, P, 2), f32), 50, track_ids=listed)
        b.predict(listed)
        st = a.last_track()
        assert len(got) == 0 and (st["vote_launches"], st["step_launches"], st["created"], st["coasted"], st["poses"]) == (0, 1, 0, 9, 0)
        same_states(a, b)
        # ... and without coast: nothing at all
        a.track(np.zeros((0, P, 2), f32), 50, track_ids=listed, coast=False)
        assert a.last_track()["step_launches"] == 0 and a.last_track()["coasted"] == 0
        same_states(a, b)
        # coast=False: the tracks nobody matched keep their state; an unlisted track is untouched either way
        z = (sc.poses + f32(0.01)).astype(f32)
        for coast in (False, True):
            unlisted = [a.state(t) for t in new[9:]]
            want, _ = sequence(b, listed, z[:5], np.arange(60, 65, dtype=u64) + u64(10 * coast), present=sc.pres[:5], coast=coast)
            got = a.track(z[:5], 60 + 10 * coast, present=sc.pres[:5], track_ids=listed, coast=coast)
            assert (got == want).all()
            same_states(a, b)
            for t, x in zip(new[9:], unlisted):
                y = a.state(t)
                assert (x[0] == y[0]).all() and bits(x[1], y[1]) and bits(x[2], y[2]), t
            assert a.last_track()["coasted"] == (9 - a.last_track()["matched"] if coast else 0)
        # a batch in which nobody has a track to be matched to: poses only where there are no tracks
        frame = [(listed[:4], np.zeros((0, P, 2), f32)), (np.zeros(0, u64), z[:3])]
        want = twin_track_batch(b, frame, np.arange(90, 93, dtype=u64))
        got = a.track_batch(frame, 90)
        st = a.last_track()
        assert all((g == w).all() for g, w in zip(got, want)) and got[1].tolist() == [90, 91, 92]
        assert (st["vote_launches"], st["step_launches"], st["created"], st["coasted"]) == (0, 1, 3, 4)
        same_states(a, b)
        # no scenes at all
        assert a.track_batch([], 200) == [] and a.last_track()["step_launches"] == 0


# ---- 6. poses in device memory -------------------------------------------------------------------------
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
    new = np.arange(1, m + 1, dtype=u64)
    with fill(PoseTrackBank(eng, P), scs) as bank, fill(PoseBank(eng, P), scs) as twin, device_block(eng, src) as ptr:
        rows = DeviceRows(ptr + off * eb, B, W, elem, index)
        dev = bank.track_batch(None, new, rows=rows, track_ids=tids, pose_counts=counts, present=pres, comps=comps, min_score=0.4, xy=True)
        st = bank.last_track()
        host = twin.track_batch([(t, zs, ms) for t, zs, ms in zip(tids, np.split(z, ends), np.split(mask, ends))], new, min_score=0.4)
        for s in range(3):
            assert (dev[s][0] == host[s]).all(), s
            assert bits(dev[s][1], np.stack([twin.state(t)[1][:, :2] for t in host[s]])), s
        same_states(bank, twin)
        T = sum(sc.T for sc in scs)
        assert st["matched"] >= 10 and st["created"] >= 4 and not bank.state(dev[0][0][3])[0].any()   # SA_ROW_NONE: a track without a state
        assert st["bytes_h2d"] == 32 * 3 + 4 * T + m * 4 + m * P and st["src_bytes"] == int(got.sum()) * L * eb   # no pose bytes
        assert st["bytes_d2h"] == 8 * m + 4 * 3 + m * P * 8
        # the single form, without an index and without a mask: pose i is row i
        one, one_twin = np.arange(500, 620, dtype=u64), np.arange(500, 620, dtype=u64)
        want = twin.track(np.ascontiguousarray(wide), one_twin, min_score=0.4)
        got1 = bank.track(None, one, rows=DeviceRows(ptr + off * eb, B, W, elem), comps=comps, min_score=0.4)
        assert (got1 == want).all() and bank.last_track()["bytes_h2d"] == 0
        same_states(bank, twin)


# ---- 7. launch counts and limits -----------------------------------------------------------------------
def test_300_small_scenes_equal_the_twin(eng):
    P, S = 3, 300
    rng = np.random.default_rng(300)
    ms, ns = rng.integers(1, 6, S), rng.integers(1, 6, S)
    centres = [PR.people(rng, int(n), P, bool(s % 2)) + 20.0 * s for s, n in enumerate(ns)]
    ids = [np.arange(1, n + 1, dtype=u64) + u64(OFF * (s + 1)) for s, n in enumerate(ns)]
    rounds = PR.track_rounds(rng, np.concatenate(centres))
    frame = [(t,) + PR.poses_of(rng, c, int(m)) for t, c, m in zip(ids, centres, ms)]
    m = int(ms.sum())
    with PoseTrackBank(eng, P) as a, PoseBank(eng, P) as b:
        for z, pres in rounds:
            a.step(np.concatenate(ids), z, present=pres)
            b.step(np.concatenate(ids), z, present=pres)
        want = b.track_batch(frame, np.arange(1, m + 1, dtype=u64))
        got = a.track_batch(frame, 1)
        st = a.last_track()
        assert all((g == w).all() for g, w in zip(got, want))
        assert (st["vote_launches"], st["step_launches"], st["scenes"], st["poses"], st["tracks"]) == (3, 2, S, m, int(ns.sum()))
        assert st["created"] >= S // 8 and st["matched"] > S // 2
        same_states(a, b)
        got = a.track_batch(frame[:1], 5000)   # one scene is a batch all the same: two launches behind the vote
        assert a.last_track()["step_launches"] == 2
        assert (got[0] == b.track_batch(frame[:1], np.arange(5000, 5006, dtype=u64))[0]).all()
        same_states(a, b, ids[0])


def test_2048_by_2048_and_one_beyond(eng):
    P, n = 2, PS.SA_POSE_MAX
    rng = np.random.default_rng(2048)
    centres = PR.people(rng, n + 1, P, False)
    ids = np.arange(1, n + 2, dtype=u64)
    poses, pres = PR.poses_of(rng, centres[:n], n)
    with PoseTrackBank(eng, P) as a, PoseBank(eng, P) as b:
        for z, mask in PR.track_rounds(rng, centres[:n], rounds=2):
            a.step(ids[:n], z, present=mask)
            b.step(ids[:n], z, present=mask)
        want = b.track(poses, np.arange(10000, 10000 + n, dtype=u64), present=pres)
        got = a.track(poses, 10000, present=pres)
        st = a.last_track()
        assert (got == want).all() and st["matched"] > 1000 and st["created"] > 100 and st["step_launches"] == 1
        same_states(a, b, ids[:n: 37])
        order = a.order().tolist()
        # one beyond, either way: 2049 poses; every track of a bank that now holds more than 2048
        more = np.concatenate([poses, poses[:1]])
        for call in (lambda: a.track(more, 20000, track_ids=ids[:n]), lambda: a.track(poses, 20000),
                     lambda: a.track_batch([(ids[:n], more)], 20000), lambda: a.track_batch([(a.order()[: n + 1], poses)], 20000)):
            with pytest.raises(EngineError) as ei:
                call()
            assert ei.value.code == abi.SA_ERR_UNSUPPORTED and a.last_track()["poses"] == 0 and a.order().tolist() == order
        # the next good call works
        z = (poses + f32(0.01)).astype(f32)
        want, _ = sequence(b, ids[:n], z, np.arange(30000, 30000 + n, dtype=u64), present=pres)
        got = a.track(z, 30000, present=pres, track_ids=ids[:n])
        assert (got == want).all()
        same_states(a, b, a.order()[:: 41])


# ---- 8. refusals ---------------------------------------------------------------------------------------
def test_every_refusal_leaves_everything_as_it_was(eng):
    P = 17
    scs = scenes_of(P, crowd=True, shapes=[(3, 5), (17, 70)])
    lib = eng.lib
    with fill(PoseTrackBank(eng, P), scs) as bank:
        tids = ids_of(scs)
        every = np.concatenate(tids)
        bank.associate(scs[1].poses, present=scs[1].pres, ids=tids[1])
        bank.associate_batch(call_of(scs))
        records = (bank.last(), bank.last_associate(), bank.last_associate_batch())
        records[2].pop("scene_roots")
        order = bank.order().tolist()
        before = [bank.state(i) for i in every]
        m = sum(sc.m for sc in scs)
        z = np.ascontiguousarray(np.concatenate([sc.poses for sc in scs]))
        zp = z.ctypes.data_as(C.POINTER(C.c_float))
        out_t, out_w, out_xy, out_r, out_c = np.full(m, 77, u64), np.full(m, 5.0, f32), np.full((m, P, 2), 3.0, f32), np.full(2, 9, u32), C.c_uint32(55)
        tp, wp, rp = out_t.ctypes.data_as(C.POINTER(C.c_uint64)), out_w.ctypes.data_as(C.POINTER(C.c_float)), out_r.ctypes.data_as(C.POINTER(C.c_uint32))
        xp, cp = out_xy.ctypes.data_as(C.POINTER(C.c_float)), C.byref(out_c)

        def rows(size=40, comps=2, host=zp, dev=None):
            return C.byref(sa_point_rows(size, comps, 0.0, 0, host, None, dev))

        def opts(size=16, min_common=1, threshold=1.0, coast=1):
            return C.byref(PT.sa_pose_track_options(size, min_common, threshold, coast))

        def arr(v, t=u64):
            a = np.array(v, t)
            return a.ctypes.data_as(C.POINTER(C.c_uint64 if t is u64 else C.c_uint32)), a

        good, new = arr(every), arr(np.arange(1, m + 1))
        tc, pc = arr([5, 70], u32), arr([3, 17], u32)
        in_two = arr(np.concatenate([tids[0], tids[1][:69], tids[0][:1]]))       # the first scene's first track again in the second
        zero = arr(np.concatenate([tids[0], np.zeros(1, u64), tids[1][1:]]))
        unknown = arr(np.concatenate([tids[0], tids[1][:69], np.full(1, 9999, u64)]))
        new_zero, new_twice = arr(np.concatenate([new[1][:7], [0], new[1][8:]])), arr(np.concatenate([new[1][:19], new[1][:1]]))
        new_held, new_listed = arr(np.concatenate([new[1][:19], tids[1][3:4]])), arr(np.concatenate([tids[0][:1], new[1][1:]]))
        many_c = arr(np.zeros(65536, u32), u32)
        big_tc, big_pc = arr([5, 2049], u32), arr([2049, 17], u32)
        d = DeviceRows(0x1000, m, P * 2, SA_ELEM_F32).struct()
        B, NF, U = abi.SA_ERR_BAD_ARG, abi.SA_ERR_NOT_FOUND, abi.SA_ERR_UNSUPPORTED
        f, g = lib.sa_points_track_batch, lib.sa_points_track

        def fb(S=2, tc=tc, ids=good, pc=pc, r=None, n_new=m, nw=new, o=None, t=tp, w=wp, c=cp):
            return lambda: f(bank.h, S, tc[0], ids[0], pc[0], r if r is not None else rows(), n_new, nw[0], o if o is not None else opts(), t, w, xp, rp, c)

        def gs(n=75, ids=good, m1=m, r=None, n_new=m, nw=new, o=None, t=tp, w=wp, c=cp):
            return lambda: g(bank.h, n, ids[0], m1, r if r is not None else rows(), n_new, nw[0], o if o is not None else opts(), t, w, xp, c)

        null = (None,)
        cases = [
            (B, "twice", fb(ids=in_two)), (B, "id 0", fb(ids=zero)), (NF, "unknown", fb(ids=unknown)),
            (B, "null", fb(tc=null)), (B, "null", fb(pc=null)), (B, "null", fb(ids=null)),
            (B, "min_common", fb(o=opts(min_common=0))), (B, "threshold", fb(o=opts(threshold=float("nan")))),
            (B, "threshold", fb(o=opts(threshold=float("inf")))), (B, "threshold", fb(o=opts(threshold=-0.5))),
            (B, "coast", fb(o=opts(coast=2))), (B, "struct_size", fb(o=opts(size=12))), (B, "struct_size", fb(r=rows(size=32))),
            (B, "null options", lambda: f(bank.h, 2, tc[0], good[0], pc[0], rows(), m, new[0], None, tp, wp, xp, rp, cp)),
            (B, "null rows", lambda: f(bank.h, 2, tc[0], good[0], pc[0], None, m, new[0], opts(), tp, wp, xp, rp, cp)),
            (B, "null", fb(t=None)), (B, "null", fb(w=None)), (B, "out_created", fb(c=None)),
            (B, "comps", fb(r=rows(comps=4))), (B, "exactly one", fb(r=rows(host=None))),
            (B, "", fb(r=rows(host=None, dev=C.pointer(d)))),   # a span in no registered block
            (U, "scenes", fb(S=65536, tc=many_c, pc=many_c)), (U, "scene 1", fb(tc=big_tc)), (U, "scene 0", fb(pc=big_pc, n_new=2066)),
            (B, "%d new ids for %d poses" % (m - 1, m), fb(n_new=m - 1)), (B, "null new ids", fb(nw=null)),
            (B, "new id 0", fb(nw=new_zero)), (B, "twice", fb(nw=new_twice)),
            (B, "is a track of the bank", fb(nw=new_held)), (B, "is a track of the bank", fb(nw=new_listed)),
            # the single form
            (B, "twice", gs(ids=in_two)), (B, "id 0", gs(ids=zero)), (NF, "unknown", gs(ids=unknown)),
            (B, "min_common", gs(o=opts(min_common=0))), (B, "coast", gs(o=opts(coast=7))), (B, "struct_size", gs(o=opts(size=20))),
            (B, "null rows", lambda: g(bank.h, 75, good[0], m, None, m, new[0], opts(), tp, wp, xp, cp)),
            (B, "null", gs(t=None)), (B, "out_created", gs(c=None)), (B, "comps", gs(r=rows(comps=1))),
            (B, "%d new ids for %d poses" % (0, m), gs(n_new=0)), (B, "null new ids", gs(nw=null)),
            (B, "new id 0", gs(nw=new_zero)), (B, "twice", gs(nw=new_twice)), (B, "is a track of the bank", gs(nw=new_held)),
            (U, "at most", gs(m1=2049, n_new=2049)),
        ]
        for k, (code, word, call) in enumerate(cases):
            assert call() == code, (k, lib.sa_last_error(eng.h).decode())
            assert word in lib.sa_last_error(eng.h).decode(), (k, lib.sa_last_error(eng.h).decode())
            st = bank.last_track()
            assert st["vote_launches"] == 0 and st["step_launches"] == 0 and st["scenes"] == 0 and st["poses"] == 0, k   # zeros after a refused call
            assert (out_t == 77).all() and (out_w == 5.0).all() and (out_xy == 3.0).all() and (out_r == 9).all() and out_c.value == 55, k
            assert bank.order().tolist() == order, k
        now = (bank.last(), bank.last_associate(), bank.last_associate_batch())
        now[2].pop("scene_roots")
        assert now == records   # the three older records
        for x, i in zip(before, every):
            y = bank.state(i)
            assert (x[0] == y[0]).all() and bits(x[1], y[1]) and bits(x[2], y[2])
        # the next good call works, and leaves the older records alone
        with fill(PoseBank(eng, P), scs) as twin:
            want = twin.track_batch(call_of(scs), new[1])
            got = bank.track_batch(call_of(scs), new[1])
            assert all((a == b).all() for a, b in zip(got, want))
            same_states(bank, twin)
        now = (bank.last(), bank.last_associate(), bank.last_associate_batch())
        now[2].pop("scene_roots")
        assert now == records
    # tracks x points at 2^31: refused before anything is read (the rows of such a call would not fit any memory)
    with PoseTrackBank(eng, 1 << 20) as wide:
        r = C.byref(sa_point_rows(40, 2, 0.0, 0, zp, None, None))
        ids = arr(np.arange(1, 2049))
        assert g(wide.h, 0, None, 2048, r, 2048, ids[0], opts(), tp, wp, None, cp) == U and "2^31" in lib.sa_last_error(eng.h).decode()
        assert len(wide) == 0
