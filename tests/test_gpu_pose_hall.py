"""The keypoint vote in packed halls on the MI355X: scenes that make the device's dense search work — hundreds of roots in ONE component,
augmenting paths through columns of every register strip of a 2048-track scene, matched rows given up for a better total —, thresholds
that cut through the live weights (99.0, 99.5: sa_pose_gain has to tell 99.6 from 99.7), covariances whose x and y are correlated (the
l10 lane of the factor) and a bank with other filter weights than the defaults.  tests/test_pose_hall_ref.py shows on the CPU that the
halls are such scenes and that the host build of the route gives kuhn_munkres's matches on them row for row; here the device has to
give the same rows.

The model is tests/pose_ref.py (weights) with the oracle's kuhn_munkres (matches) and tests/points_ref.py (states); "bits" is the
comparison of tests/test_gpu_points.py.  A hall's tracks are written with set_state, one bank per hall and module."""
import copy
import time

import numpy as np
import pytest

import points_ref as R
import pose_hall as H
import pose_ref as PR
from similari_amd import abi
from similari_amd.engine import Engine
from similari_amd.pose import PoseBank
from similari_amd.pose_track import PoseTrackBank
from test_gpu_points import Model, bits, check_states
from test_gpu_pose import check_vote, scene
from test_gpu_pose_batch import NoTracks, call_of, fill, ids_of, local
from test_gpu_pose_track import same_states

pytestmark = pytest.mark.gpu
f32, u64 = np.float32, np.uint64


@pytest.fixture(scope="module")
def eng():
    e = Engine(abi.make_config(positional="iou", positional_threshold=0.3, device=0))
    yield e
    e.close()


def build(bank, scs):
    """fill(), then every hall's states as its model has them"""
    t0 = time.perf_counter()
    fill(bank, scs)
    for sc, t in zip(scs, ids_of(scs)):
        if isinstance(sc, H.Hall):
            sc.settle(bank, t)
    print("bank of %s: %.2f s" % (scs, time.perf_counter() - t0))
    return bank


@pytest.fixture(scope="module")
def banks(eng):
    """key -> the PoseBank of that hall, built when first asked for; associate changes no state, so the tests share it"""
    made = {}

    def get(key):
        if key not in made:
            made[key] = build(PoseBank(eng, key[2]), [H.hall(*key)])
        return made[key]

    yield get
    for b in made.values():
        b.close()


def check_hall_vote(h, ids, w, st, min_common, threshold):
    """check_vote, and: the rows of the serial solver (tests/pose_emu.assign on the model's weights), which are the model's"""
    roots = check_vote(h, ids, w, st, min_common, threshold)
    col_of = {int(t): j for j, t in enumerate(h.ids)}
    got = np.array([col_of[int(t)] if t else -1 for t in ids], np.int64)
    ref = h.vote(min_common, threshold)[1]
    differ = int((got != ref).sum())
    print(h, min_common, threshold, "roots", roots, "matched", int((got >= 0).sum()), "rows that differ from the model", differ)
    assert (got == h.emu(min_common, threshold)[0]).all()
    assert differ <= h.m // 100
    return got


# ---- a. the matrix -------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", H.MATRIX, ids=[repr(H.hall(*k)) for k in H.MATRIX])
def test_the_tap_matrix_carries_the_models_bits(banks, key):
    h = H.hall(*key)
    want = h.weights()
    coupled = h.model.has & (h.model.cov[..., 1, 0] != 0)   # l10 = p10 / l00 and p10 = cov10: these states have l10 != 0
    seen = (h.pres[:, None, :] & coupled[None]).any(-1) & ~np.isnan(want)
    assert seen.sum() > want.size // 2   # the model: most compared cells went through the l10 term
    ids, w, tap = banks(key).associate(h.poses, present=h.pres, matrix=True)
    assert bits(tap, want)
    assert (want[~np.isnan(want)] > 90).any()


# ---- b. the vote ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,threshold", [(k, t) for k, thrs in H.VOTE for t in thrs],
                         ids=["%r-%g" % (H.hall(*k), t) for k, thrs in H.VOTE for t in thrs])
def test_the_vote_gives_the_serial_solvers_rows(banks, key, threshold):
    h = H.hall(*key)
    h.vote(1, threshold), h.emu(1, threshold)   # (the model first: the time printed below is the device's call)
    bank = banks(key)
    t0 = time.perf_counter()
    ids, w = bank.associate(h.poses, present=h.pres, threshold=threshold)
    print("associate: %.1f ms" % (1e3 * (time.perf_counter() - t0)))
    st = bank.last_associate()
    got = check_hall_vote(h, local(ids, 0), w, st, 1, threshold)
    assert (st["poses"], st["tracks"]) == (h.m, h.T)
    if threshold != 1.0 and h.facts(1, threshold)["matched"] < h.facts(1, 1.0)["matched"]:   # the model: the threshold costs matches
        low, _ = bank.associate(h.poses, present=h.pres)
        assert (got >= 0).sum() < (low != 0).sum() == h.facts(1, 1.0)["matched"]


# ---- c. the batch --------------------------------------------------------------------------------------
def test_a_batch_of_halls_beside_small_scenes(eng):
    P = 2
    halls = [H.hall(*k) for k in H.BATCH]
    scs = [halls[0], scene(3, 5, P), halls[1], NoTracks(4, P), halls[2]]
    for sc in scs:
        if sc.T:
            sc.vote(H.MIN_COMMON, H.THRESHOLD)
    with build(PoseBank(eng, P), scs) as bank:
        t0 = time.perf_counter()
        got = bank.associate_batch(call_of(scs), threshold=H.THRESHOLD, min_common=H.MIN_COMMON)
        print("associate_batch: %.1f ms" % (1e3 * (time.perf_counter() - t0)))
        st = bank.last_associate_batch()
    roots = st["scene_roots"]
    for s, sc in enumerate(scs):
        ids, w = got[s]
        if sc.T == 0:
            assert (ids == 0).all() and np.isnan(w).all() and roots[s] == 0
            continue
        one = {"matched": int((ids != 0).sum()), "launches": st["launches"], "roots": int(roots[s])}
        check = check_hall_vote if isinstance(sc, H.Hall) else check_vote
        check(sc, local(ids, s), w, one, H.MIN_COMMON, H.THRESHOLD)
        assert roots[s] == PR.greedy_roots(*sc.vote(H.MIN_COMMON, H.THRESHOLD)[2:])
    assert st["roots"] == int(roots.sum()) and st["launches"] == 3 and st["scenes"] == len(scs)
    assert st["matched"] == sum(int((g[0] != 0).sum()) for g in got)


# ---- d. the frame loop against the models --------------------------------------------------------------
def test_the_frame_loop_in_three_halls_against_the_models(eng):
    P = 3
    scs = [H.hall(*k) for k in H.TRACK]
    assert all(sc.m <= 300 and sc.P == P for sc in scs)
    refs = []
    for sc in scs:   # on the CPU, before any GPU call: every row of every optimum is forced, so 100 % of the ids are compared
        total, ref, wq, thr_q = sc.vote(H.MIN_COMMON, H.THRESHOLD)
        assert PR.forced_rows(wq, total, ref).all()
        refs.append(ref)
    assert sum(int((r < 0).sum()) for r in refs) >= 20 and sum(int((r >= 0).sum()) for r in refs) >= 100
    tids = ids_of(scs)
    mdl = Model(P, cap=2048)
    for sc, t in zip(scs, tids):
        mdl.call("step", t, *sc.rounds[0], create=True)
        rows = [mdl.row[int(i)] for i in t]
        mdl.b.has[rows], mdl.b.mean[rows], mdl.b.cov[rows] = sc.model.has, sc.model.mean, sc.model.cov
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
    kw = dict(threshold=H.THRESHOLD, min_common=H.MIN_COMMON)
    with build(PoseTrackBank(eng, P), scs) as bank, build(PoseBank(eng, P), scs) as twin:
        t0 = time.perf_counter()
        got = bank.track_batch(call_of(scs), new, coast=True, **kw)
        print("track_batch: %.1f ms" % (1e3 * (time.perf_counter() - t0)))
        st = bank.last_track()
        for s in range(len(scs)):
            assert (got[s] == want[s]).all(), s
        check_states(bank, mdl)
        assert st["created"] == used and st["matched"] == len(every) - used
        assert (st["scene_roots"] == [sc.facts(H.MIN_COMMON, H.THRESHOLD)["roots"] for sc in scs]).all()
        twin_got = twin.track_batch(call_of(scs), new, **kw)
        assert all((a == b).all() for a, b in zip(got, twin_got))
        same_states(bank, twin)


# ---- e. other filter weights ---------------------------------------------------------------------------
PW, VW = 25.0, 2.0


def weighted_frames(P=17, T=60, M=50, threshold=95.0, seed=5, noise=20.0):
    """On the CPU, from the models alone: T people over a 100-unit box (the gate of a filter with position weight 25 is about as wide:
    a crowd), tracks grown by two rounds of step, then three frames — the model's weights, kuhn_munkres's matches, the ids track() has
    to give, the model stepped by them -> (ids, the two rounds, one dict per frame; "model": the model after that frame)."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(T)))
    centres = PR.people(rng, T, P, False, spacing=100.0 / side)
    rounds = PR.track_rounds(rng, centres, rounds=2, noise=3.0)
    ids = np.arange(1, T + 1, dtype=u64) * 7
    mdl = Model(P, pw=PW, vw=VW, cap=512)
    for z, pres in rounds:
        mdl.call("step", ids, z, pres, create=True)
    frames, next_id = [], 1000
    for k in range(3):
        poses, pres = PR.poses_of(rng, centres, M, noise=noise)
        order = np.array(mdl.ids, u64)
        rows = [mdl.row[int(i)] for i in order]
        w = PR.weights(poses, pres, mdl.b.has[rows], mdl.b.mean[rows], mdl.b.cov[rows], PW)
        assert k or not bits(w, PR.weights(poses, pres, mdl.b.has[rows], mdl.b.mean[rows], mdl.b.cov[rows], R.PW))   # the weight is in the number
        total, ref, wq, thr_q = PR.vote(w, threshold)
        forced = PR.forced_rows(wq, total, ref)
        got = np.where(ref >= 0, order[np.maximum(ref, 0)], 0).astype(u64)
        fresh = np.flatnonzero(got == 0)
        got[fresh] = np.arange(next_id, next_id + len(fresh), dtype=u64)
        idle = np.setdiff1d(order, got)
        mdl.call("step", got, poses, pres, create=True)
        mdl.call("predict", idle)
        frames.append(dict(poses=poses, pres=pres, w=w, ids=got, next_id=next_id, created=len(fresh), forced=forced, model=copy.deepcopy(mdl),
                           roots=PR.greedy_roots(wq, thr_q), usable=float((wq[:, M:] > thr_q).mean())))
        next_id += len(fresh)
    return ids, rounds, frames


def test_a_bank_with_other_filter_weights(eng):
    P, threshold = 17, 95.0
    ids, rounds, frames = weighted_frames(P, threshold=threshold)
    for k, f in enumerate(frames):   # on the CPU: a crowd, cut by the threshold, and one optimum
        print("frame", k, "roots", f["roots"], "usable", f["usable"], "created", f["created"])
        assert f["forced"].all(), k
        assert f["roots"] >= 5 and 0.1 < f["usable"] < 0.9 and f["created"] <= len(f["ids"]) - 10, k
    assert sum(f["created"] for f in frames) >= 5
    with PoseTrackBank(eng, P, position_weight=PW, velocity_weight=VW) as bank:
        for z, pres in rounds:
            bank.step(ids, z, present=pres)
        f = frames[0]
        _, _, tap = bank.associate(f["poses"], present=f["pres"], threshold=threshold, matrix=True)
        assert bits(tap, f["w"])
        for k, f in enumerate(frames):
            got = bank.track(f["poses"], f["next_id"], present=f["pres"], threshold=threshold)
            assert (got == f["ids"]).all(), k
            assert bank.last_track()["created"] == f["created"] and bank.last_track()["roots"] == f["roots"], k
            check_states(bank, f["model"])
