"""similari_amd/csrc/sa_pose.h and the split distance of sa_kalman_point.h — the source the kernels of sa_pose.hip call — compiled by g++
(tests/emu_pose) against the numpy model tests/pose_ref.py, and the whole-scene assignment route (greedy start from the rows' bid
words, roots ascending, sa_assign_component_dense<256, 8, false> through its host path) against the oracle's kuhn_munkres on
SortVoting's dense matrix.  No GPU needed.  "Bits" is the comparison of tests/test_points_emu.py."""
import numpy as np
import pytest

import points_emu as E
import points_ref as R
import pose_emu as PE
import pose_ref as PR
from test_points_emu import WEIGHTS, bits, spd

f32 = np.float32


# ---- 1. factor + factored distance = sa_pkf_distance ----------------------------------------------
def check_split(m, c, z, pw):
    fac, ok = PE.factor(m, c, pw)
    d = PE.distance_factored(fac, ok, z)
    assert bits(d, E.distance(m, c, z, pw, 0))
    assert bits(d, R.distance(m, c, z, pw))
    assert (np.isnan(d) == ~ok).all()   # on finite states NaN means a failed pivot and nothing else
    return int((~ok).sum())


@pytest.mark.parametrize("pw,vw", WEIGHTS)
def test_the_split_distance_on_tracks_from_initiate(pw, vw):
    rng = np.random.default_rng(21)
    n = 300
    z = rng.uniform(-100, 100, (n, 2)).astype(f32)
    vel = rng.uniform(-3, 3, (n, 2)).astype(f32)
    m, c = R.initiate(z, pw, vw)
    assert check_split(m, c, z, pw) == 0
    for k in range(30):
        m, c = R.predict(m, c, pw, vw)
        z = (z + vel + rng.normal(0, 0.5, (n, 2))).astype(f32)
        assert check_split(m, c, z, pw) == 0, k
        m, c = R.update(m, c, z, pw)


@pytest.mark.parametrize("pw,vw", WEIGHTS)
def test_the_split_distance_on_general_covariances_and_failed_pivots(pw, vw):
    rng = np.random.default_rng(22)
    n = 400
    m = rng.uniform(-5, 5, (n, 4)).astype(f32)
    c = spd(rng, n)
    c[0] = -c[0]          # a negative first pivot
    c[1, 1, 1] = -5       # a negative second one
    zc = np.zeros((2, 4, 4), f32)   # pivots that are exactly 0: the first, the second
    zc[0, 0, 0] = -pw * pw
    zc[0, 1, 1] = 1
    zc[1, 0, 0] = 1
    zc[1, 1, 1] = -pw * pw
    assert check_split(m[:2], zc, m[:2, :2] + f32(1), pw) == 2
    failed = 0
    for k in range(4):
        z = (m[:, :2] + rng.normal(0, 1, (n, 2))).astype(f32)
        failed += check_split(m, c, z, pw)
        m, c = R.update(m, c, z, pw)
        m, c = R.predict(m, c, pw, vw)
    assert 2 <= failed < 4 * n


# ---- 2. the cell function = the model --------------------------------------------------------------
def scene(seed, M, T, P, crowd, pw=R.PW, vw=R.VW):
    rng = np.random.default_rng(seed)
    centres = PR.people(rng, T, P, crowd)
    bank = PR.model_bank(PR.track_rounds(rng, centres), pw, vw)
    bank.cov[0, :3] = -np.abs(bank.cov[0, :3]) - f32(1)   # track 0: its first points are indefinite, their pivots fail
    if T > 2:
        bank.cov[1] = -np.abs(bank.cov[1]) - f32(1)       # track 1: all of them
    poses, pres = PR.poses_of(rng, centres, M)
    poses[pres & (rng.random(pres.shape) < 0.05)] = np.nan   # present by the mask, absent by the value
    pres &= np.isfinite(poses).all(-1)
    return poses, pres, bank


@pytest.mark.parametrize("pw,vw", WEIGHTS)
@pytest.mark.parametrize("min_common", [1, 3])
@pytest.mark.parametrize("M,T,P", [(1, 1, 1), (7, 9, 5), (23, 31, 17), (31, 12, 17)])
@pytest.mark.parametrize("crowd", [False, True])
def test_the_cell_function_equals_the_model(crowd, M, T, P, min_common, pw, vw):
    poses, pres, bank = scene(100 + M + P, M, T, P, crowd, pw, vw)
    want = PR.weights(poses, pres, bank.has, bank.mean, bank.cov, pw, min_common)
    got = PE.matrix(poses, pres, bank.has, bank.mean, bank.cov, pw, min_common)
    assert bits(got, want)
    if P == 17:
        real = got[~np.isnan(got)]
        assert (real > 50).any() and (real == 0).any()          # pairs inside the gate, pairs wholly beyond it
        assert np.isnan(got).any() or min_common == 1
    if T > 2:
        assert np.isnan(got[:, 1]).all()   # nothing is common with a track whose pivots all fail


def test_min_common_and_nan_cells():
    """k < min_common: no pair; a pose without a present point: no pair with anybody; a failed pivot only drops its point."""
    rng = np.random.default_rng(5)
    P, T = 4, 3
    centres = PR.people(rng, T, P, False)
    bank = PR.model_bank(PR.track_rounds(rng, centres, absent=0.0, never=0.0))
    bank.cov[1, 2] = -np.abs(bank.cov[1, 2]) - f32(1)
    poses = np.repeat(centres[1][None], 3, 0).astype(f32)
    pres = np.array([[1, 1, 1, 1], [1, 0, 1, 0], [0, 0, 0, 0]], bool)
    for mc, want_k in ((1, [3, 1, 0]), (2, [3, 0, 0]), (4, [0, 0, 0])):
        w = PE.matrix(poses, pres, bank.has, bank.mean, bank.cov, R.PW, mc)
        assert bits(w, PR.weights(poses, pres, bank.has, bank.mean, bank.cov, R.PW, mc))
        assert (~np.isnan(w[:, 1])).tolist() == [k >= mc and k > 0 for k in want_k], mc
    assert PE.lib().emu_pose_threshold_q(1.0) == 1000000 and PE.lib().emu_pose_gain(f32(1.0), 1000000) == 0
    assert PE.lib().emu_pose_gain(f32(np.nan), 0) == 0 and PE.lib().emu_pose_gain(f32(100.0), 1000000) == 99000000


# ---- 3. the whole-scene route = kuhn_munkres on SortVoting's matrix --------------------------------
def check_route(w, threshold):
    M = w.shape[0]
    rm, gain, roots = PE.assign(w, threshold)
    total, ref, wq, thr_q = PR.vote(w, threshold)
    assert gain + M * thr_q == total
    assert PR.total_of(rm, wq, thr_q) == total
    cols = rm[rm >= 0]
    assert len(set(cols.tolist())) == len(cols)
    assert roots == PR.greedy_roots(wq, thr_q)
    differ = np.flatnonzero(rm != ref)
    if len(differ):   # only where the optimum is not unique
        assert not PR.forced_rows(wq, total, ref)[differ].any()
    return roots, len(differ)


def test_the_route_on_thirty_random_scenes():
    rng = np.random.default_rng(31)
    searched = scenes_with_roots = differing = 0
    for trial in range(30):
        M, T = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        crowd = trial % 2 == 1
        poses, pres, bank = scene(1000 + trial, M, T, 5, crowd)
        w = PE.matrix(poses, pres, bank.has, bank.mean, bank.cov, R.PW, 1)
        roots, diff = check_route(w, 1.0)
        searched += roots
        scenes_with_roots += roots > 0
        differing += diff
        if not crowd:
            assert roots == 0   # people apart: the greedy start is the answer
    assert scenes_with_roots >= 8 and searched >= scenes_with_roots   # over half of the 15 crowded scenes went through the dense search
    assert differing == 0   # random f32 weights: a tie between two optima has probability ~0


@pytest.mark.parametrize("density", [0.05, 0.5, 1.0])
def test_the_route_on_random_matrices_and_thresholds(density):
    """Weights over the whole range of the cost (0 .. 100), sparse and full, with thresholds that cut through them."""
    rng = np.random.default_rng(int(density * 100))
    for trial in range(10):
        M, T = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        w = rng.uniform(0, 100, (M, T)).astype(f32)
        w[rng.random((M, T)) > density] = np.nan
        check_route(w, [0.0, 1.0, 50.0][trial % 3])


def test_the_route_breaks_ties_to_a_valid_optimum():
    w = np.full((6, 4), 90.0, f32)
    w[0, 1] = np.nan
    roots, _ = check_route(w, 1.0)
    assert roots >= 1
    check_route(np.full((3, 3), np.nan, f32), 1.0)
    check_route(np.zeros((3, 3), f32), 0.0)   # a weight equal to the diagonal is no edge
