"""tests/points_ref.py, the dense model of the reference's 2D point filter, pinned to the oracle's box filter (oracle/oracle.cpp:
or_kf_initiate / _predict / _update / _distance, themselves pinned by the reference's known-answer tests) value for value, with no
tolerance.  The embedding: a point (x, y) is the box (x, y, aspect 1, height 1, no angle, confidence 1), whose standard deviations are
the point filter's (k * weight * height), and the point state is rows and columns {0, 1, 5, 6} of the box state.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import points_ref as R
from similari_amd import abi

OL = O.lib()
IDX = [0, 1, 5, 6]
f32 = np.float32


def box(x, y):
    return abi.make_boxes([x], [y], [1.0], [1.0], confidence=[1.0])


def embed(mean4, cov4):
    """4-state -> 10-state: the other diagonal entries 0.01, mean[3] = mean[4] = 1 (aspect, height)."""
    m = np.zeros(10, f32)
    m[3] = m[4] = 1
    m[IDX] = mean4
    c = np.diag(np.full(10, 0.01, f32)).astype(f32)
    c[np.ix_(IDX, IDX)] = cov4
    return m, c


def cut(m10, c10):
    return m10[IDX].copy(), c10.reshape(10, 10)[np.ix_(IDX, IDX)].copy()


def same(a, b):
    """Value for value: equal numbers (NaN equal to NaN)."""
    return np.array_equal(np.asarray(a, f32), np.asarray(b, f32), equal_nan=True)


def or_initiate(pw, vw, x, y):
    m, c = np.zeros(10, f32), np.zeros(100, f32)
    OL.or_kf_initiate(pw, vw, O.box_ptr(box(x, y)), O.fptr(m), O.fptr(c))
    return m, c


def or_predict(pw, vw, m, c):
    om, oc = np.zeros(10, f32), np.zeros(100, f32)
    OL.or_kf_predict(pw, vw, O.fptr(m), O.fptr(np.ascontiguousarray(c.reshape(-1))), O.fptr(om), O.fptr(oc))
    return om, oc


def or_update(pw, vw, m, c, x, y):
    om, oc = np.zeros(10, f32), np.zeros(100, f32)
    OL.or_kf_update(pw, vw, O.fptr(m), O.fptr(np.ascontiguousarray(c.reshape(-1))), O.box_ptr(box(x, y)), O.fptr(om), O.fptr(oc))
    return om, oc


def or_distance(pw, vw, m, c, x, y):
    return f32(OL.or_kf_distance(pw, vw, O.fptr(m), O.fptr(np.ascontiguousarray(c.reshape(-1))), O.box_ptr(box(x, y))))


def run_track(pw, vw, pts):
    """initiate, then per point: predict, distance, update — on both sides; every mean, covariance and distance compared."""
    pw, vw = f32(pw), f32(vw)
    om, oc = or_initiate(pw, vw, *pts[0])
    m, c = R.initiate(pts[0], pw, vw)
    assert same(m, cut(om, oc)[0]) and same(c, cut(om, oc)[1])
    for z in pts[1:]:
        om, oc = or_predict(pw, vw, om, oc)
        m, c = R.predict(m, c, pw, vw)
        assert same(m, cut(om, oc)[0]) and same(c, cut(om, oc)[1])
        d_o, d = or_distance(pw, vw, om, oc, *z), R.distance(m, c, z, pw)
        assert same(d, d_o), (d, d_o)
        assert same(R.cost(d, True), f32(OL.or_kf_cost(d_o, 1)))
        om, oc = or_update(pw, vw, om, oc, *z)
        m, c = R.update(m, c, z, pw)
        assert same(m, cut(om, oc)[0]) and same(c, cut(om, oc)[1])
    return m, c


def test_tracks_from_initiate_equal_the_oracle():
    rng = np.random.default_rng(11)
    for t in range(40):
        pw, vw = (R.PW, R.VW) if t % 4 == 0 else (rng.uniform(0.01, 0.2), rng.uniform(0.001, 0.05))
        start = rng.uniform(-50, 50, 2)
        vel = rng.uniform(-2, 2, 2)
        pts = np.array([start + k * vel + rng.normal(0, 0.3, 2) for k in range(31)], f32)
        run_track(pw, vw, pts)


def random_spd(rng):
    a = rng.normal(0, 1, (4, 4))
    return (a @ a.T * rng.uniform(0.01, 2.0) + np.eye(4) * 1e-3).astype(f32)


def test_general_covariances_equal_the_oracle():
    """Off-diagonal mass everywhere: three predict / distance / update rounds from 100 random SPD matrices.  A step whose update left
    the covariance indefinite answers NaN on both sides."""
    rng = np.random.default_rng(12)
    nans = 0
    for t in range(100):
        pw, vw = f32(rng.uniform(0.01, 0.2)), f32(rng.uniform(0.001, 0.05))
        m = rng.uniform(-5, 5, 4).astype(f32)
        c = random_spd(rng)
        om, oc = embed(m, c)
        for k in range(3):
            z = (m[:2] + rng.normal(0, 1, 2)).astype(f32)
            d_o, d = or_distance(pw, vw, om, oc, *z), R.distance(m, c, z, pw)
            assert same(d, d_o), (t, k, d, d_o)
            nans += int(np.isnan(d))
            om, oc = or_update(pw, vw, om, oc, *z)
            m, c = R.update(m, c, z, pw)
            assert same(m, cut(om, oc)[0]) and same(c, cut(om, oc)[1]), (t, k)
            om, oc = or_predict(pw, vw, om, oc)
            m, c = R.predict(m, c, pw, vw)
            assert same(m, cut(om, oc)[0]) and same(c, cut(om, oc)[1]), (t, k)
    print("steps with a NaN distance:", nans)


# the points of kalman_2d_point.rs:165-220 (the last one is the distance's) and of python/kalman_2d_vec.py, typed in as data
RS_POINTS = [(1.0, 0.0), (1.1, 0.1), (1.2, 0.2), (1.3, 0.3), (1.4, 0.4), (1.5, 0.5), (1.6, 0.6), (1.7, 0.7), (1.8, 0.67), (1.9, 0.60), (2.0, 0.57)]
PY_VEC = [[(1.0 + i * 0.1, 2.0 + i * 0.1) for i in range(21)], [(3.0 + i * 0.05, 4.0 + i * 0.05) for i in range(21)]]


def test_the_reference_sequences():
    m, c = run_track(R.PW, R.VW, np.array(RS_POINTS, f32))
    assert np.isfinite(m).all() and abs(float(m[0]) - 2.0) < 0.2   # it follows the points
    for pts in PY_VEC:
        run_track(R.PW, R.VW, np.array(pts, f32))
    # the vector filter is the point filter per point: the model, vectorised over both points, gives each point's own bits
    z = np.array(PY_VEC, f32)   # [2 points][21 steps][2]
    bank = R.Bank((2,))
    bank.initiate(z[:, 0], np.ones(2, bool))
    for k in range(1, 21):
        bank.predict()
        bank.update(z[:, k], np.ones(2, bool))
    for p in range(2):
        m, c = R.initiate(z[p, 0])
        for k in range(1, 21):
            m, c = R.update(*R.predict(m, c), z[p, k])
        assert m.tobytes() == bank.mean[p].tobytes() and c.tobytes() == bank.cov[p].tobytes()


def test_costs():
    d = np.array([0.0, 1.5, 5.9914, 5.9915, 5.9916, 11.069, 11.070, 11.071, 99.0, 1e9, np.inf, np.nan], f32)
    inv = R.cost(d, True)
    for i, v in enumerate(d):
        assert same(inv[i], f32(OL.or_kf_cost(v, 1))), v
    plain = R.cost(d, False)
    lit = f32(5.9915)
    below, above = np.nextafter(lit, f32(0)), np.nextafter(lit, f32(10))
    assert R.cost(below, False) == below and R.cost(lit, False) == lit and R.cost(above, False) == f32(100)
    assert np.isnan(plain[-1]) and np.isnan(inv[-1])
    assert plain[-2] == f32(100) and inv[-2] == f32(0)
    assert same(plain[:4], d[:4]) and (plain[4:11] == f32(100)).all()


def test_presence_and_step():
    rng = np.random.default_rng(13)
    z = rng.normal(0, 1, (5, 3)).astype(f32)
    z[0, 0] = np.nan
    z[1, 1] = np.inf
    z[2, 2] = 0.2
    z[3, 2] = np.nan
    z[4, 2] = 0.9
    assert R.present_of(z, 0.5).tolist() == [False, False, False, False, True]
    assert R.present_of(z[:, :2]).tolist() == [False, False, True, True, True]
    assert R.present_of(z[:, :2], mask=[1, 1, 0, 1, 1]).tolist() == [False, False, False, True, True]
    # step = initiate (first sighted) + predict + update
    a, b = R.Bank((6,)), R.Bank((6,))
    for k in range(5):
        pts = rng.normal(0, 1, (6, 2)).astype(f32)
        pres = rng.random(6) > 0.4
        xy = a.step(pts, pres)
        b.initiate(pts, pres & ~b.has)
        b.predict()
        xy2 = b.update(pts, pres)
        assert same(xy, xy2) and same(a.mean, b.mean) and same(a.cov, b.cov) and (a.has == b.has).all()
        assert np.isnan(xy[~a.has]).all() and np.isfinite(xy[a.has]).all()
