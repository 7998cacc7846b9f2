"""similari_amd/csrc/sa_kalman_point.h — the source the point bank's kernel calls — compiled by g++ (tests/emu_points) must equal the
dense model tests/points_ref.py bit for bit: it skips the constant 0 / 1 entries of the motion and update matrices, and that must
change no bit.  No GPU needed.

"Bit for bit" is taken on the value bits; two NaNs count as the same whatever their sign and payload (numpy's and the compiler's
operations propagate different ones), which test_bits_means_bits checks of the comparison itself."""
import numpy as np
import pytest

import points_emu as E
import points_ref as R

f32 = np.float32
WEIGHTS = [(R.PW, R.VW), (f32(0.11), f32(0.013))]


def bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def test_bits_means_bits():
    assert bits([1.0, np.nan], [1.0, -np.nan])
    assert not bits([0.0], [-0.0]) and not bits([1.0], [np.nextafter(f32(1), f32(2))]) and not bits([np.nan], [1.0])


def spd(rng, n):
    a = rng.normal(0, 1, (n, 4, 4))
    return (a @ np.swapaxes(a, 1, 2) * rng.uniform(0.01, 2.0, (n, 1, 1)) + np.eye(4) * 1e-3).astype(f32)


@pytest.mark.parametrize("pw,vw", WEIGHTS)
def test_tracks_from_initiate(pw, vw):
    rng = np.random.default_rng(21)
    n = 300
    z = rng.uniform(-100, 100, (n, 2)).astype(f32)
    vel = rng.uniform(-3, 3, (n, 2)).astype(f32)
    m, c = R.initiate(z, pw, vw)
    em, ec = E.initiate(z, pw, vw)
    assert bits(m, em) and bits(c, ec)
    for k in range(30):
        m, c = R.predict(m, c, pw, vw)
        em, ec = E.predict(em, ec, pw, vw)
        assert bits(m, em) and bits(c, ec), k
        z = (z + vel + rng.normal(0, 0.5, (n, 2))).astype(f32)
        for mode in (0, 1, 2):
            d = R.distance(m, c, z, pw)
            assert bits(R.cost(d, mode == 2) if mode else d, E.distance(em, ec, z, pw, mode)), (k, mode)
        m, c = R.update(m, c, z, pw)
        em, ec = E.update(em, ec, z, pw)
        assert bits(m, em) and bits(c, ec), k


@pytest.mark.parametrize("pw,vw", WEIGHTS)
def test_general_covariances_and_failed_pivots(pw, vw):
    """Random states with off-diagonal mass everywhere; the reference's update leaves many of them indefinite, so the rounds behind
    it meet failed pivots: NaN from both, and the update's bits still equal."""
    rng = np.random.default_rng(22)
    n = 400
    m = rng.uniform(-5, 5, (n, 4)).astype(f32)
    c = spd(rng, n)
    # rows that fail at once: a negative first pivot, a negative second one
    c[0] = -c[0]
    c[1, 1, 1] = -5
    # ... and pivots that are exactly 0, the first and the second (the distance only: the update divides by them)
    zc = np.zeros((2, 4, 4), f32)
    zc[0, 0, 0] = -pw * pw
    zc[0, 1, 1] = 1
    zc[1, 0, 0] = 1
    zc[1, 1, 1] = -pw * pw
    for mode in (0, 1, 2):
        got = E.distance(m[:2], zc, m[:2, :2] + f32(1), pw, mode)
        assert np.isnan(got).all() and np.isnan(R.distance(m[:2], zc, m[:2, :2] + f32(1), pw)).all()
    em, ec = m.copy(), c.copy()
    failed = 0
    for k in range(4):
        z = (m[:, :2] + rng.normal(0, 1, (n, 2))).astype(f32)
        z = np.where(np.isfinite(z), z, f32(0)).astype(f32)
        d = R.distance(m, c, z, pw)
        failed += int(np.isnan(d).sum())
        for mode in (0, 1, 2):
            assert bits(R.cost(d, mode == 2) if mode else d, E.distance(em, ec, z, pw, mode)), (k, mode)
        m, c = R.update(m, c, z, pw)
        em, ec = E.update(em, ec, z, pw)
        assert bits(m, em) and bits(c, ec), k
        m, c = R.predict(m, c, pw, vw)
        em, ec = E.predict(em, ec, pw, vw)
        assert bits(m, em) and bits(c, ec), k
    assert np.isfinite(m).all() and np.isfinite(c).all()
    assert 2 <= failed < 4 * n   # both kinds of step were met


def test_costs():
    d = np.array([0.0, 5.9914, 5.9915, np.nextafter(f32(5.9915), f32(9)), 11.069, 11.070, np.nextafter(f32(11.070), f32(12)), 1e9, np.inf, np.nan], f32)
    m, c = R.initiate(np.zeros((len(d), 2), f32))
    # a unit projected covariance: d^2 = x^2 exactly for a point (x, 0)
    c[:] = 0
    c[:, 0, 0] = c[:, 1, 1] = f32(1) - R.PW * R.PW
    z = np.zeros((len(d), 2), f32)
    z[:, 0] = np.sqrt(d)
    dd = R.distance(m, c, z)
    for mode in (0, 1, 2):
        assert bits(R.cost(dd, mode == 2) if mode else dd, E.distance(m, c, z, R.PW, mode))


def test_presence():
    rng = np.random.default_rng(23)
    pts = rng.normal(0, 1, (200, 3)).astype(f32)
    pts[::7, 0] = np.nan
    pts[1::11, 1] = np.inf
    pts[2::13, 1] = -np.inf
    pts[3::5, 2] = np.nan
    mask = rng.random(200) > 0.2
    assert (E.present(pts, 0.1) == R.present_of(pts, 0.1)).all()
    assert (E.present(pts, 0.1, mask) == R.present_of(pts, 0.1, mask)).all()
    assert (E.present(pts[:, :2]) == R.present_of(pts[:, :2])).all()
    assert (E.present(pts[:, :2], mask=mask) == R.present_of(pts[:, :2], mask=mask)).all()


@pytest.mark.parametrize("pw,vw", WEIGHTS)
def test_step_with_absent_and_first_sighted_points(pw, vw):
    rng = np.random.default_rng(24)
    n = 500
    bank = R.Bank((n,), pw, vw)
    has = np.zeros(n, np.uint8)
    mean, cov = np.zeros((n, 4), f32), np.zeros((n, 16), f32)
    pos = rng.uniform(-50, 50, (n, 2))
    late = rng.random(n) < 0.3   # never present in the first three rounds
    for k in range(8):
        pos += rng.normal(0, 1, (n, 2))
        z = pos.astype(f32)
        pres = (rng.random(n) > 0.3) & ~(late & (k < 3))
        xy = bank.step(z, pres)
        exy = E.step(has, mean, cov, z, pres, pw, vw)
        assert (has.astype(bool) == bank.has).all(), k
        assert bits(xy, exy), k
        h = bank.has
        assert bits(bank.mean[h], mean[h]) and bits(bank.cov[h], cov.reshape(n, 4, 4)[h]), k
        if k == 2:
            assert (~h).any() and np.isnan(exy[~h]).all()
    assert bank.has.all()
