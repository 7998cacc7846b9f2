"""similari_amd/csrc/sa_pose_oks.h — the source the OKS kernels of sa_pose.hip call — compiled by g++ (tests/emu_oks) against the numpy
model tests/oks_ref.py, bit for bit: exp on a dense sweep and at its boundaries, the area, the per-point constant and the cell function
with every edge the header names.  And the model's exp against f64 under the reference's EPS = 1e-5 (src/lib.rs:80).  No GPU needed."""
import numpy as np
import pytest

import oks_emu as OE
import oks_ref as OR
import pose_ref as PR

f32, u32 = np.float32, np.uint32
EPS = 1e-5
BELOW_32 = np.nextafter(f32(32), f32(0))


def bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(((a.view(u32) == b.view(u32)) | (np.isnan(a) & np.isnan(b))).all())


def sweep():
    """262 144 f32 arguments over [0, 32): evenly spaced, evenly spaced in the exponent down to 1e-30, and random ones"""
    rng = np.random.default_rng(1)
    lin = np.linspace(0, 32, 131072, endpoint=False)
    log = np.exp(np.linspace(np.log(1e-30), np.log(32), 65536, endpoint=False))
    rnd = rng.uniform(0, 32, 65536)
    e = np.concatenate([lin, log, rnd]).astype(f32)
    return e[e < f32(32)]


# ---- 1. exp ------------------------------------------------------------------------------------------
def test_exp_equals_the_model_on_the_sweep_and_is_accurate():
    e = sweep()
    assert len(e) >= 200000 and e.min() == 0 and e.max() > 31.99
    got, want = OE.exp(e), OR.oks_exp(e)
    assert bits(got, want)
    assert ((got >= 0) & (got <= 1)).all()
    assert (got[e > 0] > 0).all()   # nothing below 32 underflows
    exact = np.exp(-e.astype(np.float64))
    rel = np.abs(want.astype(np.float64) - exact) / exact
    print(f"sa_oks_exp: largest relative error over {len(e)} f32 arguments in [0, 32): {rel.max():.3e} at e = {e[np.argmax(rel)]!r}")
    assert rel.max() <= EPS


def test_exp_at_its_boundaries():
    e = np.array([0.0, -0.0, BELOW_32, 32.0, np.nextafter(f32(32), f32(64)), 1e30, np.inf, np.nan], f32)
    got = OE.exp(e)
    assert bits(got, OR.oks_exp(e))
    assert got[0].view(u32) == f32(1).view(u32) and got[1] == 1   # exp(0) is exactly 1
    assert 0 < got[2] < 2e-14 and np.isfinite(got[2]) and got[2] >= np.finfo(f32).tiny   # the last live argument gives a normal number
    assert (got[3:].view(u32) == 0).all()   # +0 for everything that is not below 32, NaN included
    tiny = np.array([1e-45, 1e-38, 1e-10, 5.96e-8, 1.2e-7], f32)
    assert bits(OE.exp(tiny), OR.oks_exp(tiny)) and (OE.exp(tiny) <= 1).all() and OE.exp(tiny)[0] == 1


def test_var2_and_area_equal_the_model():
    rng = np.random.default_rng(2)
    s = np.concatenate([OR.sigmas_for(17), rng.uniform(1e-3, 10, 100).astype(f32)])
    assert bits(OE.var2(s), OR.var2(s))
    assert OE.var2([0.5])[0] == 2.0   # 2 (2 * 0.5)^2
    xy = rng.uniform(-50, 50, (200, 9, 2)).astype(f32)
    counts = rng.random((200, 9)) < 0.4
    counts[0] = False                 # no point: no area
    counts[1] = [1] + [0] * 8         # one point: area 0
    xy[2, :, 0] = 3.0                 # collinear, axis-parallel: area 0
    counts[2] = True
    got = OE.area(xy, counts)
    assert bits(got, OR.area(xy, counts))
    assert np.isnan(got[0]) and got[1] == 0 and got[2] == 0 and (got[3:][counts[3:].sum(1) > 1] > 0).all()


# ---- 2. the cell function ----------------------------------------------------------------------------
def random_scene(seed, M, T, P, crowd):
    rng = np.random.default_rng(seed)
    centres = PR.people(rng, T, P, crowd)
    bank = PR.model_bank(PR.track_rounds(rng, centres))
    poses, pres = PR.poses_of(rng, centres, M)
    poses[pres & (rng.random(pres.shape) < 0.05)] = np.nan   # present by the mask, absent by the value
    pres &= np.isfinite(poses).all(-1)
    return poses, pres, bank


@pytest.mark.parametrize("min_common", [1, 3])
@pytest.mark.parametrize("M,T,P", [(1, 1, 1), (7, 9, 2), (7, 9, 5), (23, 31, 17), (31, 12, 17)])
@pytest.mark.parametrize("crowd", [False, True])
def test_the_cell_function_equals_the_model(crowd, M, T, P, min_common):
    poses, pres, bank = random_scene(300 + M + P, M, T, P, crowd)
    sig = OR.sigmas_for(P)
    want = OR.weights(poses, pres, bank.has, bank.mean, sig, min_common)
    got = OE.matrix(poses, pres, bank.has, bank.mean, sig, min_common)
    assert bits(got, want)
    real = got[~np.isnan(got)]
    assert ((real >= 0) & (real <= 1)).all()
    if P == 1:
        assert np.isnan(got).all()   # one point per side: no body size, every pair refused
    if P == 17:
        assert (real > 0.5).any() and (real == 0).any()   # somebody continues a track; pairs wholly beyond the cut

def cell(z, pres, mu, has, sig, min_common=1):
    """one pose against one track, by the header and by the model -> w (asserted equal)"""
    z, mu = np.asarray(z, f32)[None], np.asarray(mu, f32)[None]
    mean = np.zeros(mu.shape[:2] + (4,), f32)
    mean[..., :2] = mu
    pres, has = np.asarray(pres, bool)[None], np.asarray(has, bool)[None]
    got = OE.matrix(z, pres, has, mean, sig, min_common)
    assert bits(got, OR.weights(z, pres, has, mean, sig, min_common))
    return got[0, 0]


def test_the_edges_of_the_cell_function():
    sig = np.array([0.1, 0.2, 0.3], f32)
    tri = [[0, 0], [4, 0], [0, 3]]
    yes = [1, 1, 1]
    assert cell(tri, yes, tri, yes, sig) == 1.0                                   # the same pose: every c_p is exp(0)
    assert np.isnan(cell(tri, [1, 0, 0], tri, [0, 1, 0], sig))                    # no common point
    assert np.isnan(cell(tri, [1, 0, 0], tri, [1, 0, 0], sig))                    # one point per side: s2 = 0, refused
    line = [[0, 1], [4, 1], [9, 1]]
    assert np.isnan(cell(line, yes, line, yes, sig))                              # collinear on both sides: refused
    w = cell(line, yes, tri, yes, sig)                                            # collinear on one side only: kept
    assert w == w and 0 <= w <= 1
    assert cell(tri, [1, 1, 0], tri, yes, sig) == 1.0 and np.isnan(cell(tri, [1, 1, 0], tri, yes, sig, min_common=3))   # an absent point
    for p in range(3):                                                            # a NaN point in any position is absent
        z = np.array(tri, f32)
        z[p, 1] = np.nan
        pres = np.isfinite(z).all(-1)
        assert cell(z, pres, tri, yes, sig) == 1.0
    far = [[0, 0], [4, 0], [2e19, 3]]                                       # d2 overflows to inf with finite areas: e = inf, c = 0
    w = cell(far, yes, tri, yes, sig)
    assert w == f32(2) / f32(3)
    # both areas overflow to inf and d2 is inf: e = inf / inf = NaN, the point is dropped; the others have e = 0
    big_a = [[-3e19, -3e19], [3e19, 3e19], [0, 0]]
    big_b = [[-3e19, -3e19], [3e19, 3e19], [3e19, -3e19]]
    assert np.isinf(OE.area(np.array([big_a], f32), np.ones((1, 3), bool))[0])
    assert cell(big_a, yes, big_b, yes, sig) == 1.0 and cell(big_a, yes, big_b, yes, sig, min_common=2) == 1.0
    assert np.isnan(cell(big_a, yes, big_b, yes, sig, min_common=3))              # two common points, not three
