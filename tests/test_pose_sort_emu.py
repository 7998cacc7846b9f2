"""similari_amd/csrc/sa_pose_gate.h — the circle, the limit and the refusal the kernels of sa_pose.hip call — compiled by g++ against the
numpy model tests/pose_sort_ref.py, bit for bit; and the model's dist_in_2r and limit against the oracle's restatement of the box rule
where the two overlap.  No GPU needed."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as O
import pose_sort_ref as SR
from similari_amd import abi

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "similari_amd" / "csrc"
f32, u8, u32 = np.float32, np.uint8, np.uint32
SOURCE = r"""
#include "sa_pose_gate.h"
extern "C" {
// items x P points (x, y) with a flag each -> circle [items][4]: xc, yc, r, valid
void emu_circles(uint32_t items, uint32_t P, const float* xy, const uint8_t* counts, float* out) {
  for (uint32_t t = 0; t < items; ++t) {
    sa_pose_rect q;
    sa_pose_rect_clear(q);
    for (uint32_t p = 0; p < P; ++p)
      if (counts[(size_t)t * P + p]) sa_pose_rect_add(q, xy[((size_t)t * P + p) * 2], xy[((size_t)t * P + p) * 2 + 1]);
    sa_geo c;
    const bool ok = sa_pose_circle(q, c);
    out[t * 4] = c.xc, out[t * 4 + 1] = c.yc, out[t * 4 + 2] = c.r, out[t * 4 + 3] = ok ? 1.f : 0.f;
  }
}
void emu_refused(uint32_t M, uint32_t T, const float* pc, const float* tc, const float* limits, uint8_t* out, float* dist) {
  for (uint32_t i = 0; i < M; ++i)
    for (uint32_t j = 0; j < T; ++j) {
      const sa_geo a{pc[i * 4], pc[i * 4 + 1], pc[i * 4 + 2], 0.f}, b{tc[j * 4], tc[j * 4 + 1], tc[j * 4 + 2], 0.f};
      out[(size_t)i * T + j] = sa_pose_refused(pc[i * 4 + 3] != 0.f, a, tc[j * 4 + 3] != 0.f, b, limits[j]) ? 1 : 0;
      dist[(size_t)i * T + j] = sa_dist_in_2r(a, b);
    }
}
float emu_limit(uint32_t n, const uint32_t* delta, const float* max_dist, uint64_t epoch_delta) { return sa_pose_limit(n, delta, max_dist, epoch_delta); }
}
"""


def bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(((a.view(u32) == b.view(u32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("pose_sort_emu")
    (d / "emu.cpp").write_text(SOURCE)
    subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-I", str(CSRC),
                    str(d / "emu.cpp"), "-o", str(d / "libemu.so")], check=True)
    return C.CDLL(str(d / "libemu.so"))


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def bp(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def circles(emu, xy, counts):
    xy, counts = np.ascontiguousarray(xy, f32), np.ascontiguousarray(counts, u8)
    out = np.zeros((len(counts), 4), f32)
    emu.emu_circles(len(counts), counts.shape[1], fp(xy), bp(counts), fp(out))
    return out


def refusals(emu, pc, tc, limits):
    pc, tc, limits = np.ascontiguousarray(pc, f32), np.ascontiguousarray(tc, f32), np.ascontiguousarray(limits, f32)
    out, dist = np.zeros((len(pc), len(tc)), u8), np.zeros((len(pc), len(tc)), f32)
    emu.emu_refused(len(pc), len(tc), fp(pc), fp(tc), fp(limits), bp(out), fp(dist))
    return out.astype(bool), dist


def check(emu, xy_p, cnt_p, xy_t, cnt_t, limits):
    """circles, distances and refusals of the header == the model's -> (refused, the header's circles of both sides)"""
    got_p, got_t = circles(emu, xy_p, cnt_p), circles(emu, xy_t, cnt_t)
    for got, xy, cnt in ((got_p, xy_p, cnt_p), (got_t, xy_t, cnt_t)):
        c, ok = SR.circle(xy, cnt)
        assert bits(got[:, :3], c) and (got[:, 3] != 0).tolist() == ok.tolist()
    no, dist = refusals(emu, got_p, got_t, limits)
    assert bits(dist, SR.dist_in_2r(got_p[:, None, :3], got_t[None, :, :3]))
    want = SR.refused(got_p[:, :3], got_p[:, 3] != 0, got_t[:, :3], got_t[:, 3] != 0, limits)
    assert (no == want).all()
    return no, got_p, got_t


@pytest.mark.parametrize("P", [1, 2, 17, 65])
def test_random_sets_with_absent_points(emu, P):
    rng = np.random.default_rng(10 + P)
    M, T = 23, 31
    # people of size ~6 whose centres are up to ~40 apart: distances in units of 2r on both sides of every limit
    xy_p = (rng.uniform(-20, 20, (M, 1, 2)) + rng.uniform(-3, 3, (M, P, 2))).astype(f32)
    xy_t = (rng.uniform(-20, 20, (T, 1, 2)) + rng.uniform(-3, 3, (T, P, 2))).astype(f32)
    cnt_p, cnt_t = rng.random((M, P)) >= 0.3, rng.random((T, P)) >= 0.2
    cnt_p[3] = False   # no point at all
    cnt_t[5] = False
    xy_p[~cnt_p] = np.nan   # an absent point may hold anything
    limits = rng.choice(np.array([0.5, 1.0, 2.0, np.inf], f32), T)
    no, got_p, got_t = check(emu, xy_p, cnt_p, xy_t, cnt_t, limits)
    assert got_p[3, 3] == 0 and got_t[5, 3] == 0 and not no[3].any() and not no[:, 5].any()   # a side without a circle is never refused
    assert not no[:, np.isinf(limits)].any() and no.any() and not no[:, np.isfinite(limits)].all()


def test_one_point_on_both_sides_has_radius_zero(emu):
    xy_p = np.array([[[3.0, 4.0]], [[0.0, 0.0]]], f32)
    xy_t = np.array([[[0.0, 0.0]], [[3.0, 4.0]]], f32)
    ones = np.ones((2, 1), bool)
    no, got_p, got_t = check(emu, xy_p, ones, xy_t, ones, np.array([1000.0, 1000.0], f32))
    assert (got_p[:, 2] == 0).all() and (got_t[:, 2] == 0).all()
    # r = 0 on both sides: the distance is 5 / sqrt(1e-5), about 1581; equal circles are at distance 0
    assert no.tolist() == [[True, False], [False, True]]
    _, dist = refusals(emu, got_p, got_t, np.array([1000.0, 1000.0], f32))
    assert dist[0, 1] == 0 and dist[1, 0] == 0 and 1500 < dist[0, 0] < 1600


def test_collinear_points(emu):
    t = np.arange(7, dtype=f32)
    xy = np.stack([np.stack([t, np.zeros(7, f32)], -1), np.stack([np.full(7, 2, f32), t], -1), np.stack([t, t], -1)])   # on a row, a column, a diagonal
    cnt = np.ones((3, 7), bool)
    got = circles(emu, xy, cnt)
    c, ok = SR.circle(xy, cnt)
    assert bits(got[:, :3], c) and ok.all()
    assert got[0].tolist() == [3, 0, 3, 1] and got[1].tolist() == [2, 3, 3, 1] and got[2, :2].tolist() == [3, 3] and got[2, 2] == np.sqrt(f32(18))
    check(emu, xy, cnt, xy[::-1], cnt, np.array([0.5, 0.5, 0.5], f32))


def test_nan_and_absent_points_and_the_order_of_the_walk(emu):
    rng = np.random.default_rng(5)
    xy = rng.uniform(-9, 9, (12, 17, 2)).astype(f32)
    cnt = rng.random((12, 17)) >= 0.4
    xy[~cnt] = np.nan
    a = circles(emu, xy, cnt)
    perm = rng.permutation(17)
    assert bits(a, circles(emu, xy[:, perm], cnt[:, perm]))   # minimum and maximum are exact: the order cannot change a bit
    assert bits(a[:, :3], SR.circle(xy, cnt)[0])


def test_an_infinite_limit_refuses_nothing(emu):
    xy_p = np.array([[[1e6, 1e6], [1e6 + 1, 1e6]]], f32)
    xy_t = np.array([[[0.0, 0.0], [1.0, 1.0]]], f32)
    ones = np.ones((1, 2), bool)
    assert not check(emu, xy_p, ones, xy_t, ones, np.array([np.inf], f32))[0].any()
    assert check(emu, xy_p, ones, xy_t, ones, np.array([1e3], f32))[0].all()


def test_a_distance_exactly_equal_to_the_limit_stays(emu):
    """Exact arithmetic: circles of radius 5 (a 6 x 8 rectangle) whose centres are 7.5 apart on an axis — dist = 7.5 / sqrt(100 + 1e-5).
    The limit is that very f32; one ulp below it the pair is refused."""
    def rect(x, y):
        return [[x - 3, y - 4], [x + 3, y + 4], [x, y]]
    xy_p, xy_t = np.array([rect(10, 20)], f32), np.array([rect(17.5, 20), rect(10, 27.5)], f32)
    ones = np.ones((1, 3), bool)
    d = SR.dist_in_2r(np.array([10, 20, 5], f32), np.array([17.5, 20, 5], f32))
    assert d == f32(7.5) / np.sqrt(f32(100) + SR.EPS)
    below = np.nextafter(d, f32(0))
    no, got_p, got_t = check(emu, xy_p, ones, xy_t, np.ones((2, 3), bool), np.array([d, below], f32))
    assert got_p[0].tolist() == [10, 20, 5, 1] and got_t[:, 2].tolist() == [5, 5]
    assert no.tolist() == [[False, True]]


def test_the_limit_lookup(emu):
    cons = SR.constraints([(3, 2.0), (1, 0.5), (3, 9.0), (7, 8.5)])
    assert cons == [(1, f32(0.5)), (3, f32(2.0)), (7, f32(8.5))]   # sorted; of equal deltas the first stays
    d = np.array([c[0] for c in cons], u32)
    x = np.array([c[1] for c in cons], f32)
    for delta in range(0, 10):
        got = emu.emu_limit
        got.restype = C.c_float
        got.argtypes = [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_uint64]
        assert f32(got(len(d), d.ctypes.data_as(C.POINTER(C.c_uint32)), fp(x), delta)) == SR.limit(cons, delta)
    assert SR.limit(cons, 8) == np.inf and SR.limit([], 1) == np.inf and SR.limit(cons, 2) == f32(2.0)


def test_the_model_against_the_oracles_box_rule():
    """Where the pose rule overlaps the box rule — the points are the corners of an axis-aligned box whose arithmetic is exact — the
    model's circle is the box's (centre, radius), its dist_in_2r the oracle's, and its limit lookup the oracle's validate()."""
    L = O.lib()
    rng = np.random.default_rng(8)
    cons = SR.constraints([(1, 0.5), (2, 1.0), (4, 4.0)])
    d64 = np.array([c[0] for c in cons], np.uint64)
    x32 = np.array([c[1] for c in cons], f32)
    for _ in range(50):
        l1, t1, l2, t2 = (float(v) for v in rng.integers(-40, 40, 4))
        w1, h1, w2, h2 = (float(v) for v in rng.integers(1, 12, 4) * 2)   # even sides: half extents and centres are whole numbers
        b1, b2 = abi.ltwh(l1, t1, w1, h1), abi.ltwh(l2, t2, w2, h2)
        corners = lambda l, t, w, h: np.array([[[l, t], [l + w, t], [l, t + h], [l + w, t + h]]], f32)
        c1, ok1 = SR.circle(corners(l1, t1, w1, h1), np.ones((1, 4), bool))
        c2, ok2 = SR.circle(corners(l2, t2, w2, h2), np.ones((1, 4), bool))
        assert c1[0, 2] == f32(L.or_radius(O.box_ptr(b1))) and c2[0, 2] == f32(L.or_radius(O.box_ptr(b2)))
        dist = SR.dist_in_2r(c1[0], c2[0])
        assert dist == f32(L.or_dist_in_2r(O.box_ptr(b1), O.box_ptr(b2)))
        for delta in range(1, 6):
            ok = bool(L.or_constraints_validate(len(cons), d64.ctypes.data_as(C.POINTER(C.c_uint64)), O.fptr(x32), delta, float(dist)))
            assert ok == (not SR.refused(c1, ok1, c2, ok2, [SR.limit(cons, delta)])[0, 0])
