"""The host model of an i8 store (tests/i8_ref.py): the coding rule of include/similari_i8.h in numpy f32, and the cell formula on the
exact integers."""
import numpy as np
import pytest

import i8_ref as I

u32 = np.uint32


def rows(seed, n, D, scale=1.0):
    return (np.random.default_rng(seed).normal(0, scale, (n, D))).astype(np.float32)


@pytest.mark.parametrize("D", [1, 2, 33, 64, 65, 512])
def test_codes_stay_in_range_and_a_nonzero_row_holds_a_127(D):
    x = np.concatenate([rows(D, 40, D), rows(D + 1, 20, D, 1e-20), rows(D + 2, 20, D, 1e20)])
    q = I.codes(x)
    assert q.dtype == np.float32 and q.shape == x.shape
    assert np.array_equal(q, np.rint(q)) and np.abs(q).max() <= 127
    assert np.all(np.abs(q).max(axis=1) == 127)                  # the absmax element itself: m * (127 / m) rounds to 127
    assert np.array_equal(np.sign(q[np.arange(len(x)), np.abs(x).argmax(axis=1)]), np.sign(x[np.arange(len(x)), np.abs(x).argmax(axis=1)]))


@pytest.mark.parametrize("D", [1, 33, 100])
def test_coding_is_idempotent(D):
    x = rows(7 + D, 50, D)
    x[3] = 0
    q = I.codes(x)
    assert np.array_equal(I.codes(q).view(u32), q.view(u32))     # m = 127, inv = 1: no bit changes
    assert np.array_equal(I.codes(q * np.float32(0.25)).view(u32), q.view(u32))   # nor under a power-of-two factor


def test_zero_rows():
    D = 9
    x = rows(1, 6, D)
    x[0] = 0
    x[0, 2] = -0.0
    x[1, 4] = np.nan
    x[2, 0] = np.inf
    x[3, 8] = -np.inf
    x[4] = 0
    x[4, 1] = np.float32(2.0**-101)                               # below the floor
    q = I.codes(x)
    assert not q[:5].view(u32).any()                             # +0.0 everywhere
    assert np.abs(q[5]).max() == 127
    edge = np.zeros((2, D), np.float32)
    edge[0, 3] = np.float32(2.0**-100)                            # the floor itself is a row
    edge[1, 3] = np.nextafter(np.float32(2.0**-100), np.float32(0))
    q = I.codes(edge)
    assert q[0, 3] == 127 and not q[1].any()
    assert I.codes(np.zeros((0, D), np.float32)).shape == (0, D)


def test_one_huge_element_leaves_the_rest_at_zero():
    x = rows(2, 1, 16)
    x[0, 5] = np.float32(-3e38)
    q = I.codes(x)
    assert q[0, 5] == -127 and np.count_nonzero(q) == 1


def test_ties_round_to_even():
    # m = 127: inv = 1 exactly, so the products are the values themselves
    x = np.array([[127, 2.5, 3.5, -2.5, -0.5, 0.5, 1.5, 126.5, -126.5, 2.4999998, 2.5000002]], np.float32)
    assert I.codes(x).tolist() == [[127, 2, 4, -2, -0.0, 0, 2, 126, -126, 2, 3]]
    # m = 254: inv = 0.5 exactly
    x = np.array([[254, 5, 7, -5, 1, 253]], np.float32)
    assert I.codes(x).tolist() == [[127, 2, 4, -2, 0, 126]]


def test_the_cell_of_equal_codes_is_one_and_the_matrix_is_symmetric():
    for D in (1, 33, 128, 2048):
        q = I.codes(rows(30 + D, 24, D))
        c = I.cells_f32(q, q)
        assert c.dtype == np.float32
        assert np.array_equal(np.diag(c).view(u32), np.full(len(q), np.float32(1)).view(u32))   # sqrtf(x * x) == x
        assert np.array_equal(c.view(u32), c.T.copy().view(u32))
        assert I.cells_f32(q[:1], -q[:1])[0, 0] == np.float32(-1)
        err = np.abs(c.astype(np.float64) - I.cells_f64(q, q)).max()
        assert err <= 5e-7                                           # 4.5 roundings of 2^-24 on |cell| <= 1


def test_a_zero_row_gives_nan_cells():
    q = I.codes(rows(3, 4, 20))
    q[1] = 0
    c = I.cells_f32(q, q)
    assert np.isnan(c[1]).all() and np.isnan(c[:, 1]).all() and np.isfinite(np.delete(np.delete(c, 1, 0), 1, 1)).all()


def test_the_widest_row_fits_the_accumulator():
    D = 131072
    assert 127 * 127 * D < 2**31
    q = np.full((1, D), 127, np.float32)
    assert I.cells_f32(q, q)[0, 0] == np.float32(1) and I.cells_f32(q, -q)[0, 0] == np.float32(-1)


def test_the_tap_marks_absent_observations():
    K, D = 3, 10
    s = [rows(4, 2, D), np.zeros((0, D), np.float32), rows(5, 3, D)]
    qf = [rows(6, 1, D)]
    t = I.tap(qf, s, K)
    assert t.shape == (1, K, 3, K) and t.dtype == np.float32
    assert np.isfinite(t[0, 0, 0, :2]).all() and np.isnan(t[0, 0, 0, 2]) and np.isnan(t[0, :, 1]).all() and np.isnan(t[0, 1:]).all()
    assert np.abs(t[0, 0, 2].astype(np.float64) - I.tap(qf, s, K, I.cells_f64)[0, 0, 2]).max() <= 5e-7


def test_the_model_of_a_store_codes_on_the_way_in():
    K, D = 3, 12
    m = I.Model(K, D)
    f = [rows(8, 2, D), rows(9, 1, D)]
    m.upsert([5, 6], f)
    m.append([5], [rows(10, 1, D)])
    assert np.array_equal(m.feats(5)[:2], I.codes(f[0])) and np.array_equal(m.feats(5)[2:], I.codes(rows(10, 1, D)))
    assert np.array_equal(m.feats(6), I.codes(f[1]))
