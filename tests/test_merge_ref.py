"""Hand-worked cases of the two retention rules and of the store model the device tests compare against (tests/merge_ref.py).
Rows are one float wide and named by their value, so a bank reads as a list of names."""
import numpy as np
import pytest

import merge_ref as R


def names(model, i):
    return [float(r[0]) for r, _ in model.banks[i]]


def bank(*obs):
    return [(np.array([n], np.float32), np.float32(q)) for n, q in obs]


def test_latest_keeps_the_last_c_in_their_order():
    b = bank((1, 9), (2, 0), (3, 5), (4, 1), (5, 7))
    assert [float(r[0]) for r, _ in R.optimize(b, R.LATEST, 3)] == [3, 4, 5]
    assert [float(r[0]) for r, _ in R.optimize(b, R.LATEST, 8)] == [1, 2, 3, 4, 5]
    assert [float(r[0]) for r, _ in R.optimize(b, R.LATEST, 1)] == [5]


def test_best_sorts_by_quality_and_ties_keep_earlier_first():
    b = bank((1, 0.5), (2, 0.9), (3, 0.5), (4, 0.9), (5, 0.1), (6, 0.5))
    assert [float(r[0]) for r, _ in R.optimize(b, R.BEST, 6)] == [2, 4, 1, 3, 6, 5]
    assert [float(r[0]) for r, _ in R.optimize(b, R.BEST, 4)] == [2, 4, 1, 3]   # of the three 0.5s the latest one goes
    # -0.0 == 0.0: neither ranks before the other; infinities rank like any number
    z = bank((1, -0.0), (2, 0.0), (3, -np.inf), (4, -0.0), (5, np.inf))
    assert [float(r[0]) for r, _ in R.optimize(z, R.BEST, 5)] == [5, 1, 2, 4, 3]
    with pytest.raises(AssertionError):
        R.optimize(bank((1, 0.0), (2, np.nan)), R.BEST, 2)


def test_a_merge_with_an_empty_source_still_sorts():
    m = R.Model(4, 1)
    m.append([7], [[[1], [2], [3], [4]]], quality=[[1, 2, 3, 4]], keep=R.LATEST)
    m.upsert([8], [np.zeros((0, 1), np.float32)])
    assert names(m, 7) == [1, 2, 3, 4]
    m.merge({7: [8]}, keep=R.BEST)
    assert names(m, 7) == [4, 3, 2, 1] and m.order == [7]
    m.merge({7: []}, keep=R.LATEST, capacity=2)   # no source at all: the rule runs all the same
    assert names(m, 7) == [2, 1]


def test_an_append_of_zero_rows_changes_nothing():
    m = R.Model(4, 1)
    m.append([7], [[[1], [2], [3]]], quality=[[1, 2, 3]])
    m.append([7, 9], [None, None], keep=R.BEST, capacity=1)
    assert names(m, 7) == [1, 2, 3]                 # neither sorted nor cut to 1
    assert m.order == [7, 9] and names(m, 9) == []  # the unknown id is created, empty
    m.append([7], [[[4]]], quality=[[0.5]], keep=R.BEST, capacity=3)
    assert names(m, 7) == [3, 2, 1]


def test_one_at_a_time_equals_once_per_call():
    rng = np.random.default_rng(5)
    for _ in range(300):
        K = int(rng.integers(1, 7))
        C = int(rng.integers(1, K + 1))
        keep = (R.LATEST, R.BEST)[int(rng.integers(2))]
        old = bank(*[(n, rng.integers(0, 4)) for n in range(int(rng.integers(0, K + 1)))])
        new = bank(*[(100 + n, rng.integers(0, 4)) for n in range(int(rng.integers(1, K + 1)))])
        step = old
        for ob in new:
            step = R.optimize(step + [ob], keep, C)
        once = R.optimize(old + new, keep, C)
        assert [float(r[0]) for r, _ in step] == [float(r[0]) for r, _ in once]


def test_merge_order_is_removal_order():
    m = R.Model(2, 1)
    m.upsert(range(1, 8), [[[i]] for i in range(1, 8)])
    m.merge({7: [1], 2: [6, 3]})
    # remove 1: 7 -> slot 0; remove 6: last (6) goes; remove 3: 5 -> slot 2
    assert m.order == [7, 2, 5, 4]
    assert names(m, 7) == [7, 1]
    assert names(m, 2) == [6, 3]                  # K = 2, latest: 2 ++ 6 ++ 3 keeps the last two


def test_capacity_grows_with_the_merge_count_as_in_track_merging():
    assert [R.growth_capacity(k) for k in range(5)] == [4, 6, 9, 12, 12]
    m = R.Model(12, 1)
    for t in range(4):
        m.append([t + 1], [[[10 * t + k] for k in range(4)]], quality=[[k + t / 10 for k in range(4)]], keep=R.BEST,
                 capacity=R.growth_capacity(0))
    for merges, src in enumerate((2, 3, 4), start=1):
        m.merge({1: [src]}, keep=R.BEST, capacity={1: R.growth_capacity(merges)})
        assert len(m.banks[1]) == min(4 * (merges + 1), R.growth_capacity(merges))
    assert m.order == [1]
    q = m.quality(1)
    assert len(q) == 12 and np.all(q[:-1] >= q[1:])
    # 16 observations of qualities k + t / 10: the four of k = 0 went
    assert sorted(names(m, 1)) == sorted(10 * t + k for t in range(4) for k in range(1, 4))
