"""The packed halls of tests/pose_hall.py are what tests/test_gpu_pose_hall.py takes them for — shown from the numpy model
tests/pose_ref.py alone, no GPU and none of the product's code — and the host build of the device's assignment route
(tests/pose_emu.assign: the greedy start, then sa_assign_component_dense<256, 8, false>) gives kuhn_munkres's matches on every one of
them, row for row.  The second is what lets the GPU file compare matches and not only totals.

The floors.  The halls of the single call with at least 256 poses and 256 tracks were made for them: at least 100 search roots, at
least 100 rows matched to another column than the one they bid for (40 where threshold 99.5 leaves the 257-track hall 163 matches),
every strip of a 2048-track hall (the columns [256 c, 256 c + 256) one thread's c-th register holds) with at least 20 matched columns.
The other uses are smaller by their shape (40 tracks; 96 x 96; common points required of poses that have two): there the floor is 40
roots and 40 rows that moved or went unmatched with a usable pair — a cluster of tests/pose_ref.people's crowd has about six rows."""
import numpy as np
import pytest

import pose_hall as H
import pose_ref as PR

USES = H.uses()
BIG_VOTE = {H.hall(*k) for k, _ in H.VOTE if min(k[0], k[1]) >= H.BIG}


@pytest.mark.parametrize("h,min_common,threshold", USES, ids=["%r-%d-%g" % u for u in USES])
def test_the_hall_is_what_it_claims(h, min_common, threshold):
    f = h.facts(min_common, threshold)
    print(h, min_common, threshold, f)
    if h in BIG_VOTE and min_common == 1:
        assert f["roots"] >= 100
        assert f["moved"] >= (40 if h.T == 257 and threshold == 99.5 else 100)
    else:
        assert f["roots"] >= 40 and f["moved"] + f["dropped"] >= 40
    if h.T == 257:   # more poses than tracks, in a corner
        assert f["dropped"] >= 40 and f["winners_dropped"] >= 1   # a row the greedy start had matched ends unmatched: only a search that ends at another row's self column does that
        assert f["top"] == 256 and f["strips"][1] == 1            # the one column of strip 1
    if h.T == 2048:
        assert f["top"] >= 1792 and min(f["strips"][1:]) >= 20
    assert f["coupled_weights"] > 0   # a finite weight from a track whose x and y are correlated
    if threshold == 99.5:
        assert 0.1 < f["usable"] < 0.5
    assert f["matched"] >= 30


@pytest.mark.parametrize("h,min_common,threshold", USES, ids=["%r-%d-%g" % u for u in USES])
def test_the_host_build_of_the_route_gives_the_models_matches(h, min_common, threshold):
    rm, gain, roots = h.emu(min_common, threshold)
    total, ref, wq, thr_q = h.vote(min_common, threshold)
    assert gain + h.m * thr_q == total and PR.total_of(rm, wq, thr_q) == total
    assert roots == PR.greedy_roots(wq, thr_q) == h.facts(min_common, threshold)["roots"]
    assert (rm == ref).all()


def test_a_higher_threshold_matches_fewer_where_rows_compete():
    for k, thrs in H.VOTE:
        h = H.hall(*k)
        n = [h.facts(1, t)["matched"] for t in thrs]
        assert all(a >= b for a, b in zip(n, n[1:])), h
    h = H.hall(*H.VOTE[1][0])
    assert h.facts(1, 99.5)["matched"] < h.facts(1, 1.0)["matched"]


@pytest.mark.parametrize("k", H.TRACK, ids=[repr(H.hall(*k)) for k in H.TRACK])
def test_the_frame_loops_halls_have_one_optimum(k):
    h = H.hall(*k)
    total, ref, wq, thr_q = h.vote(H.MIN_COMMON, H.THRESHOLD)
    assert PR.forced_rows(wq, total, ref).all()


def test_forced_rows_of_a_few_rows():
    h = H.hall(*H.BATCH[2])
    total, ref, wq, thr_q = h.vote(H.MIN_COMMON, H.THRESHOLD)
    every = PR.forced_rows(wq, total, ref)
    rows = np.array([0, 7, 150, 299])
    some = PR.forced_rows(wq, total, ref, rows=rows)
    assert (some[rows] == every[rows]).all() and not np.delete(some, rows).any()
    assert not PR.forced_rows(wq, total, ref, rows=[]).any()
