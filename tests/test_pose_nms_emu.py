"""similari_amd/csrc/sa_pose_nms.h compiled by g++ (tests/pose_nms_emu.py) against the numpy model tests/pose_nms_ref.py: order, pair
matrix and keeps bit for bit, absent points and P = 65 (past one 64-point chunk of the kernel's walk) included.  No GPU needed."""
import numpy as np
import pytest

import oks_ref as OR
import pose_nms_emu as EMU
import pose_nms_ref as NR

f32 = np.float32


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


@pytest.mark.parametrize("P", [1, 2, 17, 65])
@pytest.mark.parametrize("min_common", [1, 3])
def test_matrix_and_keeps_are_the_models_bits(P, min_common):
    pts, scores, _ = NR.crowd(300 + P, 7, 45, P, jitter=0.03, absent=0.25, comps=3)
    mask = np.random.default_rng(P).random((45, P)) > 0.1
    sig = OR.sigmas_for(P)
    for thr in (0.3, 0.7):
        kw = dict(nms_threshold=thr, score_threshold=0.2, min_common=min_common, present=mask, min_score=0.15, want_matrix=True)
        keep, order, w = NR.nms(pts, scores, sig, **kw)
        ekeep, eorder, ew = EMU.nms(pts, scores, sig, **kw)
        assert eorder.tolist() == order.tolist() and ekeep.tolist() == keep.tolist()
        assert same_bits(ew, w)
    if P > 2:   # (P = 1 has no pair at all, P = 2 none with three common points)
        assert np.isfinite(w).any() and 0 < len(keep) < len(order) < 45


def test_degenerate_poses_and_duplicates():
    b = (np.random.default_rng(5).uniform(-20, 20, (17, 2)) + 100).astype(f32)
    pts = np.stack([b, b, b, b, b + f32(0.5)]).astype(f32)
    pts[1, 1:, 0] = np.nan     # a single point
    pts[2, :, 1] = 3.0         # collinear
    scores = np.array([0.9, 0.8, 0.7, 0.6, 0.5], f32)
    sig = OR.sigmas_for(17)
    keep, order, w = NR.nms(pts, scores, sig, nms_threshold=0.5, want_matrix=True)
    ekeep, eorder, ew = EMU.nms(pts, scores, sig, nms_threshold=0.5, want_matrix=True)
    assert same_bits(ew, w) and ekeep.tolist() == keep.tolist() == [0, 2]
    assert ew[0, 3] == 1.0 and 0.5 < ew[0, 4] < 1   # an exact duplicate: 1, bit for bit
    assert ew[0, 1] == 1.0         # ONE side without a body size still has a scale: the common point coincides
    assert np.isnan(ew[1, 2])      # a single point against a line: s2 = 0, refused
    assert ew[0, 2] < 0.5          # the line is far from the body in y
    assert EMU.nms(pts, scores, sig, nms_threshold=0.5).tolist() == [0, 2]   # (without the matrix: the pairs on demand)


def test_empty_and_all_filtered():
    sig = OR.sigmas_for(17)
    assert EMU.nms(np.zeros((0, 17, 2), f32), [], sig).tolist() == []
    assert EMU.nms(np.zeros((3, 17, 2), f32), [np.nan, 0.1, 0.1], sig, score_threshold=0.1).tolist() == []
