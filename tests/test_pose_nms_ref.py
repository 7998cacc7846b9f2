"""The semantics of include/similari_pose_nms.h on the numpy model tests/pose_nms_ref.py: the strict comparisons, the stable rank, the
greedy chain, poses that cannot pair, the symmetry of w, and an independent f64 OKS-NMS on 200 seeded crowds.  No GPU needed."""
import math

import numpy as np
import pytest

import oks_ref as OR
import pose_nms_ref as NR

f32 = np.float32
SIG = OR.sigmas_for(17)


def body(seed, P=17, size=40.0):
    return (np.random.default_rng(seed).uniform(-0.5, 0.5, (P, 2)) * size + 100.0).astype(f32)


def shifted(b, *shifts):
    return np.stack([b + f32(s) for s in shifts]).astype(f32)


def test_the_nms_threshold_is_strict():
    pts = shifted(body(1), 0.0, 1.5)
    _, _, w = NR.nms(pts, [0.9, 0.8], SIG, want_matrix=True)
    w01 = float(w[0, 1])
    assert 0.0 < w01 < 1.0
    assert NR.nms(pts, [0.9, 0.8], SIG, nms_threshold=w01).tolist() == [0, 1]   # w > w is false: the pair does not suppress
    assert NR.nms(pts, [0.9, 0.8], SIG, nms_threshold=float(np.nextafter(f32(w01), f32(0)))).tolist() == [0]
    assert NR.nms(pts, [0.8, 0.9], SIG, nms_threshold=float(np.nextafter(f32(w01), f32(0)))).tolist() == [1]


def test_the_score_threshold_is_strict_and_a_nan_score_is_dropped():
    pts = shifted(body(2), 0.0, 100.0, 200.0, 300.0)
    scores = np.array([0.5, np.nan, 0.7, 0.3], f32)
    assert NR.nms(pts, scores, SIG).tolist() == [2, 0, 3]
    assert NR.nms(pts, scores, SIG, score_threshold=0.5).tolist() == [2]          # 0.5 > 0.5 is false
    assert NR.nms(pts, scores, SIG, score_threshold=float("nan")).tolist() == [2, 0, 3]   # NaN: no threshold
    assert NR.nms(pts, [-np.inf, np.inf, 1.0, -1.0], SIG).tolist() == [1, 2, 3]           # f32::MIN lets -1 pass, not -inf


def test_equal_scores_keep_the_input_order():
    pts = shifted(body(3), *[100.0 * k for k in range(6)])
    assert NR.nms(pts, [0.5] * 6, SIG).tolist() == [0, 1, 2, 3, 4, 5]
    assert NR.nms(pts, [0.5, 0.7, 0.5, 0.7, 0.5, 0.7], SIG).tolist() == [1, 3, 5, 0, 2, 4]
    dup = shifted(body(3), 0.0, 0.0, 0.0)   # exact duplicates, equal scores: the first in input order survives
    assert NR.nms(dup, [0.5] * 3, SIG, nms_threshold=0.99).tolist() == [0]


def chain():
    """A suppresses B, B alone would suppress C, A does not: -> (pts, scores, thr)"""
    pts = shifted(body(4), 0.0, 1.2, 2.4)
    scores = [0.9, 0.8, 0.7]
    _, _, w = NR.nms(pts, scores, SIG, want_matrix=True)
    near, far = min(float(w[0, 1]), float(w[1, 2])), float(w[0, 2])
    assert far < near
    return pts, scores, 0.5 * (near + far)


def test_the_chain_case():
    pts, scores, thr = chain()
    assert NR.nms(pts, scores, SIG, nms_threshold=thr).tolist() == [0, 2]         # C survives: B was dead when its turn came
    assert NR.nms(pts[1:], scores[1:], SIG, nms_threshold=thr).tolist() == [0]    # B alone suppresses C


def test_a_pose_that_cannot_pair_is_kept_and_suppresses_nobody():
    b = body(5)
    pts = shifted(b, 0.0, 0.0, 0.0, 0.0)
    pts[0, :, 0] = np.nan            # the best pose has no point at all
    pts[2, 2:, 0] = np.nan           # two present points: below min_common = 3 with everybody
    keep, order, w = NR.nms(pts, [0.9, 0.8, 0.7, 0.6], SIG, nms_threshold=0.5, min_common=3, want_matrix=True)
    assert keep.tolist() == [0, 1, 2]                                             # 3 is 1's exact duplicate
    assert np.isnan(w[0, 1:]).all() and np.isnan(w[1, 2]) and np.isnan(w[2, 3]) and w[1, 3] == 1.0
    assert NR.nms(pts, [0.9, 0.8, 0.7, 0.6], SIG, nms_threshold=0.5, min_common=1).tolist() == [0, 1]
    one = shifted(b, 0.0, 0.0)
    one[:, 1:, 0] = np.nan           # single-point poses: s2 = 0, refused
    line = shifted(b, 0.0, 0.0)
    line[:, :, 1] = 7.0              # collinear, axis-parallel: s2 = 0
    for deg in (one, line):
        keep, _, w = NR.nms(deg, [0.9, 0.8], SIG, nms_threshold=0.0, want_matrix=True)
        assert keep.tolist() == [0, 1] and np.isnan(w).all()


def test_one_point_keeps_everything():
    pts = np.zeros((5, 1, 2), f32)
    keep, _, w = NR.nms(pts, [0.1, 0.5, 0.3, 0.5, 0.2], [0.05], nms_threshold=0.0, want_matrix=True)
    assert keep.tolist() == [1, 3, 2, 4, 0] and np.isnan(w).all()


def test_w_is_symmetric_bit_for_bit():
    pts, scores, _ = NR.crowd(11, 6, 40, 17, absent=0.2)
    pres = NR.present_of(pts)
    full = OR.weights(pts[..., :2], pres, pres, pts[..., :2], SIG, 2)
    assert np.array_equal(full.view(np.uint32), full.T.copy().view(np.uint32))
    assert np.isfinite(full).sum() > 100


# ---- an independent OKS-NMS in f64 ---------------------------------------------------------------------------------------------------
THR = 0.7
BAD_SEEDS = ()   # seeds of range(N_SEEDS + len(BAD_SEEDS)) where some pair's f64 w lies within 1e-5 of THR (the test asserts the margin of every seed it uses)
N_SEEDS = 200


def seeds():
    return [s for s in range(N_SEEDS + len(BAD_SEEDS)) if s not in BAD_SEEDS]


def scene_of(seed):
    rng = np.random.default_rng(100000 + seed)
    m = int(rng.integers(5, 61))
    return NR.crowd(5000 + seed, max(1, m // int(rng.integers(2, 6))), m, 17, jitter=float(rng.choice([0.01, 0.03, 0.08])), absent=0.15)


def plain_f64(pts, scores, sigmas, thr):
    """OKS-NMS as the header's text says it, in f64 with math.exp -> (keep, the smallest |w - thr| over the pairs)"""
    pts = np.asarray(pts, np.float64)
    order = sorted((i for i in range(len(scores)) if scores[i] > -math.inf), key=lambda i: -float(scores[i]))
    areas, margin = [], math.inf
    for i in order:
        here = [(x, y) for x, y in pts[i, :, :2] if math.isfinite(x) and math.isfinite(y)]
        xs, ys = [q[0] for q in here], [q[1] for q in here]
        areas.append((max(xs) - min(xs)) * (max(ys) - min(ys)) if here else math.nan)
    alive = [True] * len(order)
    for a, i in enumerate(order):
        for b in range(a + 1, len(order)):
            j = order[b]
            s2 = 0.5 * (areas[a] + areas[b])
            if not s2 > 0:
                continue
            terms = []
            for p in range(pts.shape[1]):
                (xi, yi), (xj, yj) = pts[i, p, :2], pts[j, p, :2]
                if all(map(math.isfinite, (xi, yi, xj, yj))):
                    k2 = 2.0 * float(sigmas[p])
                    terms.append(math.exp(-((xj - xi) ** 2 + (yj - yi) ** 2) / (s2 * 2.0 * k2 * k2)))
            if not terms:
                continue
            w = sum(terms) / len(terms)
            margin = min(margin, abs(w - thr))
            if alive[a] and alive[b] and w > thr:
                alive[b] = False
    return [i for a, i in enumerate(order) if alive[a]], margin


def test_the_model_agrees_with_a_plain_f64_oks_nms_on_200_crowds():
    suppressed = 0
    for seed in seeds():
        pts, scores, _ = scene_of(seed)
        keep64, margin = plain_f64(pts, scores, SIG, THR)
        # the input condition: no pair stands within 1e-5 of the threshold in f64 — the polynomial's relative error is 2.4e-7 and the
        # f32 sum of at most 17 terms adds a few 1e-7 more, so the f32 model must then decide every pair as f64 does
        assert margin > 1e-5, (seed, margin)
        assert NR.nms(pts, scores, SIG, nms_threshold=THR).tolist() == keep64, seed
        suppressed += len(scores) - len(keep64)
    assert suppressed > 1000   # the crowds are crowds


def test_the_lazy_greedy_pass_is_the_greedy_pass():
    for seed in (1, 2, 3):
        pts, scores, _ = NR.crowd(40 + seed, 9, 120, 3, jitter=0.05, absent=0.1)
        for thr in (0.3, 0.8):
            full = NR.nms(pts, scores, OR.sigmas_for(3), nms_threshold=thr, score_threshold=0.1, min_common=2)
            assert NR.nms_lazy(pts, scores, OR.sigmas_for(3), nms_threshold=thr, score_threshold=0.1, min_common=2).tolist() == full.tolist()
            assert 5 < len(full) < 110


@pytest.mark.parametrize("P", [2, 17, 65])
def test_the_matrix_has_nan_on_and_below_the_diagonal(P):
    pts, scores, _ = NR.crowd(21 + P, 3, 9, P)
    _, order, w = NR.nms(pts, scores, OR.sigmas_for(P), want_matrix=True)
    assert np.isnan(w[np.tril_indices(9)]).all() and np.isfinite(w[np.triu_indices(9, 1)]).all()
    assert order.tolist() == sorted(range(9), key=lambda i: -float(scores[i]))
