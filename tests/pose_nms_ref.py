"""Pose NMS by OKS, include/similari_pose_nms.h, as a numpy f32 model.  TEST INFRASTRUCTURE: what similari_amd/csrc/sa_pose_nms.h (through
tests/pose_nms_emu.py) and the kernels of sa_pose_nms.hip are compared with.

Filter and stable rank from the scores, the presence rule of similari_points.h, the pair matrix through the OKS functions of
tests/oks_ref.py — the earlier pose where the track stands —, the greedy pass of src/utils/nms.rs:58-70."""
import numpy as np

import oks_ref as OR

f32 = np.float32
F32_MIN = f32(-3.4028234663852886e38)


def present_of(pts, present=None, min_score=None):
    """pts [m, P, 2 or 3] -> [m, P] bool: finite x and y, score >= min_score when there is one (a NaN score is absent), the mask"""
    pts = np.asarray(pts, f32)
    ok = np.isfinite(pts[..., 0]) & np.isfinite(pts[..., 1])
    if pts.shape[-1] == 3:
        with np.errstate(invalid="ignore"):
            ok &= pts[..., 2] >= f32(0.0 if min_score is None else min_score)
    if present is not None:
        ok &= np.asarray(present).reshape(ok.shape) != 0
    return ok


def rank(scores, score_threshold=None):
    """-> the indices of the poses with score > score_threshold (None: f32::MIN), by score descending, stable"""
    scores = np.asarray(scores, f32).reshape(-1)
    thr = F32_MIN if score_threshold is None or np.isnan(score_threshold) else f32(score_threshold)
    with np.errstate(invalid="ignore"):
        idx = np.flatnonzero(scores > thr)
    return idx[np.argsort(-scores[idx].astype(np.float64), kind="stable")].astype(np.uint32)


def matrix(pts, pres, sigmas, min_common=1):
    """pts [n, P, >= 2] in rank order, pres [n, P] -> w [n, n] f32: w(i, j) for i < j, NaN elsewhere and where the pair does not
    exist or is refused.  oks_ref.weights(poses = the later, tracks = the earlier)[j, i]."""
    pts, pres = np.asarray(pts, f32)[..., :2], np.asarray(pres, bool)
    n = len(pts)
    if n == 0:
        return np.zeros((0, 0), f32)
    w = OR.weights(pts, pres, pres, pts, sigmas, min_common).T.copy()
    w[np.tril_indices(n)] = np.nan
    return w


def greedy(w, nms_threshold):
    """w [n, n] (upper triangle) -> keep [n] bool"""
    n = len(w)
    keep = np.ones(n, bool)
    with np.errstate(invalid="ignore"):
        over = w > f32(nms_threshold)
    for i in range(n):
        if keep[i]:
            keep[i + 1:] &= ~over[i, i + 1:]
    return keep


def nms(pts, scores, sigmas, nms_threshold=0.9, score_threshold=None, min_common=1, present=None, min_score=None, want_matrix=False):
    """-> kept indices into pts in rank order (np.uint32); want_matrix: (keep, order, w)"""
    pts = np.asarray(pts, f32)
    order = rank(scores, score_threshold)
    pres = present_of(pts, present, min_score)
    w = matrix(pts[order], pres[order], sigmas, min_common)
    keep = order[greedy(w, nms_threshold)]
    return (keep, order, w) if want_matrix else keep


def nms_lazy(pts, scores, sigmas, nms_threshold=0.9, score_threshold=None, min_common=1, present=None, min_score=None):
    """nms() for scenes too large for the whole matrix: the greedy pass asks only for the rows of the poses that are alive when their
    turn comes, each against the later poses still alive — the same cells by the same function, so the same keeps."""
    pts = np.asarray(pts, f32)
    order = rank(scores, score_threshold)
    z, pres = pts[order][..., :2], present_of(pts, present, min_score)[order]
    alive = np.ones(len(order), bool)
    for i in range(len(order)):
        if not alive[i]:
            continue
        later = i + 1 + np.flatnonzero(alive[i + 1:])
        if len(later) == 0:
            break
        w = OR.weights(z[later], pres[later], pres[i:i + 1], z[i:i + 1], sigmas, min_common)[:, 0]
        with np.errstate(invalid="ignore"):
            alive[later[w > f32(nms_threshold)]] = False
    return order[alive]


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def crowd(seed, people, m, P, jitter=0.02, size=40.0, spread=400.0, absent=0.0, comps=2):
    """m poses of P points: clusters of jittered duplicates around `people` distinct people (each a skeleton of about `size` units,
    anywhere in `spread`), jitter relative to the size -> (pts [m, P, comps] f32, scores [m] f32, who [m]).  absent: the share of
    points set to NaN; comps 3: a point score in [0, 1]."""
    rng = np.random.default_rng(seed)
    body = rng.uniform(-0.5, 0.5, (people, P, 2)) * size + rng.uniform(0, spread, (people, 1, 2))
    who = np.concatenate([np.arange(min(people, m)), rng.integers(0, people, max(0, m - people))])
    rng.shuffle(who)
    xy = body[who] + rng.normal(0, jitter * size, (m, P, 2))
    pts = xy if comps == 2 else np.concatenate([xy, rng.uniform(0, 1, (m, P, 1))], axis=2)
    pts = pts.astype(f32)
    if absent:
        pts[rng.random((m, P)) < absent, 0] = np.nan
    scores = rng.uniform(0.05, 1.0, m).astype(f32)
    return pts, scores, who
