"""Object keypoint similarity, the OKS metric of include/similari_pose_oks.h, as a numpy f32 model.  TEST INFRASTRUCTURE: what
similari_amd/csrc/sa_pose_oks.h, the OKS kernels of sa_pose.hip and the banks under an OksMetric are compared with.

Every operation is an f32 one and none is fused: oks_exp restates sa_oks_exp step by step (Cody-Waite reduction, degree-6 Horner form,
a power of two from exponent bits), the area walks the rectangle as sa_pose_rect_add does (pose_sort_ref.circle's walk), the cell sums
in ascending p seeded by the first term.  The presence rules are pose_ref's; the vote is pose_ref.vote — the oracle's kuhn_munkres on
SortVoting's dense matrix."""
import numpy as np

import pose_ref as PR
import pose_sort_ref as SR

f32 = np.float32
LOG2E, LN2_HI, LN2_LO = f32(1.44269504), f32(0.693359375), f32(-2.12194440e-4)
COEF = [f32(1) / f32(720), f32(1) / f32(120), f32(1) / f32(24), f32(1) / f32(6), f32(0.5), f32(1), f32(1)]
THRESHOLD = 0.3   # the reference's DEFAULT_SORT_IOU_THRESHOLD


def oks_exp(e):
    """sa_oks_exp: exp(-e) for e >= 0; exactly 0 where !(e < 32), NaN included"""
    e = np.asarray(e, f32)
    with np.errstate(all="ignore"):
        live = e < f32(32)
        x = np.where(live, -e, f32(0)).astype(f32)
        n = np.rint((x * LOG2E).astype(f32)).astype(f32)
        r = (x - (n * LN2_HI).astype(f32)).astype(f32)
        r = (r - (n * LN2_LO).astype(f32)).astype(f32)
        p = np.full(e.shape, COEF[0], f32)
        for c in COEF[1:]:
            p = ((p * r).astype(f32) + c).astype(f32)
        scale = ((n.astype(np.int32) + np.int32(127)).astype(np.uint32) << np.uint32(23)).view(f32)
        return np.where(live, (p * scale).astype(f32), f32(0)).astype(f32)


def var2(sigmas):
    """sa_oks_var2: 2 (2 sigma)^2"""
    k = (f32(2) * np.asarray(sigmas, f32)).astype(f32)
    return (f32(2) * (k * k).astype(f32)).astype(f32)


def area(xy, counts):
    """xy [..., P, 2], counts [..., P] bool -> [...] f32: (xmax - xmin) * (ymax - ymin) over the points that count, NaN: none counts"""
    xy, counts = np.asarray(xy, f32), np.asarray(counts, bool)
    lead = counts.shape[:-1]
    lo, hi = np.zeros(lead + (2,), f32), np.zeros(lead + (2,), f32)
    n = np.zeros(lead, np.int64)
    with np.errstate(all="ignore"):
        for p in range(counts.shape[-1]):
            z, c = xy[..., p, :], counts[..., p]
            first = (c & (n == 0))[..., None]
            later = (c & (n > 0))[..., None]
            lo = np.where(first, z, np.where(later & (z < lo), z, lo)).astype(f32)
            hi = np.where(first, z, np.where(later & (z > hi), z, hi)).astype(f32)
            n += c
        side = (hi - lo).astype(f32)
        a = (side[..., 0] * side[..., 1]).astype(f32)
    return np.where(n > 0, a, f32(np.nan)).astype(f32)


def scale(a_pose, a_track):
    with np.errstate(all="ignore"):
        return (f32(0.5) * (np.asarray(a_pose, f32)[:, None] + np.asarray(a_track, f32)[None, :]).astype(f32)).astype(f32)


def weights(poses, present, has, mean, sigmas, min_common=1):
    """poses [M, P, 2], present [M, P] bool; has [T, P] bool, mean [T, P, >= 2]; sigmas [P] -> w [M, T] f32, NaN = no pair"""
    poses, present, has = np.asarray(poses, f32), np.asarray(present, bool), np.asarray(has, bool)
    M, P = present.shape
    T = has.shape[0]
    z = np.where(present[..., None], poses, f32(0)).astype(f32)   # an absent point may hold anything, NaN included
    mu = np.where(has[..., None], np.asarray(mean, f32)[..., :2], f32(0)).astype(f32)
    v2 = var2(sigmas)
    s2 = scale(area(z, present), area(mu, has))
    total = np.zeros((M, T), f32)
    k = np.zeros((M, T), np.int64)
    with np.errstate(all="ignore"):
        for p in range(P):
            dx = (z[:, None, p, 0] - mu[None, :, p, 0]).astype(f32)
            dy = (z[:, None, p, 1] - mu[None, :, p, 1]).astype(f32)
            d2 = ((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32)
            e = (d2 / (s2 * v2[p]).astype(f32)).astype(f32)
            common = present[:, None, p] & has[None, :, p] & ~np.isnan(e)
            c = oks_exp(e)
            total = np.where(common, np.where(k > 0, total + c, c), total).astype(f32)
            k += common
        w = (total / k.astype(f32)).astype(f32)
        ok = (k >= min_common) & (k > 0) & (s2 > f32(0))
    return np.where(ok, w, f32(np.nan)).astype(f32)


def vote(w, threshold=THRESHOLD):
    return PR.vote(w, threshold)


def sigmas_for(P):
    """Per-point constants for a bank of P points: COCO's for 17, otherwise a spread over COCO's range."""
    coco = np.array([.026, .025, .025, .035, .035, .079, .079, .072, .072, .062, .062, .107, .107, .087, .087, .089, .089], f32)
    return coco if P == 17 else np.linspace(0.025, 0.107, P).astype(f32)


# ---- the life cycle under OKS: pose_sort_ref.RefSort with the weight matrix replaced ------------------------------------------------
class OksSort(SR.RefSort):
    def __init__(self, P, sigmas, max_idle_epochs=5, cons=(), min_common=1, threshold=THRESHOLD, coast=True):
        super().__init__(P, max_idle_epochs, cons, min_common, threshold, coast)
        self.sigmas = np.asarray(sigmas, f32)

    def weights(self, pl, k, poses, present):
        has, mean, cov = self.states_of(pl["tracks"][k])
        m = len(poses)
        if m == 0 or len(has) == 0:
            z = np.full((m, len(has)), np.nan, f32)
            return z, np.zeros((m, len(has)), bool), z
        w = weights(poses, present, has, mean, self.sigmas, self.min_common)
        g, no = SR.gate(w, poses, present, has, mean, pl["limits"][k])
        return g, no, w


# ---- the scenes of tests/test_gpu_oks.py, checked on the model alone by tests/test_oks_scenes_ref.py --------------------------------
class Scene:
    """pose_ref's people, tracks from four rounds of step, the poses of the next frame: test_gpu_pose.Scene's recipe without the seeded
    indefinite state (OKS reads no covariance).  Read-only once built; the model's matrices are computed once."""

    def __init__(self, m, T, P, crowd, grid=False):
        rng = np.random.default_rng(7000 + 1000 * P + 10 * m + T)
        self.m, self.T, self.P = m, T, P
        self.ids = (np.arange(T, dtype=np.uint64) * 3 + 5)
        self.sigmas = sigmas_for(P)
        centres = PR.people(rng, T, P, crowd)
        if grid:   # multiples of 4 below 1024: exact in f16 and in bf16, so a 16-bit source shows the poses where the tracks are
            centres = np.round(centres / 4.0) * 4.0
        self.rounds = PR.track_rounds(rng, centres)
        self.model = PR.model_bank(self.rounds)
        self.poses, self.pres = PR.poses_of(rng, centres, m, noise=0.0 if grid else 0.05)
        for a in (self.poses, self.pres):
            a.setflags(write=False)
        self._w, self._vote = {}, {}

    def weights(self, min_common=1):
        if min_common not in self._w:
            w = weights(self.poses, self.pres, self.model.has, self.model.mean, self.sigmas, min_common)
            w.setflags(write=False)
            self._w[min_common] = w
        return self._w[min_common]

    def mahalanobis(self, min_common=1):
        return PR.weights(self.poses, self.pres, self.model.has, self.model.mean, self.model.cov, min_common=min_common)

    def vote(self, min_common=1, threshold=THRESHOLD):
        key = (min_common, threshold)
        if key not in self._vote:
            self._vote[key] = PR.vote(self.weights(min_common), threshold)
        return self._vote[key]


_scenes = {}
VOTE_SHAPES = [(3, 5), (17, 70), (70, 17)]
CROWD = (150, 150, 2)


def scene(m, T, P, crowd=False, grid=False):
    key = (m, T, P, crowd, grid)
    if key not in _scenes:
        _scenes[key] = Scene(m, T, P, crowd, grid)
    return _scenes[key]


SORT_PEOPLE = [7, 18]      # per camera; 18 people and the newcomers cross the 16-row tile
SORT_CONS = [(1, 1.0)]
SORT_FRAMES, SORT_IDLE = 8, 2
_sort = {}


def sort_sigmas(P):
    """Wide per-point tolerances, of the order of a body: a neighbour ten units away still has a weight above the diagonal — a real
    assignment problem without the gate, and pairs for the gate to refuse (the circles of two neighbours do not touch)."""
    return np.linspace(0.8, 1.2, P).astype(f32)


def sort_frames(P=17, seed=91):
    """Eight frames of two cameras.  People stand on pose_ref's lattice; every camera has people who are away for one epoch (they coast
    and come back), one who is away from epoch 3 on (their track expires: SORT_IDLE = 2) and one who arrives at epoch 4; a fifth of the
    points of a pose are absent.  Pose 1 of camera 2 has no present point in epoch 5.  -> [[(scene, poses, present), ...] x 8]"""
    if (P, seed) in _sort:
        return _sort[(P, seed)]
    rng = np.random.default_rng(seed)
    centres = [PR.people(rng, n + 1, P, False) + 400.0 * k for k, n in enumerate(SORT_PEOPLE)]
    frames = []
    for e in range(1, SORT_FRAMES + 1):
        fr = []
        for k, n in enumerate(SORT_PEOPLE):
            here = np.ones(n + 1, bool)
            here[n] = e >= 4                       # the newcomer
            here[0] = e < 3                        # leaves for good
            here[1 + (e % 3)] = e in (1, 8)        # away for an epoch, in turn
            shown = rng.permutation(np.flatnonzero(here))
            z = (centres[k][shown] + rng.normal(0, 0.05, (len(shown), P, 2))).astype(f32)
            pres = rng.random((len(shown), P)) >= 0.2
            if k == 1 and e == 5:
                pres[1] = False
            fr.append((k + 1, z, pres))
        frames.append(fr)
    _sort[(P, seed)] = frames
    return frames


def sort_model(gated, P=17):
    return OksSort(P, sort_sigmas(P), SORT_IDLE, SORT_CONS if gated else [])
