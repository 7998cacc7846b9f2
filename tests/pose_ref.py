"""The keypoint association of include/similari_pose.h as a numpy f32 model.  TEST INFRASTRUCTURE: what similari_amd/csrc/sa_pose.h,
the kernels of sa_pose.hip and PoseBank.associate are compared with.

The pair weight is built on points_ref.distance and points_ref.cost (the dense restatement of the reference's point filter): per point
the squared Mahalanobis distance and calculate_cost(d2, inverted = True), then the f32 sum over the common points in ascending p — a
loop seeded by the first term, never np.sum, which adds pairwise — divided by their number.  The vote is SortVoting::winners
(sort/voting.rs): the oracle's kuhn_munkres on the dense M x (M + T) matrix, weights (w * 1e6f) as i64, diagonal (threshold * 1e6f)
as i64, exactly as dense_reference of tests/test_device_logic_emu.py builds it."""
import ctypes as C

import numpy as np

import oracle_lib as O
import points_ref as R

f32 = np.float32


def weights(poses, present, has, mean, cov, pw=R.PW, min_common=1):
    """poses [M, P, 2], present [M, P] bool; has [T, P] bool, mean [T, P, 4], cov [T, P, 4, 4] -> w [M, T] f32, NaN = no pair."""
    poses, present, has = np.asarray(poses, f32), np.asarray(present, bool), np.asarray(has, bool)
    M, P = present.shape
    T = has.shape[0]
    z = np.where(present[..., None], poses, f32(0))   # an absent point may hold anything, NaN included
    mean = np.where(has[..., None], mean, f32(0)).astype(f32)
    cov = np.where(has[..., None, None], cov, f32(0)).astype(f32)
    total = np.zeros((M, T), f32)
    k = np.zeros((M, T), np.int64)
    with np.errstate(all="ignore"):
        for p in range(P):
            d2 = R.distance(mean[None, :, p], cov[None, :, p], z[:, None, p], pw)   # [M, T]
            common = present[:, None, p] & has[None, :, p] & ~np.isnan(d2)
            c = R.cost(d2, True)
            total = np.where(common, np.where(k > 0, total + c, c), total).astype(f32)
            k += common
        w = total / k.astype(f32)
    return np.where((k >= min_common) & (k > 0), w, f32(np.nan)).astype(f32)


def quantised(w, threshold=1.0):
    """-> (SortVoting's dense matrix [M, M + T] i64, threshold_q)"""
    w = np.asarray(w, f32)
    M, T = w.shape
    L = O.lib()
    thr_q = L.or_quantise(float(f32(threshold)))
    wq = np.zeros((M, M + T), np.int64)
    for i in range(M):
        for j in np.flatnonzero(~np.isnan(w[i])):
            wq[i, M + j] = L.or_quantise(float(w[i, j]))
        wq[i, i] = thr_q
    return wq, thr_q


def solve(wq):
    """kuhn_munkres on the dense matrix -> (total, match [M]: column of w or -1)"""
    M = wq.shape[0]
    if M == 0:
        return 0, np.zeros(0, np.int64)
    wq = np.ascontiguousarray(wq, np.int64)
    total = C.c_int64()
    assign = np.zeros(M, np.uint32)
    rc = O.lib().or_kuhn_munkres(M, wq.shape[1], wq.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(total), assign.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == 0
    return total.value, np.where(assign >= M, assign.astype(np.int64) - M, -1)


def vote(w, threshold=1.0):
    """-> (total of the dense matrix, match [M], wq, threshold_q).  A pose matched to a track whose weight does not exceed the diagonal
    is as good as unmatched; kuhn_munkres never prefers it over the row's own diagonal cell unless they tie, so it reads -1 here."""
    wq, thr_q = quantised(w, threshold)
    total, match = solve(wq)
    M = len(match)
    for i in range(M):
        if match[i] >= 0 and wq[i, M + match[i]] <= thr_q:
            match[i] = -1
    return total, match, wq, thr_q


def total_of(match, wq, thr_q):
    """The dense matrix's total of a matching given as columns of w (or -1): matched cells plus the diagonal of every other row."""
    M = wq.shape[0]
    return int(sum(int(wq[i, M + match[i]]) if match[i] >= 0 else int(thr_q) for i in range(M)))


def forced_rows(wq, total, match, rows=None):
    """Which rows of the optimum `match` are the same in EVERY optimum: row i is forced iff forbidding its cell lowers the total.
    rows: solve for these rows only (None: all) -> [M] bool, False for a row that was not asked about."""
    M = wq.shape[0]
    out = np.zeros(M, bool)
    for i in range(M) if rows is None else (int(r) for r in rows):
        alt = wq.copy()
        alt[i, M + match[i] if match[i] >= 0 else i] = 0
        out[i] = solve(alt)[0] < total
    return out


def greedy_roots(wq, thr_q):
    """The greedy start on the model's matrix: every row bids for the column of its heaviest gain (lowest column on ties), a column
    goes to the lowest row that bids for it -> the number of rows that lost their bid."""
    M = wq.shape[0]
    gain = wq[:, M:] - thr_q
    owner, lost = {}, 0
    for i in range(M):
        if gain.shape[1] == 0 or gain[i].max() <= 0:
            continue
        j = int(np.argmax(gain[i]))   # the first of the maxima
        if j in owner:
            lost += 1
        else:
            owner[j] = i
    return lost


# ---- scenes: people as P keypoints, tracks grown by four rounds of step, the poses of the next frame -------------------------------
def people(rng, n, P, crowd, spacing=10.0, extent=1000.0):
    """The keypoints [n, P, 2] of n people.  Apart: on a lattice `spacing` apart, so nobody lies inside another's gate (the filter's
    position deviation is ~0.1).  crowd: in clusters of about six, 0.05 apart — tighter than the gate, so several poses want one
    track —, the clusters anywhere in `extent`."""
    if crowd:
        nc = max(n // 6, 1)
        centre = rng.uniform(0, extent, (nc, 1, 2))
        base = centre[rng.integers(0, nc, n)] + rng.normal(0, 0.05, (n, 1, 2))
    else:
        side = int(np.ceil(np.sqrt(n)))
        cell = rng.permutation(side * side)[:n]
        base = (np.stack([cell % side, cell // side], -1) * spacing)[:, None, :] + rng.uniform(0, spacing / 10, (n, 1, 2))
    return base + rng.uniform(-3, 3, (1, P, 2))


def hall(seed, M, T, P, side=100.0, sigma=50.0, corner=None):
    """A packed hall, built from the model alone (no filter ran): T tracks anywhere in [0, side]^2 whose position deviation `sigma` is
    of the order of the hall, so nearly every pose lies inside nearly every track's gate, the weights spread over the whole live range
    of the cost and the scene is ONE component; M poses anywhere in [0, corner or side]^2 (a corner: many poses for few near tracks).
    Everybody has the same skeleton.  A tenth of the tracks' points are absent (no track loses all), a quarter of the poses' points;
    x and y of every covariance are correlated, up to +-0.3.  -> (poses [M, P, 2] f32, present [M, P], has [T, P], mean [T, P, 4] f32,
    cov [T, P, 4, 4] f32)"""
    rng = np.random.default_rng(seed)
    skeleton = rng.uniform(-3, 3, (1, P, 2))
    centres = rng.uniform(0, side, (T, 1, 2))
    has = rng.random((T, P)) >= 0.1
    has[~has.any(1), 0] = True
    mean = np.zeros((T, P, 4), f32)
    mean[..., :2] = centres + skeleton
    sd = rng.uniform(0.8, 1.2, (T, P)) * sigma
    cov = np.zeros((T, P, 4, 4), f32)
    cov[..., 0, 0] = cov[..., 1, 1] = sd * sd
    cov[..., 2, 2] = cov[..., 3, 3] = 1
    cov[..., 0, 1] = cov[..., 1, 0] = 0.3 * sd * sd * rng.uniform(-1, 1, (T, P))
    poses = rng.uniform(0, corner or side, (M, 1, 2)) + skeleton + rng.normal(0, 1, (M, P, 2))
    return poses.astype(f32), rng.random((M, P)) >= 0.25, has, mean, cov


def track_rounds(rng, centres, rounds=4, absent=0.3, never=0.1, noise=0.03):
    """What the tracks were shown: `rounds` x (z [T, P, 2] f32, present [T, P]); `never`: the share of points never sighted."""
    T, P = centres.shape[:2]
    nev = rng.random((T, P)) < never
    return [((centres + rng.normal(0, noise, centres.shape)).astype(f32), (rng.random((T, P)) >= absent) & ~nev) for _ in range(rounds)]


def model_bank(rounds, pw=R.PW, vw=R.VW):
    bank = R.Bank(rounds[0][1].shape, pw, vw)
    for z, pres in rounds:
        bank.step(z, pres)
    return bank


def poses_of(rng, centres, M, absent=0.3, noise=0.05, new=0.2):
    """The next frame: pose i continues a track of its own (a random one, while there are any) or, with probability `new`, shows
    somebody new far away -> (poses [M, P, 2] f32, present [M, P])."""
    T, P = centres.shape[:2]
    src = rng.permutation(T)
    poses = np.empty((M, P, 2))
    for i in range(M):
        if i < T and rng.random() >= new:
            poses[i] = centres[src[i]] + rng.normal(0, noise, (P, 2))
        else:
            poses[i] = 5000.0 + 10.0 * i + rng.uniform(-3, 3, (P, 2))
    return poses.astype(f32), rng.random((M, P)) >= absent
