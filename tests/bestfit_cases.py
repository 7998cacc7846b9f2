"""The data of tests/test_gpu_bestfit.py and what chose it: seeded banks, attributes, and the contention case of the issue with the
seeds its thresholded variant was chosen for.  The choice is made on the host — host_cells: f64 numpy distances rounded to f32,
then tests/bestfit_ref.py — and tests/test_bestfit_ref.py asserts that the committed seeds have the property on those distances;
the GPU test asserts it again on the engine's own cells.  Test infrastructure only."""
import numpy as np

from similari_amd import attrs as A

D33 = 33   # no multiple of the 32-float row pad


def rows(rng, k, D, kind):
    f = rng.uniform(0, 1, (k, D)).astype(np.float32)
    return f - 0.5 if kind == "cosine" else f


def banks(rng, n, K, D, kind, ragged=True):
    return [rows(rng, int(rng.integers(1, K + 1)) if ragged and i % 3 else K, D, kind) for i in range(n)]


def packed(attrs):
    return A.pack_attrs([a[0] for a in attrs], [a[1] for a in attrs], [a[2] for a in attrs])


def spans(rng, n):
    start = rng.integers(0, 100, n)
    return [(int(rng.integers(1, 3)), int(s), int(s + rng.integers(0, 40))) for s in start]


def quantile(cells, q):
    return float(np.quantile(cells[~np.isnan(cells)], q))


def host_distances(kind, a, b):
    """what the engine computes, in f64 on the host: for choosing a case, never for checking one"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    dot = a @ b.T
    na, nb = (a * a).sum(1), (b * b).sum(1)
    if kind == "cosine":
        return dot / np.sqrt(na[:, None] * nb[None, :])
    return np.sqrt(np.maximum(na[:, None] + nb[None, :] - 2.0 * dot, 0.0))


def host_cells(kind, q_feats, s_feats, K):
    """[Q][K][T][K] from host_distances, NaN where an observation is absent"""
    D = next(f.shape[1] for f in s_feats if f is not None and len(f))
    pad = lambda f: np.concatenate([np.zeros((0, D)) if f is None else f, np.full((K - (0 if f is None else len(f)), D), np.nan)])
    q, s = np.stack([pad(f) for f in q_feats]), np.stack([pad(f) for f in s_feats])
    with np.errstate(invalid="ignore"):
        d = host_distances(kind, q.reshape(-1, D), s.reshape(-1, D))
    return d.reshape(len(q_feats), K, len(s_feats), K).astype(np.float32)


# ---- the contention case ----
CONTENTION_SEED = {"cosine": 25, "euclidean": 27}   # chosen on the host (host_cells + bestfit_ref) for the thresholded variant below
CONTENTION_QUANTILE = 0.45


def contention_case(kind, seed):
    """T = 5 (the last stored track has no observations), Q = 8 noisy copies of stored tracks 0 and 1 (one query has none), K = 3,
    ragged on both sides"""
    rng = np.random.default_rng(seed)
    K = 3
    s_feats = [rows(rng, k, D33, kind) for k in (3, 2, 3, 1)] + [None]
    q_feats = []
    for i in range(8):
        src = s_feats[i % 2]
        q_feats.append((src[rng.integers(0, len(src), 1 + i % 3)] + rng.normal(0, 0.15, (1 + i % 3, D33))).astype(np.float32))
    q_feats[5] = None
    return K, np.arange(11, 16), s_feats, np.arange(101, 109), q_feats


def loses_first_wins_later(res):
    return [q for q, lst in res.items() if lst[0][0] == q and any(w == t for w, _, t in lst[1:])]


def contention_thresholded(kind, cells):
    """(max_distance, min_votes) of the thresholded variant on a tap of the unthresholded call"""
    return quantile(cells, CONTENTION_QUANTILE), 2


def queries_without_a_group(res, q_ids, q_feats):
    """queries that have observations and no group"""
    return [int(q) for q, f in zip(q_ids, q_feats) if f is not None and int(q) not in res]
