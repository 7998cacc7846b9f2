"""Host restatement of track search: TrackStore::foreign_track_distances + TopNVoting::winners (src/track/store.rs:199-240, 429-460;
src/track.rs:604-652; src/track/voting/topn.rs:82-135), steps 1-8 of include/similari_search.h.  Test infrastructure only.

winners(): TopNVoting::winners on a list of (query id, winner id, distance or None) in the order the reference produces them.
restate(): the whole search on a cell matrix [Q][K][T][K] (NaN = absent observation), as sa_store_search_topn(out_cells) returns it.
Ranking: weight descending, then winner id ascending (the reference leaves ties in HashMap order)."""
from __future__ import annotations

import math

import numpy as np

f32 = np.float32


def winners(metrics, topn, max_distance, min_votes=1):
    """TopNVoting::winners over (query, winner, distance | None) triples: {query: [(winner, weight), ...]}, and M."""
    M = f32(-1.0)
    md = f32(max_distance)
    groups = {}
    for q, w, d in metrics:
        if d is None:
            continue
        d = f32(d)
        if M < d:
            M = d
        if d <= md:
            groups.setdefault((int(q), int(w)), []).append(d)
    res = {}
    need = max(1, int(min_votes))
    for (q, w), ds in groups.items():
        if len(ds) < need:
            continue
        weight = 0.0
        for d in ds:
            weight += float(f32(M - d))
        res.setdefault(q, []).append((w, weight))
    for q in res:
        res[q].sort(key=lambda e: (-e[1], e[0]))
        res[q] = res[q][: int(topn)]
    return res, M


def pair_metrics(q_ids, s_ids, cells, keep_below=math.inf):
    """Steps 1-3 as the reference produces them: (query, stored track, d) per observation pair in cartesian order, query tracks in
    order, stored tracks in column order; self pairs skipped; d >= keep_below dropped; absent observations (NaN) left out — a NaN
    distance the reference would keep behaves the same in winners() (it neither raises M nor is kept)."""
    kb = f32(keep_below)
    cells = np.asarray(cells, f32)
    Q, K, T, _ = cells.shape
    out = []
    for qi in range(Q):
        for ti in range(T):
            if int(q_ids[qi]) == int(s_ids[ti]):
                continue
            for a in range(K):
                for b in range(K):
                    d = cells[qi, a, ti, b]
                    if np.isnan(d) or d >= kb:
                        continue
                    out.append((int(q_ids[qi]), int(s_ids[ti]), d))
    return out


def restate(q_ids, s_ids, cells, topn, max_distance, min_votes=1, keep_below=math.inf):
    """Steps 1-8 vectorised over a cell matrix [Q][K][T][K] (f32; NaN = absent): ({query: [(winner, weight), ...]}, M).
    Weights are sequential f64 sums (np.cumsum) of f64(f32(M - d)) over the kept cells in row-major order of the group."""
    q_ids = np.asarray(q_ids, np.uint64).reshape(-1)
    s_ids = np.asarray(s_ids, np.uint64).reshape(-1)
    d = np.asarray(cells, f32)
    Q, K, T, _ = d.shape
    self_pair = q_ids[:, None] == s_ids[None, :]
    with np.errstate(invalid="ignore"):
        valid = ~np.isnan(d) & ~self_pair[:, None, :, None] & ~(d >= f32(keep_below))
        M = f32(-1.0)
        if valid.any():
            M = max(M, d[valid].max())
        kept = valid & (d <= f32(max_distance))
    counts = kept.sum(axis=(1, 3))
    need = max(1, int(min_votes))
    res = {}
    for qi in range(Q):
        cand = []
        for ti in np.nonzero(counts[qi] >= need)[0]:
            vals = d[qi, :, ti, :][kept[qi, :, ti, :]]
            w = float(np.cumsum((M - vals).astype(f32).astype(np.float64))[-1])
            cand.append((int(s_ids[ti]), w))
        if cand:
            cand.sort(key=lambda e: (-e[1], e[0]))
            res[int(q_ids[qi])] = cand[: int(topn)]
    return res, M


def first_difference(a, b):
    """The first rank where two winner lists part, and the winner each holds there (None past its end); None when they agree."""
    for r in range(max(len(a), len(b))):
        x = a[r] if r < len(a) else None
        y = b[r] if r < len(b) else None
        if x != y:
            return r, x, y
    return None


def explained(x, y, weights, near_groups, spread):
    """Whether the decision between groups x and y (winner ids; None = no group at that rank) is a borderline one: one of them has a
    distance within the tolerance of max_distance or keep_below (its kept cells may differ), or both exist with exact weights within
    `spread` of each other."""
    if any(g is not None and g in near_groups for g in (x, y)):
        return True
    return x is not None and y is not None and x in weights and y in weights and abs(weights[x] - weights[y]) <= spread


def compare_winners(q_ids, s_ids, exact, approx, topn, max_distance, tol, min_votes=1, keep_below=math.inf):
    """Winner lists of the restatement on `approx` (engine distances) against those on `exact` (oracle distances).  A query's list may
    differ only through a borderline decision, tied to the groups that part first: one of them has a distance within `tol` of max_distance
    or keep_below, or their exact weights lie within the spread that `tol` allows (tol on every cell of both groups and on M).  Returns
    (queries whose lists differ, the ones no borderline decision explains, borderline groups counted)."""
    ra, _ = restate(q_ids, s_ids, exact, topn, max_distance, min_votes, keep_below)
    rb, _ = restate(q_ids, s_ids, approx, topn, max_distance, min_votes, keep_below)
    full, _ = restate(q_ids, s_ids, exact, 1 << 30, max_distance, min_votes, keep_below)
    ex = np.asarray(exact, f32)
    with np.errstate(invalid="ignore"):
        near = ((np.abs(ex - f32(max_distance)) <= tol) | (np.abs(ex - f32(keep_below)) <= tol)).any(axis=(1, 3))
    s_ids = np.asarray(s_ids, np.uint64)
    K = ex.shape[1]
    spread = 4.0 * tol * K * K
    differ, unexplained = [], []
    for qi, q in enumerate(np.asarray(q_ids, np.uint64)):
        a = [w for w, _ in ra.get(int(q), [])]
        b = [w for w, _ in rb.get(int(q), [])]
        d = first_difference(a, b)
        if d is None:
            continue
        differ.append(int(q))
        near_groups = {int(s_ids[t]) for t in np.nonzero(near[qi])[0]}
        if not explained(d[1], d[2], dict(full.get(int(q), [])), near_groups, spread):
            unexplained.append(int(q))
    return differ, unexplained, int(near.sum())
