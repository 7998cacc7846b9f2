"""Track search timing: FeatureStore.search_topn (include/similari_search.h) on the layouts of the reference's benches
(benches/track_search.rs, benches/feature_tracker.rs) and one re-identification size, one JSON line per configuration.

Per line: device-event microseconds of launch 1 (contraction + group epilogue), launch 2 (weights + top-N) and the whole call, the
call's wall time with the query upload and the result download, launch 1's share of peak against both bounds — algorithmic FLOPs
(2 rows cols D, padding not counted) over the 157.3 TF/s f32 MFMA peak, and store plus query bytes over 8 TB/s of HBM — with the
binding one named, the padding overhead, the surviving groups, whether the first call reran on a grown pool, and `match`: the winners
equal the host restatement (tests/topn_ref.py steps) on f64 numpy distances apart from borderline decisions, each tied to the
groups whose ranks part (`differ` counts the queries whose lists differ at all).
   python scripts/bench_search.py [--quick] [--reps N]"""
import argparse
import json
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    sys.path.insert(0, p)
from similari_amd import abi, synth  # noqa: E402
from similari_amd.engine import Engine  # noqa: E402
from similari_amd.search import FeatureStore  # noqa: E402
import topn_ref as R  # noqa: E402

PEAK_F32_MFMA = 157.3e12
HBM = 8.0e12
f32 = np.float32


def host_distances(kind, qf, sf):
    """[Q*K][C*K] f64 distances of query rows against a chunk of stored rows."""
    a = qf.astype(np.float64)
    b = sf.astype(np.float64)
    dot = a @ b.T
    na = (a * a).sum(1)
    nb = (b * b).sum(1)
    if kind == "cosine":
        with np.errstate(invalid="ignore", divide="ignore"):
            return dot / np.sqrt(na[:, None] * nb[None, :])
    return np.sqrt(np.maximum(na[:, None] + nb[None, :] - 2.0 * dot, 0.0))


def host_search(kind, q_ids, qf, s_ids, sf, topn, md, kb, tol, chunk=400):
    """Steps 1-8 on f64 distances rounded to f32, the store walked in chunks (a [Q][K][T][K] matrix at the re-ID size is 10 GB).
    Returns ({query: [(winner, weight)]}, {query: {winner: weight}} of every group, {query: {stored track with a borderline cell}})."""
    Q, Kq, D = qf.shape
    T, Ks = sf.shape[:2]
    M = f32(-1.0)
    kept_blocks = {}
    near = {}
    qrows = qf.reshape(Q * Kq, D)
    self_pair = q_ids[:, None] == s_ids[None, :]
    for t0 in range(0, T, chunk):
        t1 = min(T, t0 + chunk)
        d = host_distances(kind, qrows, sf[t0:t1].reshape(-1, D)).astype(f32).reshape(Q, Kq, t1 - t0, Ks)
        valid = ~np.isnan(d) & ~self_pair[:, None, t0:t1, None] & ~(d >= f32(kb))
        if valid.any():
            M = max(M, d[valid].max())
        kept = valid & (d <= f32(md))
        with np.errstate(invalid="ignore"):
            nearg = ((np.abs(d - f32(md)) <= tol) | (np.abs(d - f32(kb)) <= tol)).any(axis=(1, 3))
        for qi, ti in zip(*np.nonzero(nearg)):
            near.setdefault(int(q_ids[qi]), set()).add(int(s_ids[t0 + ti]))
        cnt = kept.sum(axis=(1, 3))
        for qi, ti in zip(*np.nonzero(cnt >= 1)):
            kept_blocks[(qi, t0 + ti)] = d[qi, :, ti, :][kept[qi, :, ti, :]]
    full = {}
    for (qi, ti), vals in kept_blocks.items():
        w = float(np.cumsum((M - vals).astype(f32).astype(np.float64))[-1])
        full.setdefault(int(q_ids[qi]), {})[int(s_ids[ti])] = w
    res = {q: sorted(g.items(), key=lambda e: (-e[1], e[0]))[:topn] for q, g in full.items()}
    return res, full, near


def matches(got, want, full, near, spread):
    """(match, queries that differ, of those the ones a borderline decision explains).  The explanation is tied to the decision that
    differs — the first rank where the lists part — as in tests/topn_ref.compare_winners."""
    differ, explained = 0, 0
    for q in set(got) | set(want):
        a = [w for w, _ in got.get(q, [])]
        b = [w for w, _ in want.get(q, [])]
        d = R.first_difference(a, b)
        if d is None:
            continue
        differ += 1
        explained += R.explained(d[1], d[2], full.get(q, {}), near.get(q, set()), spread)
    return differ == explained, differ, explained


def run(eng, name, kind, q_ids, qf, s_ids, sf, topn, md, kb=math.inf, mv=1, reps=5):
    Q, Kq, D = qf.shape
    T, Ks = sf.shape[:2]
    K = max(Kq, Ks)
    store = FeatureStore(eng, kind, D, K)
    try:
        for t0 in range(0, T, 1000):   # upsert in slices: the host staging of one call is [n][Kp][D]
            store.upsert(s_ids[t0:t0 + 1000], list(sf[t0:t0 + 1000]))
        got = store.search_topn(q_ids, list(qf), topn, md, mv, kb)
        first = store.last_stats()
        l1, l2, call, wall = [], [], [], []
        for _ in range(reps):
            t = time.perf_counter()
            store.search_topn(q_ids, list(qf), topn, md, mv, kb)
            wall.append(time.perf_counter() - t)
            st = store.last_stats()
            l1.append(st["launch1_ms"])
            l2.append(st["launch2_ms"])
            call.append(st["call_ms"])
        order = store.order()
    finally:
        store.close()
    assert np.array_equal(order, s_ids)
    tol = 1e-5 if kind == "cosine" else 1e-5 * max(1.0, float(md) if math.isfinite(md) else 1.0)
    want, full, near = host_search(kind, q_ids, qf, s_ids, sf, topn, md, kb, tol)
    ok, differ, explained = matches(got, want, full, near, 4.0 * tol * K * K)
    rows, cols = Q * Kq, T * Ks
    flops = 2.0 * rows * cols * D
    nbytes = 4.0 * (rows + cols) * D
    Kp = 1 << (K - 1).bit_length()
    Dp = (D + 31) // 32 * 32
    t1 = float(np.median(l1)) * 1e-3
    b_mfma, b_hbm = flops / PEAK_F32_MFMA, nbytes / HBM
    line = {
        "config": name, "kind": kind, "queries": Q, "query_observations": Kq, "tracks": T, "track_observations": Ks, "D": D, "topn": topn,
        "max_distance": round(float(md), 6), "keep_below": None if math.isinf(kb) else kb,
        "launch1_us": round(t1 * 1e6, 1), "launch2_us": round(float(np.median(l2)) * 1e3, 1),
        "call_us": round(float(np.median(call)) * 1e3, 1), "wall_us": round(float(np.median(wall)) * 1e6, 1),
        "mfma_bound_us": round(b_mfma * 1e6, 2), "hbm_bound_us": round(b_hbm * 1e6, 2),
        "binding": "mfma" if b_mfma >= b_hbm else "hbm", "launch1_share_of_peak": round(max(b_mfma, b_hbm) / t1, 3),
        "padding_overhead": round((Q * Kp) * (T * Kp) * Dp / (rows * cols * D) - 1.0, 3),
        "groups": first["groups"], "pool_rerun": bool(first["reruns"]), "match": ok, "differ": differ, "borderline": explained,
    }
    print(json.dumps(line), flush=True)
    return ok


def reid_threshold(kind, qf, sf, frac, rng):
    """max_distance that keeps about `frac` of the (query, track) groups (one kept cell makes a group): from a sample of groups' best cells."""
    Q, Kq, D = qf.shape
    t = rng.choice(sf.shape[0], min(400, sf.shape[0]), replace=False)
    d = host_distances(kind, qf.reshape(Q * Kq, D), sf[t].reshape(-1, D)).reshape(Q, Kq, len(t), sf.shape[1])
    best = d.min(axis=(1, 3))
    return float(np.quantile(best, frac))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="the small layouts only")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    eng = Engine(abi.make_config(device=0))
    ok = True
    try:
        rng = np.random.default_rng(0)
        # benches/track_search.rs: one 30-observation query against 100 / 1000 tracks of 30, U(0, 1) features
        for T in (100, 1000):
            for D in (256, 512, 1024):
                sf = rng.uniform(0, 1, (T, 30, D)).astype(f32)
                qf = rng.uniform(0, 1, (1, 30, D)).astype(f32)
                md = reid_threshold("euclidean", qf, sf, 0.1, rng)
                ok &= run(eng, "track_search", "euclidean", np.array([T + 1], np.uint64), qf, np.arange(1, T + 1, dtype=np.uint64), sf,
                          5, md, reps=args.reps)
        # benches/feature_tracker.rs: N one-observation queries against N tracks of 3, TopN(1, 100, 1), keep_below 100
        for N in (10, 100, 500):
            ident = synth.reid_identities(rng, N, 256)
            sf = np.stack([synth.observe(rng, ident) for _ in range(3)], axis=1)
            qf = synth.observe(rng, ident)[:, None, :]
            ok &= run(eng, "feature_tracker", "euclidean", np.arange(N + 1, 2 * N + 1, dtype=np.uint64), qf,
                      np.arange(1, N + 1, dtype=np.uint64), sf, 1, 100.0, kb=100.0, reps=args.reps)
        if not args.quick:
            # re-identification: 64 queries x 32 observations against 20 000 tracks x 32, 512-d, about 1 % of the groups surviving
            T, Q, K, D = 20000, 64, 32, 512
            ident = synth.reid_identities(rng, T, D)
            sf = np.empty((T, K, D), f32)
            for k in range(K):
                sf[:, k] = synth.observe(rng, ident, 0.05)
            pick = rng.choice(T, Q, replace=False)
            qf = np.stack([synth.observe(rng, ident[pick], 0.05) for _ in range(K)], axis=1)
            for kind in ("cosine", "euclidean"):
                md = reid_threshold(kind, qf, sf, 0.01, rng)   # (cosine keeps d <= max_distance of the similarity: the reference's quirk)
                ok &= run(eng, "reid", kind, np.arange(T + 1, T + Q + 1, dtype=np.uint64), qf, np.arange(1, T + 1, dtype=np.uint64), sf,
                          10, md, reps=args.reps)
    finally:
        eng.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
