"""BestFit search timing (include/similari_bestfit.h) beside the TopN call with the same parameters on the same store, in one
process, one JSON line per configuration (stdout, and appended to --out; by default profiles/bestfit_search.jsonl, and no file
for a --quick run, whose lines carry "quick": true):

  gallery_join   the two seeded galleries of scripts/bench_gallery.py (4096 x 8 and 8192 x 4, 512-d) joined with themselves
  reid           64 queries x 32 observations against 20 000 tracks x 32, 512-d (scripts/bench_search.py), host-fed

(a) the BestFit call and (b) the TopN call alternate, 7 rounds after a warm-up round (which also grows the pool); device events.
Per line, medians with 10th / 90th percentiles in microseconds: launch 1 of both — the same kernel over the same data, so
`launch1_agree` says whether the two medians lie within the larger of the two spreads —, the three stage-2 launches of (a) and their
sum beside launch 2 of (b) (`stage2_over_topn_launch2`, the yardstick), `stage2_over_launch1`, the groups and claimed tracks of (a).
`host_check`: at a reduced size of the same data (256 tracks or 8 x 256) the winners, tracks and weight bits of (a) equal
tests/bestfit_ref.py on (a)'s own tap cells.
   python scripts/bench_bestfit.py [--quick] [--reps N] [--out FILE]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests"), str(ROOT / "scripts")):
    sys.path.insert(0, p)
from similari_amd import abi, synth  # noqa: E402
from similari_amd.bestfit import BestFitStore  # noqa: E402
from similari_amd.engine import Engine  # noqa: E402
import bestfit_ref as B  # noqa: E402
from bench_gallery import pair_threshold, pct  # noqa: E402
from bench_search import reid_threshold  # noqa: E402

f32 = np.float32
INF = float("inf")


def fill(store, ids, sf):
    for t0 in range(0, len(ids), 1000):   # upsert in slices: the host staging of one call is [n][Kp][D]
        store.upsert(ids[t0:t0 + 1000], list(sf[t0:t0 + 1000]))


def host_check(eng, kind, ids, sf, q_ids, qf, topn, md):
    """(a) against the restatement on (a)'s own tap; qf None: a join"""
    store = BestFitStore(eng, kind, sf.shape[2], sf.shape[1])
    try:
        fill(store, ids, sf)
        if qf is None:
            raw = store.join_bestfit_raw(topn, md, tap=True)
            q_ids, want = ids, B.join(ids, raw[4], md)
        else:
            raw = store.search_bestfit_raw(q_ids, list(qf), topn, md, tap=True)
            want = B.restate(q_ids, ids, raw[4], md)
        st = store.bestfit_stats()
    finally:
        store.close()
    ok = (st["groups"], st["claimed"]) == (want[1], want[2])
    res = B.cut(want[0], topn)
    for i, q in enumerate(q_ids):
        lst = res.get(int(q), [])
        n = len(lst)
        ok &= int(raw[0][i]) == n and [int(x) for x in raw[1][i, :n]] == [w for w, _, _ in lst] and [int(x) for x in raw[2][i, :n]] == [t for _, _, t in lst]
        ok &= bool(np.array_equal(raw[3][i, :n].view(np.uint64), np.array([w for _, w, _ in lst], np.float64).view(np.uint64)))
    return bool(ok)


def run(eng, name, kind, ids, sf, q_ids, qf, topn, md, reps, small, quick):
    T, K, D = sf.shape
    store = BestFitStore(eng, kind, D, K)
    feats = None if qf is None else list(qf)
    if qf is None:
        fit = lambda: store.join_bestfit_raw(topn, md)
        top = lambda: store.join_raw(topn, md)
    else:
        fit = lambda: store.search_bestfit_raw(q_ids, feats, topn, md)
        top = lambda: store.search_raw(q_ids, feats, topn, md)
    keys = ("launch1_us", "weigh_us", "claim_us", "rank_us", "stage2_us")
    a = {k: [] for k in keys}
    b = {"launch1_us": [], "launch2_us": []}
    try:
        fill(store, ids, sf)
        x, y = fit(), top()   # warm-up: buffers, the pool's growth
        same_lists = bool(np.array_equal(x[0], y[0]) and np.array_equal(x[2], y[1]) and np.array_equal(x[3].view(np.uint64), y[2].view(np.uint64)))
        for _ in range(reps):
            fit()
            st, fs = store.last_stats(), store.bestfit_stats()
            a["launch1_us"].append(st["launch1_ms"] * 1e3)
            for k in ("weigh", "claim", "rank"):
                a[k + "_us"].append(fs[k + "_ms"] * 1e3)
            a["stage2_us"].append(st["launch2_ms"] * 1e3)
            top()
            st = store.last_stats()
            b["launch1_us"].append(st["launch1_ms"] * 1e3)
            b["launch2_us"].append(st["launch2_ms"] * 1e3)
        blocks = st["groups"]
    finally:
        store.close()
    A, Bt = {k: pct(v) for k, v in a.items()}, {k: pct(v) for k, v in b.items()}
    spread = max(A["launch1_us"]["p90"] - A["launch1_us"]["p10"], Bt["launch1_us"]["p90"] - Bt["launch1_us"]["p10"])
    line = {"config": name, "quick": bool(quick), "kind": kind, "tracks": T, "observations": K, "D": D, "queries": T if qf is None else len(q_ids), "topn": topn,
            "max_distance": round(float(md), 6), "reps": reps, "bestfit": A, "topn_call": Bt, "pool_blocks": blocks,
            "groups": fs["groups"], "claimed": fs["claimed"], "lost": fs["groups"] - fs["claimed"],
            "launch1_agree": bool(abs(A["launch1_us"]["median"] - Bt["launch1_us"]["median"]) <= spread),
            "stage2_over_topn_launch2": round(A["stage2_us"]["median"] / Bt["launch2_us"]["median"], 3),
            "stage2_over_launch1": round(A["stage2_us"]["median"] / A["launch1_us"]["median"], 3),
            "tracks_are_topn_winners": same_lists, "host_check": host_check(eng, kind, *small, topn, md)}
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes only (512 x 4 x 128-d joined; 8 x 4 against 2000 x 4)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["gallery_join", "reid"], default=None)
    ap.add_argument("--out", default=None, help="file the lines are appended to (default: profiles/bestfit_search.jsonl; none with --quick)")
    args = ap.parse_args()
    reps = max(5, args.reps)
    eng = Engine(abi.make_config(device=0))
    ok = True
    path = args.out or (None if args.quick else str(ROOT / "profiles" / "bestfit_search.jsonl"))
    out = open(path, "a") if path else None

    def emit(line):
        nonlocal ok
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()
        ok &= line["host_check"] and line["tracks_are_topn_winners"]

    try:
        for kind in ("cosine", "euclidean"):
            if args.only in (None, "gallery_join"):
                for T, K, D in ([(512, 4, 128)] if args.quick else [(4096, 8, 512), (8192, 4, 512)]):
                    rng = np.random.default_rng(0)
                    ident = synth.reid_identities(rng, T, D)
                    sf = np.stack([synth.observe(rng, ident, 0.05) for _ in range(K)], axis=1).astype(f32)
                    ids = np.arange(1, T + 1, dtype=np.uint64)
                    md = pair_threshold(kind, sf, 0.01, rng)
                    emit(run(eng, "gallery_join", kind, ids, sf, None, None, 10, md, reps, (ids[:256], sf[:256], None, None), args.quick))
            if args.only in (None, "reid"):
                T, Q, K, D = (2000, 8, 4, 128) if args.quick else (20000, 64, 32, 512)
                rng = np.random.default_rng(0)
                ident = synth.reid_identities(rng, T, D)
                sf = np.empty((T, K, D), f32)
                for k in range(K):
                    sf[:, k] = synth.observe(rng, ident, 0.05)
                pick = rng.choice(T, Q, replace=False)
                qf = np.stack([synth.observe(rng, ident[pick], 0.05) for _ in range(K)], axis=1)
                ids, q_ids = np.arange(1, T + 1, dtype=np.uint64), np.arange(T + 1, T + Q + 1, dtype=np.uint64)
                md = reid_threshold(kind, qf, sf, 0.01, rng)
                emit(run(eng, "reid", kind, ids, sf, q_ids, qf, 10, md, reps, (ids[:256], sf[:256], q_ids[:8], qf[:8]), args.quick))
    finally:
        eng.close()
        if out:
            out.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
