"""An f16 feature store against an f32 store (include/similari_f16.h): the same seeded, f16-representable features in both, in one
process, for both metrics, one JSON line per size and metric:

  reid   the re-identification size of DESIGN section 10: 64 queries x 32 observations against 20 000 tracks x 32, 512-d, about 1 %
         of the groups surviving (host-fed queries, sa_store_search_topn)
  join   the whole-gallery join at 4096 tracks x 8, 512-d, about 1 % of the pairs surviving (sa_store_join_topn)

Calls on the two stores alternate, after one warm-up round (which also grows the pools).  Per store: median / 10th / 90th percentile
of launch 1, launch 2 and the whole call from the store's own device events (sa_search_stats, microseconds), and feature_bytes
(sa_store_get_info).  `launch1_gain` / `call_gain`: f32 over f16, medians; `launch1_p90_below_f32_p10`: the f16 store's slow end lies
below the f32 store's fast end.  The f32 store is the baseline: the same shape, the same process, the kernels the library had before
(for euclidean the direct sum on the vector pipe).  The rows are f16-representable, so both stores hold the same values and
`queries_differing` — how many queries' winner lists (ids, in order) differ — and `max_cell_move` (absolute for cosine, relative for
euclidean, over the tapped cells of a sample of queries) measure the arithmetic alone.  `expand`: what the f16 euclidean launch 1
recomputed directly (sa_store_expand_last: flagged cells, tiles that recomputed any) beside the cells and tiles it ran.
   python scripts/bench_f16.py [--quick] [--rounds N] [--out profiles/f16_store.jsonl]"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from similari_amd import abi, synth  # noqa: E402
from similari_amd.bestfit import BestFitStore  # noqa: E402
from similari_amd.f16 import F16Store, store_info  # noqa: E402
from similari_amd.engine import Engine  # noqa: E402
from similari_amd.search import _p, pack_tracks, sa_topn_params  # noqa: E402

f32 = np.float32
STORES = ("f32", "f16")


def host_cosine(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return (a @ b.T) / np.sqrt((a * a).sum(1)[:, None] * (b * b).sum(1)[None, :])


def host_euclid(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.sqrt(np.maximum((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T), 0.0))


def as_f16(x):
    """the nearest f16-representable values, as f32"""
    return x.astype(np.float16).astype(f32)


def threshold(kind, qf, sf, frac, rng, own=False):
    """max_distance that keeps about `frac` of the (query, track) groups — one kept cell makes a group — from a sample of tracks
    (own: the queries are those tracks themselves, the self pairs stay out)."""
    t = rng.choice(sf.shape[0], min(400, sf.shape[0]), replace=False)
    q = sf[t] if own else qf
    d = (host_cosine if kind == "cosine" else host_euclid)(q.reshape(-1, q.shape[2]), sf[t].reshape(-1, sf.shape[2])).reshape(q.shape[0], q.shape[1], len(t), sf.shape[1])
    best = d.min(axis=(1, 3))
    return float(np.quantile(best[~np.eye(len(t), dtype=bool)] if own else best, frac))


def pct(v):
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), 1), "p10": round(float(np.quantile(v, 0.1)), 1), "p90": round(float(np.quantile(v, 0.9)), 1)}


def beyond_spread(slow, fast):
    gap = slow["median"] - fast["median"]
    return bool(gap > max(slow["p90"] - slow["p10"], fast["p90"] - fast["p10"]))


def features(rng, T, K, D):
    ident = synth.reid_identities(rng, T, D)
    sf = np.empty((T, K, D), f32)
    for k in range(K):
        sf[:, k] = synth.observe(rng, ident, 0.05)
    return ident, as_f16(sf)


def run(eng, name, kind, T, K, D, Q, topn, rounds, rng, sample):
    ident, sf = features(rng, T, K, D)
    s_ids = np.arange(1, T + 1, dtype=np.uint64)
    join = Q == 0
    if join:
        qf, q_ids, n = None, s_ids, T
        md = threshold(kind, None, sf, 0.01, rng, own=True)
    else:
        pick = rng.choice(T, Q, replace=False)
        qf = as_f16(np.stack([synth.observe(rng, ident[pick], 0.05) for _ in range(K)], axis=1))
        q_ids, n = np.arange(T + 1, T + Q + 1, dtype=np.uint64), Q
        md = threshold(kind, qf, sf, 0.01, rng)
        pq_ids, pq_n_obs, pq_feats = pack_tracks(q_ids, list(qf), D)
    stores = {"f32": BestFitStore(eng, kind, D, K), "f16": F16Store(eng, kind, D, K)}
    prm = sa_topn_params(topn, 1, md, float("inf"))
    out = {s: (np.zeros(n, np.uint32), np.zeros((n, topn), np.uint64), np.zeros((n, topn), np.float64)) for s in STORES}

    def call(s):
        st = stores[s]
        o = (_p(out[s][0], C.c_uint32), _p(out[s][1], C.c_uint64), _p(out[s][2], C.c_double), None)
        if join:
            st._chk(st.lib.sa_store_join_topn(st.h, C.byref(prm), *o))
        else:
            st._chk(st.lib.sa_store_search_topn(st.h, C.byref(prm), Q, _p(pq_ids, C.c_uint64), _p(pq_n_obs, C.c_uint32),
                                                _p(pq_feats, C.c_float), *o))
        return st.last_stats()

    try:
        for st in stores.values():
            for t0 in range(0, T, 1000):   # upsert in slices: the host staging of one call is [n][Kp][D]
                st.upsert(s_ids[t0:t0 + 1000], list(sf[t0:t0 + 1000]))
        for s in STORES:                   # warm-up: buffers, the pool's growth
            call(s)
        t = {s: {"launch1_us": [], "launch2_us": [], "call_us": []} for s in STORES}
        groups, expand = {}, {"cells": 0, "tiles": 0}
        for _ in range(rounds):
            for s in STORES:
                ls = call(s)
                t[s]["launch1_us"].append(ls["launch1_ms"] * 1e3)
                t[s]["launch2_us"].append(ls["launch2_ms"] * 1e3)
                t[s]["call_us"].append(ls["call_ms"] * 1e3)
                groups[s] = ls["groups"]
                if s == "f16":
                    expand = stores[s].expand_stats()
        info = {s: store_info(stores[s]) for s in STORES}
        # the cost: the cells of a sample of queries through the tap of either store
        if join:
            cells = {s: stores[s].search_stored_raw(s_ids[:sample], topn, md, tap=True)[3] for s in STORES}
        else:
            cells = {s: stores[s].search_raw(q_ids[:sample], list(qf[:sample]), topn, md, tap=True)[3] for s in STORES}
    finally:
        for st in stores.values():
            st.close()
    a, b = cells["f32"], cells["f16"]
    both = ~np.isnan(a) & ~np.isnan(b)
    differ = sum(1 for i in range(n) if out["f32"][0][i] != out["f16"][0][i]
                 or not np.array_equal(out["f32"][1][i, : out["f32"][0][i]], out["f16"][1][i, : out["f16"][0][i]]))
    line = {"config": name, "kind": kind, "queries": n, "tracks": T, "observations": K, "D": D, "topn": topn,
            "max_distance": round(md, 6), "rounds": rounds}
    for s in STORES:
        d = {k: pct(v) for k, v in t[s].items()}
        d["groups"] = groups[s]
        d["feature_bytes"] = info[s]["feature_bytes"]
        line[s] = d
    for k in ("launch1", "launch2", "call"):
        line[k + "_gain"] = round(line["f32"][k + "_us"]["median"] / max(line["f16"][k + "_us"]["median"], 1e-9), 3)
    line["launch1_beyond_spread"] = beyond_spread(line["f32"]["launch1_us"], line["f16"]["launch1_us"])
    line["call_beyond_spread"] = beyond_spread(line["f32"]["call_us"], line["f16"]["call_us"])
    line["launch1_p90_below_f32_p10"] = bool(line["f16"]["launch1_us"]["p90"] < line["f32"]["launch1_us"]["p10"])
    line["feature_bytes_ratio"] = round(info["f16"]["feature_bytes"] / info["f32"]["feature_bytes"], 4)
    rows_q, rows_s = n * info["f16"]["Kp"], T * info["f16"]["Kp"]
    tr, tc = -(-rows_q // 64), -(-rows_s // 64)
    tiles = tr * (tr + 1) // 2 if join else tr * tc
    cells_run = tiles * 4096
    line["expand"] = {"cells": expand["cells"], "tiles": expand["tiles"], "tiles_run": tiles,
                      "flagged_share": round(expand["cells"] / cells_run, 6), "tile_share": round(expand["tiles"] / tiles, 6)}
    line["queries_differing"] = int(differ)
    line["cells_sampled"] = int(both.sum())
    line["same_nan_pattern"] = bool(np.array_equal(np.isnan(a), np.isnan(b)))
    move = np.abs(a[both].astype(np.float64) - b[both])
    if kind != "cosine":
        move = move / np.maximum(np.abs(a[both].astype(np.float64)), 1e-30)
    line["max_cell_move"] = float(move.max()) if both.any() else None
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes only (2000 x 8 against 16 x 8, a join of 512 x 4; 128-d)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "f16_store.jsonl"))
    args = ap.parse_args()
    sizes = [("reid", 2000, 8, 128, 16, 2), ("join", 512, 4, 128, 0, 8)] if args.quick else [("reid", 20000, 32, 512, 64, 2), ("join", 4096, 8, 512, 0, 8)]
    eng = Engine(abi.make_config(device=0))
    try:
        with open(args.out, "w") as fh:
            for name, T, K, D, Q, sample in sizes:
                for kind in ("cosine", "euclidean"):
                    line = run(eng, name, kind, T, K, D, Q, 10, max(1, args.rounds), np.random.default_rng(0), sample)
                    text = json.dumps(line)
                    print(text, flush=True)
                    fh.write(text + "\n")
                    fh.flush()
    finally:
        eng.close()


if __name__ == "__main__":
    main()
