"""An i8 feature store against a bf16 and an f32 store (include/similari_i8.h): the same seeded features in all three, in one process,
one JSON line per size:

  reid   the re-identification size of DESIGN section 10: 64 queries x 32 observations against 20 000 tracks x 32, 512-d, about 1 %
         of the groups surviving (host-fed queries, sa_store_search_topn)
  join   the whole-gallery join at 4096 tracks x 8, 512-d, about 1 % of the pairs surviving (sa_store_join_topn)

Calls on the three stores alternate, after one warm-up round (which also grows the pools).  Per store: median / 10th / 90th
percentile of launch 1, launch 2 and the whole call from the store's own device events (sa_search_stats, microseconds), and
feature_bytes (sa_store_get_info).  `launch1_gain_over_f32` / `_over_bf16`, `call_gain_over_*`: that store's median over the i8 store's;
`*_beyond_spread`: the gap of the medians exceeds the 10th-90th spread of either side (false also when the i8 store is the slower
one).  What int8 costs stands beside what it buys: `queries_differing` — how many queries' winner lists (ids, in order) differ from
the f32 store's, for the bf16 and for the i8 store — and `max_cell_move`, the largest |cell - f32 cell| over the tapped cells of a
sample of queries.
   python scripts/bench_i8.py [--quick] [--rounds N] [--out profiles/i8_store.jsonl]"""
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
from similari_amd.bf16 import Bf16Store, store_info  # noqa: E402
from similari_amd.engine import Engine  # noqa: E402
from similari_amd.i8 import I8Store  # noqa: E402
from similari_amd.search import _p, pack_tracks, sa_topn_params  # noqa: E402

f32 = np.float32
STORES = ("f32", "bf16", "i8")


def host_cosine(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return (a @ b.T) / np.sqrt((a * a).sum(1)[:, None] * (b * b).sum(1)[None, :])


def threshold(qf, sf, frac, rng, own=False):
    """max_distance that keeps about `frac` of the (query, track) groups — one kept cell makes a group — from a sample of tracks
    (own: the queries are those tracks themselves, the self pairs stay out)."""
    t = rng.choice(sf.shape[0], min(400, sf.shape[0]), replace=False)
    q = sf[t] if own else qf
    d = host_cosine(q.reshape(-1, q.shape[2]), sf[t].reshape(-1, sf.shape[2])).reshape(q.shape[0], q.shape[1], len(t), sf.shape[1])
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
    return ident, sf


def run(eng, name, T, K, D, Q, topn, rounds, rng, sample):
    ident, sf = features(rng, T, K, D)
    s_ids = np.arange(1, T + 1, dtype=np.uint64)
    join = Q == 0
    if join:
        qf, q_ids, n = None, s_ids, T
        md = threshold(None, sf, 0.01, rng, own=True)
    else:
        pick = rng.choice(T, Q, replace=False)
        qf = np.stack([synth.observe(rng, ident[pick], 0.05) for _ in range(K)], axis=1)
        q_ids, n = np.arange(T + 1, T + Q + 1, dtype=np.uint64), Q
        md = threshold(qf, sf, 0.01, rng)
        pq_ids, pq_n_obs, pq_feats = pack_tracks(q_ids, list(qf), D)
    stores = {"f32": BestFitStore(eng, "cosine", D, K), "bf16": Bf16Store(eng, "cosine", D, K), "i8": I8Store(eng, "cosine", D, K)}
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
        groups = {}
        for _ in range(rounds):
            for s in STORES:
                ls = call(s)
                t[s]["launch1_us"].append(ls["launch1_ms"] * 1e3)
                t[s]["launch2_us"].append(ls["launch2_ms"] * 1e3)
                t[s]["call_us"].append(ls["call_ms"] * 1e3)
                groups[s] = ls["groups"]
        info = {s: store_info(stores[s]) for s in STORES}
        # the cost: the cells of a sample of queries through the tap of either store
        if join:
            cells = {s: stores[s].search_stored_raw(s_ids[:sample], topn, md, tap=True)[3] for s in STORES}
        else:
            cells = {s: stores[s].search_raw(q_ids[:sample], list(qf[:sample]), topn, md, tap=True)[3] for s in STORES}
    finally:
        for st in stores.values():
            st.close()
    def differing(s):
        return sum(1 for i in range(n) if out["f32"][0][i] != out[s][0][i]
                   or not np.array_equal(out["f32"][1][i, : out["f32"][0][i]], out[s][1][i, : out[s][0][i]]))

    line = {"config": name, "kind": "cosine", "queries": n, "tracks": T, "observations": K, "D": D, "topn": topn,
            "max_distance": round(md, 6), "rounds": rounds}
    for s in STORES:
        d = {k: pct(v) for k, v in t[s].items()}
        d["groups"] = groups[s]
        d["feature_bytes"] = info[s]["feature_bytes"]
        line[s] = d
    a = cells["f32"]
    for s in ("bf16", "i8"):
        b = cells[s]
        both = ~np.isnan(a) & ~np.isnan(b)
        line[s]["feature_bytes_ratio"] = round(info[s]["feature_bytes"] / info["f32"]["feature_bytes"], 4)
        line[s]["queries_differing"] = int(differing(s))
        line[s]["cells_sampled"] = int(both.sum())
        line[s]["same_nan_pattern"] = bool(np.array_equal(np.isnan(a), np.isnan(b)))
        line[s]["max_cell_move"] = float(np.abs(a[both].astype(np.float64) - b[both]).max()) if both.any() else None
    for other in ("f32", "bf16"):   # the i8 store against each of the others, in this run
        for k in ("launch1", "call"):
            line["%s_gain_over_%s" % (k, other)] = round(line[other][k + "_us"]["median"] / max(line["i8"][k + "_us"]["median"], 1e-9), 3)
            line["%s_beyond_spread_over_%s" % (k, other)] = beyond_spread(line[other][k + "_us"], line["i8"][k + "_us"])
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes only (2000 x 8 against 16 x 8, a join of 512 x 4; 128-d)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "i8_store.jsonl"))
    args = ap.parse_args()
    sizes = [("reid", 2000, 8, 128, 16, 2), ("join", 512, 4, 128, 0, 8)] if args.quick else [("reid", 20000, 32, 512, 64, 2), ("join", 4096, 8, 512, 0, 8)]
    eng = Engine(abi.make_config(device=0))
    try:
        with open(args.out, "w") as fh:
            for name, T, K, D, Q, sample in sizes:
                line = run(eng, name, T, K, D, Q, 10, max(1, args.rounds), np.random.default_rng(0), sample)
                text = json.dumps(line)
                print(text, flush=True)
                fh.write(text + "\n")
                fh.flush()
    finally:
        eng.close()


if __name__ == "__main__":
    main()
