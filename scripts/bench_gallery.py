"""Whole-gallery search timing (include/similari_gallery.h): every stored track searched against every other one, three ways on
the same seeded store in one process, one JSON line per configuration:

  (a) join      Gallery.join_raw: the store against itself, tiles on or above the diagonal only, one pool block per unordered pair
  (b) stored    Gallery.search_stored_raw over all ids: the queries gathered on the device, the rectangular grid
  (c) foreign   sa_store_search_topn with the whole gallery handed over as host queries (the only way without similari_gallery.h)

The forms alternate, after one warm-up round (which also grows the pool).  Per form: median / 10th / 90th percentile of launch 1,
launch 2 and the whole call (device events, microseconds), of the C call's wall time (transfers and host staging included; the
arguments are packed before the clock starts), launch 1's share of the 157.3 TF/s f32 MFMA peak counting the FLOPs of the tiles
it actually ran (2 BM BN Dp each), and tiles / tiles_rect.  `same_winner_bits`: (a), (b) and (c) returned identical out_n, winners and
weights (u64 views; the cells are not tapped while timing).  `launch1_gain` / `wall_gain`: (c) over (a) for launch 1, (c) over (b) for wall time, medians;
`*_beyond_spread`: the gap of the medians exceeds the 10th-90th spread of either side.
   python scripts/bench_gallery.py [--quick] [--reps N]"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from similari_amd import abi, synth  # noqa: E402
from similari_amd.engine import Engine  # noqa: E402
from similari_amd.gallery import Gallery  # noqa: E402
from similari_amd.search import _p, pack_tracks, sa_topn_params  # noqa: E402

PEAK_F32_MFMA = 157.3e12
f32 = np.float32
FORMS = ("join", "stored", "foreign")


def host_distances(kind, a, b):
    a = a.astype(np.float64)
    b = b.astype(np.float64)
    dot = a @ b.T
    na, nb = (a * a).sum(1), (b * b).sum(1)
    if kind == "cosine":
        return dot / np.sqrt(na[:, None] * nb[None, :])
    return np.sqrt(np.maximum(na[:, None] + nb[None, :] - 2.0 * dot, 0.0))


def pair_threshold(kind, sf, frac, rng, sample=400):
    """max_distance that lets about `frac` of the track pairs survive (one kept cell makes a group), from a sample of tracks."""
    T, K, D = sf.shape
    t = rng.choice(T, min(sample, T), replace=False)
    d = host_distances(kind, sf[t].reshape(-1, D), sf[t].reshape(-1, D)).reshape(len(t), K, len(t), K)
    best = d.min(axis=(1, 3))[~np.eye(len(t), dtype=bool)]
    return float(np.quantile(best, frac))


def pct(v):
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), 1), "p10": round(float(np.quantile(v, 0.1)), 1), "p90": round(float(np.quantile(v, 0.9)), 1)}


def beyond_spread(slow, fast):
    gap = slow["median"] - fast["median"]
    return bool(gap > max(slow["p90"] - slow["p10"], fast["p90"] - fast["p10"]))


def run(eng, kind, T, K, D, topn, reps, rng):
    ident = synth.reid_identities(rng, T, D)
    sf = np.empty((T, K, D), f32)
    for k in range(K):
        sf[:, k] = synth.observe(rng, ident, 0.05)
    ids = np.arange(1, T + 1, dtype=np.uint64)
    md = pair_threshold(kind, sf, 0.01, rng)
    store = Gallery(eng, kind, D, K)
    lib, h = store.lib, store.h
    prm = sa_topn_params(topn, 1, md, float("inf"))
    q_ids, q_n_obs, q_feats = pack_tracks(ids, list(sf), D)
    out = {f: (np.zeros(T, np.uint32), np.zeros((T, topn), np.uint64), np.zeros((T, topn), np.float64)) for f in FORMS}

    def call(form):
        n, w, x = out[form]
        o = (_p(n, C.c_uint32), _p(w, C.c_uint64), _p(x, C.c_double), None)
        t = time.perf_counter()
        if form == "join":
            rc = lib.sa_store_join_topn(h, C.byref(prm), *o)
        elif form == "stored":
            rc = lib.sa_store_search_stored(h, C.byref(prm), 0, T, _p(q_ids, C.c_uint64), *o)
        else:
            rc = lib.sa_store_search_topn(h, C.byref(prm), T, _p(q_ids, C.c_uint64), _p(q_n_obs, C.c_uint32), _p(q_feats, C.c_float), *o)
        wall = time.perf_counter() - t
        store._chk(rc)
        return wall

    try:
        for t0 in range(0, T, 1000):   # upsert in slices: the host staging of one call is [n][Kp][D]
            store.upsert(ids[t0:t0 + 1000], list(sf[t0:t0 + 1000]))
        assert np.array_equal(store.order(), ids)
        for f in FORMS:                # warm-up: buffers, the pool's growth
            call(f)
        t = {f: {"launch1_us": [], "launch2_us": [], "call_us": [], "wall_us": []} for f in FORMS}
        groups = {}
        for _ in range(reps):
            for f in FORMS:
                wall = call(f)
                st = store.last_stats()
                t[f]["launch1_us"].append(st["launch1_ms"] * 1e3)
                t[f]["launch2_us"].append(st["launch2_ms"] * 1e3)
                t[f]["call_us"].append(st["call_ms"] * 1e3)
                t[f]["wall_us"].append(wall * 1e6)
                groups[f] = st["groups"]
        js = store.join_stats()
    finally:
        store.close()
    same = all(np.array_equal(out["join"][i].view(np.uint64 if i else np.uint32), out[f][i].view(np.uint64 if i else np.uint32))
               for f in ("stored", "foreign") for i in range(3))
    Dp = (D + 31) // 32 * 32
    bm, bn = (64, 64) if kind == "cosine" else (32, 128)
    line = {"config": "gallery_join", "kind": kind, "tracks": T, "observations": K, "D": D, "topn": topn, "max_distance": round(md, 6),
            "reps": reps, "tiles": js["tiles"], "tiles_rect": js["tiles_rect"], "tiles_over_rect": round(js["tiles"] / js["tiles_rect"], 4),
            "blocks": js["blocks"], "surviving_pair_share": round(js["blocks"] / (T * (T - 1) / 2), 5), "same_winner_bits": bool(same)}
    for f in FORMS:
        s = {k: pct(v) for k, v in t[f].items()}
        tiles = js["tiles"] if f == "join" else js["tiles_rect"]
        s["launch1_share_of_mfma_peak"] = round(2.0 * bm * bn * Dp * tiles / PEAK_F32_MFMA / (s["launch1_us"]["median"] * 1e-6), 3)
        s["groups"] = groups[f]
        line[f] = s
    line["launch1_gain"] = round(line["foreign"]["launch1_us"]["median"] / line["join"]["launch1_us"]["median"], 3)
    line["wall_gain"] = round(line["foreign"]["wall_us"]["median"] / line["stored"]["wall_us"]["median"], 3)
    line["launch1_beyond_spread"] = beyond_spread(line["foreign"]["launch1_us"], line["join"]["launch1_us"])
    line["wall_beyond_spread"] = beyond_spread(line["foreign"]["wall_us"], line["stored"]["wall_us"])
    print(json.dumps(line), flush=True)
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a small gallery only (512 tracks x 4 x 128-d)")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    reps = max(5, args.reps)
    eng = Engine(abi.make_config(device=0))
    ok = True
    try:
        for kind in ("cosine", "euclidean"):
            for T, K, D in ([(512, 4, 128)] if args.quick else [(4096, 8, 512), (8192, 4, 512)]):
                ok &= run(eng, kind, T, K, D, 10, reps, np.random.default_rng(0))
    finally:
        eng.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
