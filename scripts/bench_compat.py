"""What the attribute gates of include/similari_attrs.h cost and save in a whole-gallery join: the seeded galleries of
scripts/bench_gallery.py (4096 x 8 and 8192 x 4, 512-d, both kinds), every track with one of 16 keys (cameras) and a time span, in
two arrangements of the same tracks:

  clustered   inserted key by key, in time order inside a key: pairs of different keys fill whole tiles, which leave before their main loop
  shuffled    inserted in random order: hardly a tile without a live group

Three joins alternate in one process on each store, after one warm-up round (which also grows the pool):

  (a) compat   sa_store_join_topn_compat under SA_COMPAT_SAME_KEY | SA_COMPAT_DISJOINT
  (b) plain    sa_store_join_topn: the only way without the header — and not the same answer (M is taken over dead pairs too)
  (c) flags0   sa_store_join_topn_compat with flags 0: the bits of (b) through the gated kernel — what the gate costs when it gates nothing

One JSON line per (kind, size, arrangement), appended to --out: per form median / 10th / 90th percentile of launch 1, launch 2 and
the whole call (device events, microseconds); `tiles_skipped / tiles` of (a); `plain_over_compat` = (b) / (a) and `flags0_over_plain`
= (c) / (b) on launch 1 medians, each with whether the gap of the medians exceeds the 10th-90th spread of both sides;
`flags0_same_bits`: (c) returned out_n, winners and weight bits of (b).
   python scripts/bench_compat.py [--quick] [--reps N] [--out FILE]"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
from bench_gallery import pair_threshold, pct  # noqa: E402
from similari_amd import abi, attrs as A, synth  # noqa: E402
from similari_amd.attrs import AttrStore  # noqa: E402
from similari_amd.engine import Engine  # noqa: E402
from similari_amd.search import _p, sa_topn_params  # noqa: E402

f32 = np.float32
FORMS = ("compat", "plain", "flags0")
KEYS = 16


def gap_beyond_spread(x, y):
    return bool(abs(x["median"] - y["median"]) > max(x["p90"] - x["p10"], y["p90"] - y["p10"]))


def run(eng, kind, T, K, D, topn, reps, arrangement, out_path):
    rng = np.random.default_rng(0)   # the same tracks in both arrangements
    ident = synth.reid_identities(rng, T, D)
    sf = np.empty((T, K, D), f32)
    for k in range(K):
        sf[:, k] = synth.observe(rng, ident, 0.05)
    md = pair_threshold(kind, sf, 0.01, rng)
    key = rng.integers(1, KEYS + 1, T)
    start = rng.integers(0, 100000, T)
    end = start + rng.integers(1, 2000, T)
    perm = np.lexsort((start, key)) if arrangement == "clustered" else rng.permutation(T)
    sf, key, start, end = sf[perm], key[perm], start[perm], end[perm]
    ids = np.arange(1, T + 1, dtype=np.uint64)
    store = AttrStore(eng, kind, D, K)
    lib, h = store.lib, store.h
    prm = sa_topn_params(topn, 1, md, float("inf"))
    rules = {"compat": A.compat(same_key=True, disjoint=True).struct(), "flags0": A.compat().struct()}
    out = {f: (np.zeros(T, np.uint32), np.zeros((T, topn), np.uint64), np.zeros((T, topn), np.float64)) for f in FORMS}

    def call(form):
        n, w, x = out[form]
        o = (_p(n, C.c_uint32), _p(w, C.c_uint64), _p(x, C.c_double), None)
        if form == "plain":
            store._chk(lib.sa_store_join_topn(h, C.byref(prm), *o))
        else:
            store._chk(lib.sa_store_join_topn_compat(h, C.byref(prm), C.byref(rules[form]), *o))

    try:
        for t0 in range(0, T, 1000):
            store.upsert(ids[t0:t0 + 1000], list(sf[t0:t0 + 1000]))
        store.set_attrs(ids, key, start, end)
        for f in FORMS:
            call(f)
        t = {f: {"launch1_us": [], "launch2_us": [], "call_us": []} for f in FORMS}
        groups, tiles = {}, {}
        for _ in range(reps):
            for f in FORMS:
                call(f)
                st = store.last_stats()
                t[f]["launch1_us"].append(st["launch1_ms"] * 1e3)
                t[f]["launch2_us"].append(st["launch2_ms"] * 1e3)
                t[f]["call_us"].append(st["call_ms"] * 1e3)
                groups[f] = st["groups"]
                if f != "plain":
                    tiles[f] = store.compat_stats()
    finally:
        store.close()
    same = all(np.array_equal(out["plain"][i].view(np.uint64 if i else np.uint32), out["flags0"][i].view(np.uint64 if i else np.uint32))
               for i in range(3))
    line = {"config": "compat_join", "kind": kind, "tracks": T, "observations": K, "D": D, "topn": topn, "max_distance": round(md, 6),
            "keys": KEYS, "arrangement": arrangement, "reps": reps, "tiles": tiles["compat"]["tiles"],
            "tiles_skipped": tiles["compat"]["tiles_skipped"],
            "tiles_skipped_share": round(tiles["compat"]["tiles_skipped"] / tiles["compat"]["tiles"], 4),
            "flags0_tiles_skipped": tiles["flags0"]["tiles_skipped"], "flags0_same_bits": bool(same)}
    for f in FORMS:
        s = {k: pct(v) for k, v in t[f].items()}
        s["groups"] = groups[f]
        line[f] = s
    a, b, c = (line[f]["launch1_us"] for f in FORMS)
    line["plain_over_compat"] = round(b["median"] / a["median"], 3)
    line["plain_over_compat_beyond_spread"] = gap_beyond_spread(b, a)
    line["flags0_over_plain"] = round(c["median"] / b["median"], 3)
    line["flags0_over_plain_beyond_spread"] = gap_beyond_spread(c, b)
    line["call_plain_over_compat"] = round(line["plain"]["call_us"]["median"] / line["compat"]["call_us"]["median"], 3)
    text = json.dumps(line)
    print(text, flush=True)
    with open(out_path, "a") as fh:
        fh.write(text + "\n")
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a small gallery only (512 tracks x 4 x 128-d)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "compat_search.jsonl"))
    args = ap.parse_args()
    reps = max(5, args.reps)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    eng = Engine(abi.make_config(device=0))
    ok = True
    try:
        for kind in ("cosine", "euclidean"):
            for T, K, D in ([(512, 4, 128)] if args.quick else [(4096, 8, 512), (8192, 4, 512)]):
                for arrangement in ("clustered", "shuffled"):
                    ok &= run(eng, kind, T, K, D, 10, reps, arrangement, args.out)
    finally:
        eng.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
