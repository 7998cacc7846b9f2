"""Merge timing on a seeded gallery (include/similari_merge.h): tracklets in pairs of one identity (cosine: of antipodal ones, the
pair the voting ranks first) are joined, every track whose top winner names it back is merged with that winner, two ways in one
process, one JSON line per configuration:

  (a) device   MergeStore.merge: ids only cross the bus, the rows move on the device (SA_KEEP_LATEST, capacity K)
  (b) host     the only way without similari_merge.h: the merged banks are built from a host mirror of every feature, written
               with sa_store_upsert(dst) and the absorbed tracks taken out with sa_store_remove(src)

A merge consumes the store, so it is rebuilt (untimed) before every timed call; the forms alternate, after one warm-up round.  Per
form: median / 10th / 90th percentile of the wall time of the calls (microseconds; (b) includes building the banks on the host, its
arguments packed inside the clock as a caller must).  For (a) also what sa_store_merge_last reports: device time (events), rows
rewritten, tracks moved, launches, and bytes_moved / device time beside the 6.29 TB/s a float4 copy measures on this part.
`host_over_device`: (b) over (a), wall medians; `beyond_spread`: the gap of the medians exceeds the 10th-90th spread of either side.
`same_store_bits`: after the last round both stores hold the same order, counts and rows.
   python scripts/bench_merge.py [--quick] [--reps N]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from similari_amd import abi, synth  # noqa: E402
from similari_amd.engine import Engine  # noqa: E402
from similari_amd.merge import MergeStore  # noqa: E402

COPY_RATE = 6.29e12
f32 = np.float32


def pct(v):
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), 1), "p10": round(float(np.quantile(v, 0.1)), 1), "p90": round(float(np.quantile(v, 0.9)), 1)}


def beyond_spread(slow, fast):
    gap = slow["median"] - fast["median"]
    return bool(gap > max(slow["p90"] - slow["p10"], fast["p90"] - fast["p10"]))


def build(eng, kind, ids, sf):
    store = MergeStore(eng, kind, sf.shape[2], sf.shape[1])
    for t0 in range(0, len(ids), 1000):   # upsert in slices: the host staging of one call is [n][Kp][D]
        store.upsert(ids[t0:t0 + 1000], list(sf[t0:t0 + 1000]))
    return store


def run(eng, kind, T, K, D, reps, rng):
    ident = np.repeat(synth.reid_identities(rng, T // 2, D), 2, axis=0)
    if kind == "cosine":
        ident[1::2] *= -1   # the voting ranks by smallest value and cosine is a similarity: a tracklet's partner is its antipode
    sf = np.empty((T, K, D), f32)
    for k in range(K):
        sf[:, k] = synth.observe(rng, ident, 0.05)
    ids = np.arange(1, T + 1, dtype=np.uint64)
    mirror = {int(i): sf[k] for k, i in enumerate(ids)}

    store = build(eng, kind, ids, sf)
    try:
        t = time.perf_counter()
        win = {q: lst[0][0] for q, lst in store.join_topn(1, float("inf")).items()}
        join_ms = (time.perf_counter() - t) * 1e3
    finally:
        store.close()
    pairs = {a: [b] for a, b in win.items() if a < b and win.get(b) == a}

    def device(store):
        t = time.perf_counter()
        store.merge(pairs, keep="latest")
        return time.perf_counter() - t

    def host(store):
        t = time.perf_counter()
        dst = list(pairs)
        banks = [np.concatenate([mirror[d]] + [mirror[s] for s in pairs[d]])[-K:] for d in dst]
        store.upsert(dst, banks)
        store.remove([s for d in dst for s in pairs[d]])
        return time.perf_counter() - t

    times = {"device": [], "host": []}
    dev_us, stats, same = [], {}, True
    for rnd in range(reps + 1):   # round 0 warms up
        a, b = build(eng, kind, ids, sf), build(eng, kind, ids, sf)
        try:
            wa = device(a)
            st = a.merge_stats()
            wb = host(b)
            if rnd:
                times["device"].append(wa * 1e6)
                times["host"].append(wb * 1e6)
                dev_us.append(st["device_ms"] * 1e3)
                stats = st
            if rnd == reps:
                order = a.order()
                same = np.array_equal(order, b.order())
                for t0 in range(0, len(order), 1000):
                    fa, fb = a.fetch_raw(order[t0:t0 + 1000]), b.fetch_raw(order[t0:t0 + 1000])
                    same = same and np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1].view(np.uint32), fb[1].view(np.uint32))
        finally:
            a.close()
            b.close()
    line = {"config": "store_merge", "kind": kind, "tracks": T, "observations": K, "D": D, "reps": reps, "merged_pairs": len(pairs),
            "join_wall_ms": round(join_ms, 2), "same_store_bits": bool(same), "device": {"wall_us": pct(times["device"]), "device_us": pct(dev_us)},
            "host": {"wall_us": pct(times["host"])}}
    line["device"].update({k: stats[k] for k in ("rows_rewritten", "tracks_moved", "launches", "bytes_moved")})
    med = line["device"]["device_us"]["median"]
    line["device"]["moved_TBps"] = round(stats["bytes_moved"] / (med * 1e-6) / 1e12, 3) if med else None
    line["device"]["share_of_copy_rate"] = round(stats["bytes_moved"] / (med * 1e-6) / COPY_RATE, 3) if med else None
    line["host_over_device"] = round(line["host"]["wall_us"]["median"] / line["device"]["wall_us"]["median"], 2)
    line["beyond_spread"] = beyond_spread(line["host"]["wall_us"], line["device"]["wall_us"])
    print(json.dumps(line), flush=True)
    return same and len(pairs) > 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a small gallery only (512 tracks x 4 x 128-d)")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    eng = Engine(abi.make_config(device=0))
    ok = True
    try:
        for kind in ("cosine", "euclidean"):
            for T, K, D in ([(512, 4, 128)] if args.quick else [(4096, 8, 512), (8192, 4, 512)]):
                ok &= run(eng, kind, T, K, D, max(1, args.reps), np.random.default_rng(0))
    finally:
        eng.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
