"""Tracks that leave an engine's table and enter a feature store in one call (include/similari_waste.h) against the only route the
calls before it offer — sa_tracks_get_state per id, the compaction on the host, sa_store_append or sa_store_absorb_keep,
sa_tracks_remove — on twin engines and twin stores fed the same seeded tables, in one process, one JSON line per configuration.  The
size is examples/track_merging.rs's: N tracks of K observations leave for a gallery of T tracks; in the absorb about half of them
are built on a gallery track and join it.

  waste          engine A / store A take every round through sa_tracks_waste, engine B / store B through the host route; the routes
                 alternate, `rounds` rounds after a warm-up
  waste_absorb   the same with sa_tracks_waste_absorb against sa_store_absorb_keep

Times are HOST-clock microseconds around the Python wrappers of the synchronous C calls, median [p10, p90]; for the host route the
sum of its calls with their split (the compaction in numpy is inside "get_state").  capture_us is k_waste_capture alone, from DEVICE
events around its launches, with the bytes it moves (every present row read and written once, the flags, qualities and tables) and
the rate they make; body_device_us is the append's (sa_merge_stats.device_ms) or the absorb step's (step_ms) own device time.  Every
round asserts that both routes returned the same bits and left the same stores and tables.

   python scripts/bench_waste.py [--quick] [--rounds N] [--out profiles/waste.jsonl]"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from similari_amd import abi, waste as W  # noqa: E402
from similari_amd.engine import Engine  # noqa: E402
from similari_amd.retain import RetainStore  # noqa: E402

u8, u32, u64, f32 = np.uint8, np.uint32, np.uint64, np.float32
P = C.POINTER
STAY = 8   # tracks of the scene that do not leave


def pct(v):
    v = np.asarray(v, np.float64) * 1e6
    return {"median": round(float(np.median(v)), 1), "p10": round(float(np.quantile(v, 0.1)), 1), "p90": round(float(np.quantile(v, 0.9)), 1)}


def clock(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def same_bits(a, b):
    return all((x is None) == (y is None) and (x is None or np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes())
               for x, y in zip(a, b))


def fill(eng, scene, ids, present, feats, quality):
    """sa_tracks_upsert with feat_present, then the qualities (and a filter state) through sa_tracks_set_state."""
    n = len(ids)
    boxes = abi.make_boxes(100.0 + 150.0 * (np.arange(n) % 40), 100.0 + 150.0 * (np.arange(n) // 40), np.full(n, 0.5), np.full(n, 80.0))
    eng.upsert(scene, abi.make_tracks(ids, boxes, np.full(n, 1, u64), feats=feats, feat_present=present))
    fp = P(C.c_float)
    mean, cov = np.zeros(10, f32), np.zeros(100, f32)
    for i, t in enumerate(ids):
        q = np.ascontiguousarray(quality[i], f32)
        eng._chk(eng.lib.sa_tracks_set_state(eng.h, scene, int(t), mean.ctypes.data_as(fp), cov.ctypes.data_as(fp), q.ctypes.data_as(fp)))


def get_states(eng, scene, ids, K, D):
    """The host route's first step: sa_tracks_get_state per id and the compaction of the present slots."""
    fp = P(C.c_float)
    q, pres, feats = np.zeros(K, f32), np.zeros(K, u8), np.zeros((K, D), f32)
    rows, quality = [], []
    for t in ids:
        eng._chk(eng.lib.sa_tracks_get_state(eng.h, scene, int(t), None, None, q.ctypes.data_as(fp), pres.ctypes.data_as(P(C.c_uint8)), feats.ctypes.data_as(fp)))
        keep = pres != 0
        rows.append(feats[keep].copy())
        quality.append(q[keep].copy())
    return rows, quality


def config(mode, ea, eb, N, K, D, T, rounds, warm=2):
    rng = np.random.default_rng(N + T + len(mode))
    cut, scene = -0.9, 0
    sa, sb = (RetainStore(e, "cosine", D, K) for e in (ea, eb))
    wall = {"one_call": [], "host_route": []}
    parts = {"get_state": [], "store_call": [], "remove": []}
    dev = {"capture": [], "body": []}
    Dp = (D + 31) // 32 * 32
    try:
        g_ids = np.arange(1, T + 1, dtype=u64)
        g_banks = [rng.uniform(-1, 1, (int(m), D)).astype(f32) for m in rng.integers(1, K + 1, T)]
        g_quality = [rng.uniform(0, 1, len(x)).astype(f32) for x in g_banks]
        for s in (sa, sb):
            s.append(g_ids, g_banks, g_quality, "latest")
        next_id, stats = 10 * T, None
        for r in range(warm + rounds):
            ids = np.arange(next_id, next_id + N + STAY, dtype=u64)
            next_id += N + STAY
            present = (rng.uniform(0, 1, (N + STAY, K)) < 0.85).astype(u8)
            present[:, K - 1] |= (present.sum(1) == 0).astype(u8)   # (the benchmark's tracks all bring a row)
            feats = rng.uniform(-1, 1, (N + STAY, K, D)).astype(f32)
            if mode == "waste_absorb":   # half of the leaving tracks are built on a gallery track, each named once
                named = rng.permutation(T)[: N // 2]
                for i in range(N // 2):
                    feats[i] = -g_banks[int(named[i])][0][None, :] + rng.normal(0, 1e-3, (K, D))
            feats = (feats * present[:, :, None]).astype(f32)
            quality = rng.uniform(0.05, 1, (N + STAY, K)).astype(f32)
            for e in (ea, eb):
                fill(e, scene, ids, present, feats, quality)
            gone = ids[:N]

            def one_call():
                if mode == "waste":
                    t, out = clock(lambda: W.waste_raw(ea, sa, {scene: gone}, "best"))
                    return t, (out[1],), None
                t, out = clock(lambda: W.waste_absorb_raw(ea, sa, {scene: gone}, 1, cut, "best"))
                return t, out[1], None

            def host_route():
                t0, (rows, q) = clock(lambda: get_states(eb, scene, gone, K, D))
                if mode == "waste":
                    t1, _ = clock(lambda: sb.append(gone, rows, q, "best"))
                    out = (np.array([len(x) for x in rows], u32),)
                else:
                    t1, out = clock(lambda: sb.absorb_keep_raw(gone, rows, 1, cut, "best", quality=q))
                t2, _ = clock(lambda: eb.remove(scene, gone))
                return t0 + t1 + t2, out, (t0, t1, t2)

            order = [("one_call", one_call), ("host_route", host_route)]
            res = {}
            for k, fn in (order if r % 2 == 0 else order[::-1]):   # the routes alternate
                t, out, split = fn()
                res[k] = out
                if r >= warm:
                    wall[k].append(t)
                    if split:
                        for name, x in zip(parts, split):
                            parts[name].append(x)
            stats = W.last(sa)
            if r >= warm:
                dev["capture"].append(stats["capture_ms"] * 1e-3)
                dev["body"].append((sa.merge_stats()["device_ms"] if mode == "waste" else sa.retain_stats()["step_ms"]) * 1e-3)
            assert same_bits(res["one_call"], res["host_route"]), "round %d: the two routes returned different bits" % r
            assert np.array_equal(sa.order(), sb.order()), "round %d: the stores hold different tracks" % r
            look = np.concatenate([sa.order()[:: max(1, len(sa) // 256)], sa.order()[-N:]])
            assert same_bits(sa.fetch_raw(look), sb.fetch_raw(look)), "round %d: the stores hold different rows" % r
            assert np.array_equal(ea.order(scene), eb.order(scene)) and ea.count(scene) == STAY, "round %d: the tables differ" % r
            assert stats["feature_bytes_h2d"] == 0 and stats["feature_bytes_d2h"] == 0 and stats["launches_capture"] == 1 and stats["tracks"] == N
            for e in (ea, eb):
                e.remove(scene, e.order(scene))
        out = {k: {"wall_us": pct(v)} for k, v in wall.items()}
        out["host_route"]["parts_us"] = {k: pct(v)["median"] for k, v in parts.items()}
        Kp = 1 << (K - 1).bit_length()
        moved = int(stats["rows"]) * Dp * 4 * 2 + N * (4 + K * 5 + 4 + Kp * 8)   # rows in and out; the row index, flags and qualities in; count, qualities and table out
        cap = pct(dev["capture"])
        out["capture_us"] = cap
        out["capture_bytes"] = moved
        out["capture_GBps"] = round(moved / (cap["median"] * 1e-6) / 1e9, 1) if cap["median"] else None
        out["body_device_us"] = pct(dev["body"])["median"]
        out["waste_stats"] = {k: v for k, v in stats.items() if not k.endswith("_ms")}
        out["p90_below_p10"] = out["one_call"]["wall_us"]["p90"] < out["host_route"]["wall_us"]["p10"]
        out["wall_gain"] = round(out["host_route"]["wall_us"]["median"] / out["one_call"]["wall_us"]["median"], 3)
    finally:
        for s in (sa, sb):
            s.close()
    return {"config": mode, "leaving": N, "observations": K, "D": D, "gallery": T, "kind": "cosine", "store": "f32", "keep": "best",
            "rounds": rounds, "clock": "host (wall_us, parts_us), device events (capture_us, body_device_us)", "same_bits": True, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes (50 leaving tracks against a gallery of 500, 64-d)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "waste.jsonl"))
    args = ap.parse_args()
    rounds = max(1, args.rounds)
    q = args.quick
    N, K, D, T = (50, 3, 64, 500) if q else (500, 3, 256, 5000)
    ea, eb = (Engine(abi.make_config(device=0, visual="cosine", feature_len=D, max_observations=K)) for _ in range(2))
    try:
        with open(args.out, "w") as fh:
            for mode in ("waste", "waste_absorb"):
                text = json.dumps(config(mode, ea, eb, N, K, D, T, rounds))
                print(text, flush=True)
                fh.write(text + "\n")
                fh.flush()
    finally:
        ea.close()
        eb.close()


if __name__ == "__main__":
    main()
