"""Ready tracks handed from a temporary store to a gallery in one call (include/similari_handover.h) against the three-call route it
replaces — sa_store_fetch, sa_store_absorb_keep, sa_store_remove (no rule, so no attributes are read) — on twin pairs of stores fed the same
seeded tracks, in one process, one JSON line per configuration.  The layout is examples/track_merging.rs: N ready tracks of up to K
observations leave a temp store (which keeps a few that are not ready) for a gallery of T tracks; about half of them are built on a
gallery track and join it, the others become tracks.

  hand_over   pair A takes every round through sa_store_hand_over, pair B through the three calls; the routes alternate, `rounds`
              rounds after a warm-up.  Times are HOST-clock microseconds around the Python wrappers of the synchronous C calls, median
              [p10, p90] — for the three-call route the sum of its calls (the absorb's includes packing fetch's rows into the call's
              layout, the copy a C caller makes to drop the unfilled rows), the slicing between them left out.  Every round
              asserts that both routes returned the same bits and left the same stores.
  remove      sa_store_remove of N ids out of N + 8, one launch, against the same call of the parent commit's library (two copies per
              id) when --parent-lib names one: both libraries are loaded into this process, each with an engine of its own, and the
              calls alternate.  Without --parent-lib the parent's figure is "not measured".

   python scripts/bench_handover.py [--quick] [--rounds N] [--parent-lib PATH] [--out profiles/handover.jsonl]"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from similari_amd import abi, handover as H  # noqa: E402
from similari_amd.engine import Engine  # noqa: E402
from similari_amd.f16 import SA_ELEM_F16, SA_ELEM_F32  # noqa: E402
from similari_amd.retain import RetainStore  # noqa: E402
from similari_amd.search import FeatureStore, _p  # noqa: E402

u32, u64, f32 = np.uint32, np.uint64, np.float32
NAME = {SA_ELEM_F32: "f32", SA_ELEM_F16: "f16"}
STAY = 8   # tracks of the temp store that are not ready


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


def hand_over_config(eng, N, K, D, T, src_elem, dst_elem, kind, rounds, warm=2):
    rng = np.random.default_rng(N + T)
    cut = -0.9 if kind == "cosine" else 0.25
    sa, sb = (RetainStore(eng, kind, D, K, src_elem) for _ in range(2))
    da, db = (RetainStore(eng, kind, D, K, dst_elem) for _ in range(2))
    wall = {"hand_over": [], "three_calls": []}
    parts = {"fetch": [], "absorb_keep": [], "remove": []}
    dev = {"fill": [], "compact": []}
    try:
        g_ids = np.arange(1, T + 1, dtype=u64)
        g_banks = [rng.uniform(-1, 1, (int(m), D)).astype(f32) for m in rng.integers(1, K + 1, T)]
        g_quality = [rng.uniform(0, 1, len(x)).astype(f32) for x in g_banks]
        for s in (da, db):
            s.append(g_ids, g_banks, g_quality, "latest")
        first = {int(i): x[0] for i, x in zip(g_ids, g_banks)}
        sign = f32(-1) if kind == "cosine" else f32(1)
        next_id = 10 * T
        stats = None
        for r in range(warm + rounds):
            ids = np.arange(next_id, next_id + N + STAY, dtype=u64)
            next_id += N + STAY
            named = rng.permutation(T)[: N // 2] + 1   # each gallery track is named once
            banks = []
            for i in range(N + STAY):
                m = int(rng.integers(1, K + 1))
                if i < N // 2:
                    banks.append((sign * first[int(named[i])][None, :] + rng.normal(0, 1e-3, (m, D))).astype(f32))
                else:
                    banks.append(rng.uniform(-1, 1, (m, D)).astype(f32))
            quality = [rng.uniform(0, 1, len(x)).astype(f32) for x in banks]
            for s in (sa, sb):
                s.append(ids, banks, quality, "latest")
                s.set_attrs(ids, np.zeros(N + STAY, u64), np.zeros(N + STAY), [0] * N + [10] * STAY)
            ready = np.array(H.ready(sa, 5), u64)
            assert len(ready) == N and H.ready(sb, 5) == [int(i) for i in ready]

            def one_call():
                t, out = clock(lambda: H.hand_over_raw(sa, da, ready, 1, cut, "best"))
                return t, out, None

            def three_calls():
                t0, (n_obs, feats, qual) = clock(lambda: sb.fetch_raw(ready))
                rows = [feats[i, : n_obs[i]] for i in range(N)]
                q = [qual[i, : n_obs[i]] for i in range(N)]
                t1, out = clock(lambda: db.absorb_keep_raw(ready, rows, 1, cut, "best", quality=q))
                t2, _ = clock(lambda: sb.remove(ready))
                return t0 + t1 + t2, out, (t0, t1, t2)

            order = [("hand_over", one_call), ("three_calls", three_calls)]
            res = {}
            for k, fn in (order if r % 2 == 0 else order[::-1]):   # the routes alternate
                t, out, split = fn()
                res[k] = out
                if r >= warm:
                    wall[k].append(t)
                    if split:
                        for name, x in zip(parts, split):
                            parts[name].append(x)
            stats = H.last(da)
            if r >= warm:
                dev["fill"].append(stats["fill_ms"] * 1e-3)
                dev["compact"].append(stats["compact_ms"] * 1e-3)
            assert same_bits(res["hand_over"], res["three_calls"]), "round %d: the two routes returned different bits" % r
            assert np.array_equal(da.order(), db.order()) and np.array_equal(sa.order(), sb.order()), "round %d: the stores hold different tracks" % r
            look = da.order()[:: max(1, len(da) // 256)]
            assert same_bits(da.fetch_raw(look), db.fetch_raw(look)), "round %d: the galleries hold different rows" % r
            assert same_bits(sa.fetch_raw(sa.order()), sb.fetch_raw(sb.order())), "round %d: the temp stores hold different rows" % r
            assert stats["feature_bytes_h2d"] == 0 and stats["feature_bytes_d2h"] == 0 and stats["launches_fill"] == 1
            matched = da.retain_stats()["matched"]
            for s in (sa, sb):   # what was not ready leaves too: every round starts with an empty temp store
                s.remove(s.order())
        out = {k: {"wall_us": pct(v)} for k, v in wall.items()}
        out["three_calls"]["parts_us"] = {k: pct(v)["median"] for k, v in parts.items()}
        out["fill_us"], out["compact_us"] = pct(dev["fill"])["median"], pct(dev["compact"])["median"]
        out["handover_stats"] = {k: v for k, v in stats.items() if not k.endswith("_ms")}
        out["p90_below_p10"] = out["hand_over"]["wall_us"]["p90"] < out["three_calls"]["wall_us"]["p10"]
        out["wall_gain"] = round(out["three_calls"]["wall_us"]["median"] / out["hand_over"]["wall_us"]["median"], 3)
    finally:
        for s in (sa, sb, da, db):
            s.close()
    return {"config": "hand_over", "ready": N, "observations": K, "D": D, "gallery": T, "kind": kind, "temp": NAME[src_elem],
            "store": NAME[dst_elem], "keep": "best", "rounds": rounds, "matched_last": matched, "same_bits": True, **out}


def remove_config(eng, parent_eng, N, K, D, rounds, warm=2):
    """sa_store_remove of N ids (every second one first, so that tracks move) out of N + STAY, on this library and the parent's."""
    rng = np.random.default_rng(7 * N)
    engines = {"this": eng, **({"parent": parent_eng} if parent_eng else {})}
    stores = {k: FeatureStore(e, "cosine", D, K) for k, e in engines.items()}
    wall = {k: [] for k in stores}
    try:
        ids = np.arange(1, N + STAY + 1, dtype=u64)
        banks = [rng.uniform(-1, 1, (K, D)).astype(f32) for _ in ids]
        gone = np.ascontiguousarray(np.concatenate([ids[:N:2], ids[1:N:2]]))
        for r in range(warm + rounds):
            names = list(stores) if r % 2 == 0 else list(stores)[::-1]
            for k in names:
                s = stores[k]
                s.upsert(ids, banks)
                t, _ = clock(lambda: s._chk(s.lib.sa_store_remove(s.h, len(gone), _p(gone, C.c_uint64))))
                if r >= warm:
                    wall[k].append(t)
                if k == "this":
                    last = H.last(s)
            orders = [stores[k].order().tobytes() for k in stores]
            assert all(o == orders[0] for o in orders) and len(stores["this"]) == STAY, "round %d: the libraries leave different orders" % r
            probe = rng.uniform(-1, 1, (1, D)).astype(f32)
            cells = [stores[k].search_raw([9 * 10**6], [probe], 1, 3e38, tap=True)[3].tobytes() for k in stores]
            assert all(c == cells[0] for c in cells), "round %d: the libraries leave different banks" % r
            for s in stores.values():
                s.remove(s.order())
        out = {"this": {"wall_us": pct(wall["this"])}, "parent": {"wall_us": pct(wall["parent"])} if parent_eng else "not measured"}
        if parent_eng:
            out["wall_gain"] = round(out["parent"]["wall_us"]["median"] / out["this"]["wall_us"]["median"], 3)
            out["p90_below_p10"] = out["this"]["wall_us"]["p90"] < out["parent"]["wall_us"]["p10"]
        out["launches_compact"], out["tracks_moved"] = last["launches_compact"], last["tracks_moved"]
    finally:
        for s in stores.values():
            s.close()
    return {"config": "remove", "removed": N, "of": N + STAY, "observations": K, "D": D, "store": "f32", "rounds": rounds, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes (20 ready tracks against a gallery of 200, 64-d)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--parent-lib", default=None, help="libsimilari_assoc.so built from the parent commit: sa_store_remove is timed on it too")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "handover.jsonl"))
    args = ap.parse_args()
    rounds = max(1, args.rounds)
    eng = Engine(abi.make_config(device=0))
    parent_eng = Engine(abi.make_config(device=0), lib=abi.load_library(args.parent_lib)) if args.parent_lib else None
    q = args.quick
    try:
        with open(args.out, "w") as fh:
            for line in (
                lambda: hand_over_config(eng, 20 if q else 100, 5, 64 if q else 256, 200 if q else 1000, SA_ELEM_F32, SA_ELEM_F32, "cosine", rounds),
                lambda: hand_over_config(eng, 50 if q else 500, 5, 64 if q else 256, 500 if q else 5000, SA_ELEM_F32, SA_ELEM_F32, "cosine", rounds),
                lambda: hand_over_config(eng, 50 if q else 500, 5, 64 if q else 256, 500 if q else 5000, SA_ELEM_F32, SA_ELEM_F16, "euclidean", rounds),
                lambda: remove_config(eng, parent_eng, 20 if q else 100, 5, 64 if q else 256, rounds),
                lambda: remove_config(eng, parent_eng, 50 if q else 500, 5, 64 if q else 256, rounds),
            ):
                text = json.dumps(line())
                print(text, flush=True)
                fh.write(text + "\n")
                fh.flush()
    finally:
        if parent_eng:
            parent_eng.close()
        eng.close()


if __name__ == "__main__":
    main()
