"""A store's mutual best pairs merged in one call (include/similari_consolidate.h) against the two-call route it replaces —
sa_store_join_bestfit followed by sa_store_merge — on twin stores, in one process, one JSON line per configuration:

  tracklet_pairs    T tracks of two 256-d observations, tracks 2i and 2i + 1 on one identity (uniform idents, noise 0.02; an i8
                    store: normal idents, the sign alternating, cosine), max_observations 4, TopN(1), the cut between the pairs and
                    the strangers: T / 2 pairs merge, every second track leaves.  T = 2000 and T = 10000 in an f32 euclidean store,
                    the same gallery in an i8 cosine store.

A consolidation consumes its input, so both stores are rebuilt from the same seeded banks every round and joined once untimed (the
group pool then fits, and neither route pays its growth); then store A takes the one call and store B the two, the routes alternating.
Times are HOST-clock microseconds around the synchronous C calls, median [p10, p90] — for the two-call route the sum of its two calls;
the Python between them (the pairs from the join's outputs) is left out and reported separately as glue_us — with the device events
beside them (`device_us`: the join's call_ms plus the step's and the compaction's, or plus the merge's device_ms).  The two-call route
is the baseline: its kernels are the ones the library had before.  Every round asserts that both routes returned the same bits and
left the same store.
   python scripts/bench_consolidate.py [--quick] [--rounds N] [--out profiles/consolidate.jsonl]"""
import argparse
import ctypes as C
import json
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from similari_amd import abi, consolidate as CO  # noqa: E402
from similari_amd.engine import Engine  # noqa: E402
from similari_amd.f16 import SA_ELEM_F32  # noqa: E402
from similari_amd.i8 import I8Store  # noqa: E402
from similari_amd.retain import RetainStore  # noqa: E402
from similari_amd.search import _p, sa_topn_params  # noqa: E402

u32, u64, f32 = np.uint32, np.uint64, np.float32


def pct(v):
    v = np.asarray(v, np.float64) * 1e6
    return {"median": round(float(np.median(v)), 1), "p10": round(float(np.quantile(v, 0.1)), 1), "p90": round(float(np.quantile(v, 0.9)), 1)}


def clock(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def same_bits(a, b):
    return all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(a, b))


class Outputs:
    def __init__(self, T):
        self.n, self.win, self.trk, self.wt = np.zeros(T, u32), np.zeros((T, 1), u64), np.zeros((T, 1), u64), np.zeros((T, 1), np.float64)
        self.ids, self.dest = np.zeros(T, u64), np.zeros(T, u64)

    def join(self):
        return [_p(self.n, C.c_uint32), _p(self.win, C.c_uint64), _p(self.trk, C.c_uint64), _p(self.wt, C.c_double)]

    def all(self):
        return self.n, self.win, self.trk, self.wt, self.ids, self.dest


def pairs_of(o):
    """Step 2 of include/similari_consolidate.h on the join's outputs: the glue of the two-call route.  -> (dst ids, src ids)"""
    ids = o.ids
    w = np.where(o.n >= 1, o.win[:, 0], ids)
    by_id = np.argsort(ids)
    at = by_id[np.searchsorted(ids[by_id], w)]   # every winner is a stored id
    mutual = (w != ids) & (w[at] == ids) & (ids < w)
    o.dest[:] = ids
    o.dest[at[mutual]] = ids[mutual]
    return np.ascontiguousarray(ids[mutual]), np.ascontiguousarray(w[mutual])


def tracklet_pairs(eng, T, store, rounds, D=256, K=4, n_obs=2, warm=1):
    kind = "cosine" if store == "i8" else "euclidean"
    rng = np.random.default_rng(T)
    ident = rng.normal(0, 1, (T // 2, D)) if kind == "cosine" else rng.uniform(0, 1, (T // 2, D))
    sign = np.where((np.arange(T) % 2 == 1) & (kind == "cosine"), -1.0, 1.0)
    rows = (sign[:, None, None] * ident[np.arange(T) // 2][:, None, :] + rng.normal(0, 0.02, (T, n_obs, D))).astype(f32)
    ids = np.arange(1, T + 1, dtype=u64)
    banks = list(rows)
    cut = -0.9 if kind == "cosine" else 0.08 * math.sqrt(2 * D)
    prm = sa_topn_params(1, 1, cut, math.inf)
    wall = {"consolidate": [], "two_call": []}
    dev = {"consolidate": [], "two_call": []}
    glue, stats, groups = [], None, 0
    for i in range(warm + rounds):
        a, b = [I8Store(eng, "cosine", D, K) if store == "i8" else RetainStore(eng, kind, D, K, SA_ELEM_F32) for _ in range(2)]
        try:
            CO._lib(a)
            for s in (a, b):
                for t0 in range(0, T, 1000):
                    s.upsert(ids[t0:t0 + 1000], banks[t0:t0 + 1000])
                s.join_bestfit_raw(1, cut)   # untimed: the pool grows here
            oa, ob = Outputs(T), Outputs(T)

            def one_call():
                t = clock(lambda: a._chk(a.lib.sa_store_consolidate(a.h, 0, C.byref(prm), None, 0, *oa.join(), _p(oa.ids, C.c_uint64),
                                                                    _p(oa.dest, C.c_uint64))))
                st = CO.last(a)
                return t, a.last_stats()["call_ms"] + st["step_ms"] + st["compact_ms"]

            def two_call():
                ob.ids[:] = b.order()
                t = clock(lambda: b._chk(b.lib.sa_store_join_bestfit(b.h, C.byref(prm), None, *ob.join(), None)))
                d = b.last_stats()["call_ms"]
                g = time.perf_counter()
                dst, src = pairs_of(ob)
                ones = np.ones(len(dst), u32)
                glue.append(time.perf_counter() - g)
                t += clock(lambda: b._chk(b.lib.sa_store_merge(b.h, 0, len(dst), _p(dst, C.c_uint64), _p(ones, C.c_uint32), _p(src, C.c_uint64), None)))
                return t, d + b.merge_stats()["device_ms"]

            order = [("consolidate", one_call), ("two_call", two_call)]
            for k, fn in (order if i % 2 == 0 else order[::-1]):   # the routes alternate
                t, d = fn()
                if i >= warm:
                    wall[k].append(t)
                    dev[k].append(d * 1e-3)
            stats, groups = CO.last(a), a.last_stats()["groups"]
            assert stats["pairs"] == T // 2 and len(a) == T // 2, "round %d: %d pairs" % (i, stats["pairs"])
            assert same_bits(oa.all(), ob.all()), "round %d: the two routes returned different bits" % i
            left = a.order()
            assert np.array_equal(left, b.order()), "round %d: the stores hold different tracks" % i
            look = left[:: max(1, len(left) // 256)]
            assert same_bits(a.fetch_raw(look), b.fetch_raw(look)), "round %d: the stores hold different rows" % i
        finally:
            a.close()
            b.close()
    out = {k: {"wall_us": pct(wall[k]), "device_us": pct(dev[k])} for k in wall}
    one, two = out["consolidate"]["wall_us"], out["two_call"]["wall_us"]
    return {"config": "tracklet_pairs", "tracks": T, "observations": n_obs, "kind": kind, "store": store, "D": D, "capacity": K, "rounds": rounds,
            "groups": groups, "same_bits": True, **out, "glue_us": pct(glue[warm:]),
            "consolidate_stats": {k: v for k, v in stats.items() if not k.endswith("_ms")},
            "step_us": round(stats["step_ms"] * 1e3, 1), "compact_us": round(stats["compact_ms"] * 1e3, 1),
            "p90_below_p10": one["p90"] < two["p10"], "above_the_spread": one["median"] - two["median"] > two["p90"] - two["p10"],
            "wall_gain": round(two["median"] / one["median"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes (T = 200 and 1000)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "consolidate.jsonl"))
    args = ap.parse_args()
    rounds = max(1, args.rounds)
    small, large = (200, 1000) if args.quick else (2000, 10000)
    eng = Engine(abi.make_config(device=0))
    try:
        with open(args.out, "w") as fh:
            for T, store in ((small, "f32"), (large, "f32"), (small, "i8"), (large, "i8")):
                text = json.dumps(tracklet_pairs(eng, T, store, rounds))
                print(text, flush=True)
                fh.write(text + "\n")
                fh.flush()
    finally:
        eng.close()


if __name__ == "__main__":
    main()
