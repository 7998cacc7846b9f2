"""A frame's tracks absorbed in one call (include/similari_absorb.h) against the two-call route it replaces — sa_store_search_bestfit
followed by sa_store_append — on twin stores fed the same seeded frames, in one process, one JSON line per configuration:

  feature_tracker   benches/feature_tracker.rs: N one-observation 256-d euclidean queries per step against N tracks of capacity 3,
                    TopN(1, 100, 1) and keep_below 100 — no pair is pruned, N x N groups — on the unit identities scripts/bench_search.py
                    uses for this layout, an f32 store; N = 100 and N = 500
  reid_step         64 one-observation f16 rows from a device block against 20 000 tracks x 32 at 512-d in an f16 euclidean store:
                    sa_store_absorb_dev against sa_store_search_dev (BestFit) + sa_store_append_dev

Store A takes every frame through absorb, store B through the two calls; the routes alternate, 7 rounds after a warm-up of both (the
warm-up also fills the banks, so every timed step shifts full banks).  Times are HOST-clock microseconds around the synchronous C
calls, median [p10, p90] — for the two-call route the sum of its two calls, the Python between them left out — with the device events
beside them (`device_us`: the search's call_ms plus the step's, or plus the append's device_ms).  The two-call route is the baseline:
its kernels are the ones the library had before.  Every round asserts that both routes returned the same bits and left the same store.
   python scripts/bench_absorb.py [--quick] [--rounds N] [--out profiles/absorb.jsonl]"""
import argparse
import contextlib
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
torch.zeros(1, device="cuda:0")   # torch's context first, as in a process that runs its ReID model before the tracker
from similari_amd import abi, synth  # noqa: E402
from similari_amd.absorb import AbsorbStore  # noqa: E402
from similari_amd.devrows import DeviceRows, register_tensor  # noqa: E402
from similari_amd.engine import Engine  # noqa: E402
from similari_amd.f16 import SA_ELEM_F16, SA_ELEM_F32  # noqa: E402
from similari_amd.search import _p, sa_topn_params  # noqa: E402

u32, u64, f32 = np.uint32, np.uint64, np.float32
INF = float("inf")


def pct(v):
    v = np.asarray(v, np.float64) * 1e6
    return {"median": round(float(np.median(v)), 1), "p10": round(float(np.quantile(v, 0.1)), 1), "p90": round(float(np.quantile(v, 0.9)), 1)}


def clock(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def same_bits(a, b):
    return all((x is None) == (y is None) and (x is None or np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes())
               for x, y in zip(a, b))


class Outputs:
    def __init__(self, Q, topn):
        self.n, self.win, self.trk = np.zeros(Q, u32), np.zeros((Q, topn), u64), np.zeros((Q, topn), u64)
        self.wt, self.dest = np.zeros((Q, topn), np.float64), np.zeros(Q, u64)

    def tail(self):
        return [_p(self.n, C.c_uint32), _p(self.win, C.c_uint64), _p(self.trk, C.c_uint64), _p(self.wt, C.c_double)]

    def all(self):
        return self.n, self.win, self.trk, self.wt, self.dest


def dest_of(q_ids, o):
    """Step 2 of include/similari_absorb.h on the BestFit call's outputs: the glue of the two-call route (not timed)."""
    o.dest[:] = np.where((o.n >= 1) & (o.win[:, 0] != q_ids), o.win[:, 0], q_ids)


def run_frames(a, b, frames, prm, cap, rounds, warm, sample=None):
    """frames(i) -> (q_ids, n_obs, the rows argument of the C calls, rows are a device descriptor): frame i for both stores; cap: every
    query's capacity; sample: the slice of order() whose banks are compared (None: all).  -> the timing dict."""
    wall = {"absorb": [], "two_call": []}
    dev = {"absorb": [], "two_call": []}
    stats = None
    for i in range(warm + rounds):
        q_ids, n_obs, rows, is_dev = frames(i)
        Q = len(q_ids)
        oa, ob = Outputs(Q, prm.topn), Outputs(Q, prm.topn)
        capv = np.full(Q, cap, u32)
        ids_p, nobs_p, cap_p = _p(q_ids, C.c_uint64), _p(n_obs, C.c_uint32), _p(capv, C.c_uint32)

        def absorb():
            fn = a.lib.sa_store_absorb_dev if is_dev else a.lib.sa_store_absorb
            a._chk(fn(a.h, C.byref(prm), None, Q, ids_p, nobs_p, rows, None, None, cap_p, *oa.tail(), _p(oa.dest, C.c_uint64)))

        def search():
            if is_dev:
                b._chk(b.lib.sa_store_search_dev(b.h, C.byref(prm), 1, None, Q, ids_p, nobs_p, rows, None, *ob.tail(), None))
            else:
                b._chk(b.lib.sa_store_search_bestfit(b.h, C.byref(prm), None, Q, ids_p, nobs_p, rows, None, *ob.tail(), None))

        def append():
            dp = _p(ob.dest, C.c_uint64)
            if is_dev:
                b._chk(b.lib.sa_store_append_dev(b.h, 0, Q, dp, nobs_p, rows, None, cap_p))
            else:
                b._chk(b.lib.sa_store_append(b.h, 0, Q, dp, nobs_p, rows, None, cap_p))

        def two_call():
            t = clock(search)
            d = b.last_stats()["call_ms"]
            dest_of(q_ids, ob)
            t += clock(append)
            return t, d + b.merge_stats()["device_ms"]

        def one_call():
            t = clock(absorb)
            return t, a.last_stats()["call_ms"] + a.absorb_stats()["step_ms"]

        order = [("absorb", one_call), ("two_call", two_call)]
        for k, fn in (order if i % 2 == 0 else order[::-1]):   # the routes alternate
            t, d = fn()
            if i >= warm:
                wall[k].append(t)
                dev[k].append(d * 1e-3)
        stats = a.absorb_stats()
        assert same_bits(oa.all(), ob.all()), "frame %d: the two routes returned different bits" % i
        ids = a.order()
        assert np.array_equal(ids, b.order()), "frame %d: the stores hold different tracks" % i
        look = ids if sample is None else ids[sample]
        assert same_bits(a.fetch_raw(look), b.fetch_raw(look)), "frame %d: the stores hold different rows" % i
    out = {k: {"wall_us": pct(wall[k]), "device_us": pct(dev[k])} for k in wall}
    out["absorb_stats"] = {k: v for k, v in stats.items() if k != "step_ms"}
    out["step_us"] = round(stats["step_ms"] * 1e3, 1)
    out["p90_below_p10"] = out["absorb"]["wall_us"]["p90"] < out["two_call"]["wall_us"]["p10"]
    out["wall_gain"] = round(out["two_call"]["wall_us"]["median"] / out["absorb"]["wall_us"]["median"], 3)
    return out


def feature_tracker(eng, N, rounds, D=256, cap=3):
    rng = np.random.default_rng(N)
    ident = synth.reid_identities(rng, N, D)
    a, b = AbsorbStore(eng, "euclidean", D, cap, SA_ELEM_F32), AbsorbStore(eng, "euclidean", D, cap, SA_ELEM_F32)
    prm = sa_topn_params(1, 1, 100.0, 100.0)
    n_obs = np.ones(N, u32)
    keep = []

    def frames(i):
        feats = np.ascontiguousarray(synth.observe(rng, ident))
        keep.append(feats)
        return np.arange(1 + i * N, 1 + (i + 1) * N, dtype=u64), n_obs, _p(feats, C.c_float), False

    try:
        line = run_frames(a, b, frames, prm, cap, rounds, warm=cap + 1)   # frame 0 creates the tracks, the next `cap` fill them
        assert len(a) == N and a.absorb_stats()["matched"] == N and (a.fetch_raw(a.order())[0] == cap).all()
        groups = a.last_stats()["groups"]
    finally:
        a.close()
        b.close()
    return {"config": "feature_tracker", "objects": N, "kind": "euclidean", "store": "f32", "D": D, "capacity": cap, "rounds": rounds,
            "groups": groups, "same_bits": True, **line}


def reid_step(eng, T, K, D, Q, rounds, gen, noise=0.05):
    ident = torch.nn.functional.normalize(torch.randn(T, D, generator=gen, device="cuda:0"), dim=1)

    def observe(idx, k):
        x = ident[idx][:, None, :] + noise * torch.randn(len(idx), k, D, generator=gen, device="cuda:0") / D ** 0.5
        return x.reshape(len(idx) * k, D).to(torch.float16).contiguous()

    rows = observe(torch.arange(T, device="cuda:0"), K)
    n_frames = rounds + 2
    picks = [torch.randperm(T, generator=gen, device="cuda:0")[:Q] for _ in range(n_frames)]
    q_rows = [observe(p, 1) for p in picks]
    d = torch.cdist(q_rows[0].float(), rows[: 400 * K].float()).reshape(Q, -1, K).amin(dim=2)
    md = float(torch.quantile(d.flatten(), 0.01))   # about 1 % of the groups survive, the matching identity's among them
    own = torch.cdist(q_rows[0].float(), rows.reshape(T, K, D)[picks[0], 0].float()).diagonal().max()
    md = max(md, float(own) * 1.5)
    torch.cuda.synchronize()
    s_ids, s_n = np.arange(1, T + 1, dtype=u64), np.full(T, K, u32)
    a, b = AbsorbStore(eng, "euclidean", D, K, SA_ELEM_F16), AbsorbStore(eng, "euclidean", D, K, SA_ELEM_F16)
    prm = sa_topn_params(1, 1, md, INF)
    n_obs = np.ones(Q, u32)
    alive = []
    try:
        with register_tensor(eng, rows):
            for st in (a, b):
                for t0 in range(0, T, 1000):
                    st.upsert_rows(s_ids[t0:t0 + 1000], s_n[t0:t0 + 1000], DeviceRows.from_tensor(rows[t0 * K:(t0 + 1000) * K]))
        with contextlib.ExitStack() as blocks:
            for q in q_rows:
                blocks.enter_context(register_tensor(eng, q))

            def frames(i):
                dr = DeviceRows.from_tensor(q_rows[i]).struct()
                alive.append(dr)
                return np.arange(T + 1 + i * Q, T + 1 + (i + 1) * Q, dtype=u64), n_obs, C.byref(dr), True

            line = run_frames(a, b, frames, prm, K, rounds, warm=2, sample=slice(None, None, max(1, T // 256)))
        groups, matched = a.last_stats()["groups"], a.absorb_stats()["matched"]
        assert matched > Q // 2
    finally:
        a.close()
        b.close()
    return {"config": "reid_step", "queries": Q, "tracks": T, "observations": K, "kind": "euclidean", "store": "f16", "source": "float16",
            "D": D, "rounds": rounds, "groups": groups, "same_bits": True, **line}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes (N = 10 and 100; 16 rows against 2000 tracks x 8, 128-d)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "absorb.jsonl"))
    args = ap.parse_args()
    rounds = max(1, args.rounds)
    T, K, D, Q = (2000, 8, 128, 16) if args.quick else (20000, 32, 512, 64)
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    eng = Engine(abi.make_config(device=0))
    try:
        with open(args.out, "w") as fh:
            for line in (
                lambda: feature_tracker(eng, 10 if args.quick else 100, rounds),
                lambda: feature_tracker(eng, 100 if args.quick else 500, rounds),
                lambda: reid_step(eng, T, K, D, Q, rounds, gen),
            ):
                text = json.dumps(line())
                print(text, flush=True)
                fh.write(text + "\n")
                fh.flush()
    finally:
        eng.close()


if __name__ == "__main__":
    main()
