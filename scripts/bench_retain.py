"""A frame's tracks absorbed under "keep the best" in one call (include/similari_retain.h) against the two-call route it replaces —
sa_store_search_bestfit followed by sa_store_append(SA_KEEP_BEST) — on twin stores fed the same seeded frames and qualities, in one
process, one JSON line per configuration: the configurations of scripts/bench_absorb.py with a random quality per observation

  feature_tracker   benches/feature_tracker.rs: N one-observation 256-d euclidean queries per step against N tracks of capacity 3,
                    an f32 store; N = 100 and N = 500
  reid_step         64 one-observation f16 rows from a device block against 20 000 tracks x 32 at 512-d in an f16 euclidean store

Store A takes every frame through absorb_keep(SA_KEEP_BEST), store B through the two calls; the routes alternate, 7 rounds after a
warm-up of both that fills the banks.  Times are HOST-clock microseconds around the synchronous C calls, median [p10, p90] — for the
two-call route the sum of its two calls, the Python between them left out — with the device events beside them.  The two-call route
is the baseline: its kernels are the ones the library had before.  Every round asserts that both routes returned the same bits and
left the same store.  A third store takes the same frames through absorb_keep(SA_KEEP_LATEST): `step_us_latest` is its step's event
time beside `step_us`, the keep-best step's (both medians; the stores hold different rows by then, the shapes are the same).
   python scripts/bench_retain.py [--quick] [--rounds N] [--out profiles/retain.jsonl]"""
import argparse
import contextlib
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
from bench_absorb import INF, Outputs, clock, dest_of, pct, same_bits, torch  # noqa: E402  (torch's context first, as there)
from similari_amd import abi, synth  # noqa: E402
from similari_amd.devrows import DeviceRows, register_tensor  # noqa: E402
from similari_amd.engine import Engine  # noqa: E402
from similari_amd.f16 import SA_ELEM_F16, SA_ELEM_F32  # noqa: E402
from similari_amd.merge import SA_KEEP_BEST, SA_KEEP_LATEST  # noqa: E402
from similari_amd.retain import RetainStore  # noqa: E402
from similari_amd.search import _p, sa_topn_params  # noqa: E402

u32, u64, f32 = np.uint32, np.uint64, np.float32


def run_frames(a, b, c, frames, prm, cap, rounds, warm, sample=None):
    """bench_absorb.run_frames under SA_KEEP_BEST.  frames(i) -> (q_ids, n_obs, the rows argument of the C calls, rows are a device
    descriptor, one quality per observation); c: the store that takes the frames under SA_KEEP_LATEST (its step's event time only)."""
    wall = {"absorb_keep": [], "two_call": []}
    dev = {"absorb_keep": [], "two_call": []}
    step = {"best": [], "latest": []}
    uploads = []
    stats = None
    for i in range(warm + rounds):
        q_ids, n_obs, rows, is_dev, quality = frames(i)
        Q = len(q_ids)
        oa, ob, oc = Outputs(Q, prm.topn), Outputs(Q, prm.topn), Outputs(Q, prm.topn)
        capv = np.full(Q, cap, u32)
        ids_p, nobs_p, cap_p, q_p = _p(q_ids, C.c_uint64), _p(n_obs, C.c_uint32), _p(capv, C.c_uint32), _p(quality, C.c_float)

        def absorb(s, keep, o):
            fn = s.lib.sa_store_absorb_keep_dev if is_dev else s.lib.sa_store_absorb_keep
            s._chk(fn(s.h, keep, C.byref(prm), None, Q, ids_p, nobs_p, rows, None, q_p, cap_p, *o.tail(), _p(o.dest, C.c_uint64)))

        def search():
            if is_dev:
                b._chk(b.lib.sa_store_search_dev(b.h, C.byref(prm), 1, None, Q, ids_p, nobs_p, rows, None, *ob.tail(), None))
            else:
                b._chk(b.lib.sa_store_search_bestfit(b.h, C.byref(prm), None, Q, ids_p, nobs_p, rows, None, *ob.tail(), None))

        def append():
            dp = _p(ob.dest, C.c_uint64)
            if is_dev:
                b._chk(b.lib.sa_store_append_dev(b.h, SA_KEEP_BEST, Q, dp, nobs_p, rows, q_p, cap_p))
            else:
                b._chk(b.lib.sa_store_append(b.h, SA_KEEP_BEST, Q, dp, nobs_p, rows, q_p, cap_p))

        def two_call():
            t = clock(search)
            d = b.last_stats()["call_ms"]
            dest_of(q_ids, ob)
            t += clock(append)
            return t, d + b.merge_stats()["device_ms"]

        def one_call():
            t = clock(lambda: absorb(a, SA_KEEP_BEST, oa))
            return t, a.last_stats()["call_ms"] + a.retain_stats()["step_ms"]

        order = [("absorb_keep", one_call), ("two_call", two_call)]
        for k, fn in (order if i % 2 == 0 else order[::-1]):   # the routes alternate
            t, d = fn()
            if i >= warm:
                wall[k].append(t)
                dev[k].append(d * 1e-3)
        stats = a.retain_stats()
        absorb(c, SA_KEEP_LATEST, oc)
        if i >= warm:
            step["best"].append(stats["step_ms"] * 1e-3)
            step["latest"].append(c.retain_stats()["step_ms"] * 1e-3)
            uploads.append(stats["qual_upload_bytes"])
        assert same_bits(oa.all(), ob.all()), "frame %d: the two routes returned different bits" % i
        ids = a.order()
        assert np.array_equal(ids, b.order()), "frame %d: the stores hold different tracks" % i
        look = ids if sample is None else ids[sample]
        assert same_bits(a.fetch_raw(look), b.fetch_raw(look)), "frame %d: the stores hold different rows" % i
    out = {k: {"wall_us": pct(wall[k]), "device_us": pct(dev[k])} for k in wall}
    out["retain_stats"] = {k: v for k, v in stats.items() if k != "step_ms"}
    out["qual_upload_bytes_timed"] = int(sum(uploads))   # 0: in the timed rounds only the frame's own qualities crossed the bus
    out["step_us"] = pct(step["best"])["median"]
    out["step_us_latest"] = pct(step["latest"])["median"]
    out["p90_below_p10"] = out["absorb_keep"]["wall_us"]["p90"] < out["two_call"]["wall_us"]["p10"]
    out["wall_gain"] = round(out["two_call"]["wall_us"]["median"] / out["absorb_keep"]["wall_us"]["median"], 3)
    return out


def feature_tracker(eng, N, rounds, D=256, cap=3):
    rng = np.random.default_rng(N)
    ident = synth.reid_identities(rng, N, D)
    a, b, c = (RetainStore(eng, "euclidean", D, cap, SA_ELEM_F32) for _ in range(3))
    prm = sa_topn_params(1, 1, 100.0, 100.0)
    n_obs = np.ones(N, u32)
    keep = []

    def frames(i):
        feats = np.ascontiguousarray(synth.observe(rng, ident))
        quality = rng.uniform(0, 1, N).astype(f32)
        keep.append((feats, quality))
        return np.arange(1 + i * N, 1 + (i + 1) * N, dtype=u64), n_obs, _p(feats, C.c_float), False, quality

    try:
        line = run_frames(a, b, c, frames, prm, cap, rounds, warm=cap + 1)   # frame 0 creates the tracks, the next `cap` fill them
        assert len(a) == N and a.retain_stats()["matched"] == N and (a.fetch_raw(a.order())[0] == cap).all()
        groups = a.last_stats()["groups"]
    finally:
        for s in (a, b, c):
            s.close()
    return {"config": "feature_tracker", "objects": N, "kind": "euclidean", "store": "f32", "D": D, "capacity": cap, "keep": "best",
            "rounds": rounds, "groups": groups, "same_bits": True, **line}


def reid_step(eng, T, K, D, Q, rounds, gen, noise=0.05):
    ident = torch.nn.functional.normalize(torch.randn(T, D, generator=gen, device="cuda:0"), dim=1)
    rng = np.random.default_rng(T)

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
    a, b, c = (RetainStore(eng, "euclidean", D, K, SA_ELEM_F16) for _ in range(3))
    prm = sa_topn_params(1, 1, md, INF)
    n_obs = np.ones(Q, u32)
    alive = []
    try:
        with register_tensor(eng, rows):
            for st in (a, b, c):
                for t0 in range(0, T, 1000):
                    st.upsert_rows(s_ids[t0:t0 + 1000], s_n[t0:t0 + 1000], DeviceRows.from_tensor(rows[t0 * K:(t0 + 1000) * K]))
        with contextlib.ExitStack() as blocks:
            for q in q_rows:
                blocks.enter_context(register_tensor(eng, q))

            def frames(i):
                dr = DeviceRows.from_tensor(q_rows[i]).struct()
                quality = rng.uniform(0, 1, Q).astype(f32)
                alive.append((dr, quality))
                return np.arange(T + 1 + i * Q, T + 1 + (i + 1) * Q, dtype=u64), n_obs, C.byref(dr), True, quality

            line = run_frames(a, b, c, frames, prm, K, rounds, warm=2, sample=slice(None, None, max(1, T // 256)))
        groups, matched = a.last_stats()["groups"], a.retain_stats()["matched"]
        assert matched > Q // 2
    finally:
        for s in (a, b, c):
            s.close()
    return {"config": "reid_step", "queries": Q, "tracks": T, "observations": K, "kind": "euclidean", "store": "f16", "source": "float16",
            "D": D, "keep": "best", "rounds": rounds, "groups": groups, "same_bits": True, **line}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes (N = 10 and 100; 16 rows against 2000 tracks x 8, 128-d)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "retain.jsonl"))
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
