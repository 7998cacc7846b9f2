"""Feature rows read from device memory (include/similari_devrows.h) against the host-fed calls, on the same seeded rows, in one
process, one JSON line per configuration:

  track_search   benches/track_search.rs: one 30-observation query against 1000 tracks of 30, 512-d, an f32 store and an f32 source
  reid           the re-identification search of DESIGN section 10 (64 queries x 32 against 20 000 tracks x 32, 512-d, about 1 % of the
                 groups surviving) on an f16 store with an f16 source
  bulk_upsert    loading that store: 20 000 x 32 x 512-d, an f16 source into an f16 store, in slices of 1000 tracks on either side

The host-fed call and the *_dev call alternate, 7 rounds after a warm-up of both.  Times are HOST-clock microseconds around the
synchronous C call, median [p10, p90]: the stores' device events (`call_us`, printed beside) do not see the host's spreading of the
rows or the copy out of pageable memory, which are what the *_dev calls remove.  For the f16 configurations the host-fed side is
timed twice: `host` is handed f32 rows that are already on the host, `host_with_copy` first brings the fp16 device rows to the host
and widens them (torch: .float().cpu()), as a caller holding a ReID network's output must.  The host-fed call is the baseline: the
code path the library had before.  Every configuration asserts that both calls returned (or left in the store) the same bits.
   python scripts/bench_devrows.py [--quick] [--rounds N] [--out profiles/devrows.jsonl]"""
import argparse
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
from similari_amd import abi  # noqa: E402
from similari_amd.devrows import DeviceRows, DeviceRowsStore, register_tensor  # noqa: E402
from similari_amd.engine import Engine  # noqa: E402
from similari_amd.f16 import SA_ELEM_F16, SA_ELEM_F32  # noqa: E402
from similari_amd.search import _p, sa_topn_params  # noqa: E402

u32, u64 = np.uint32, np.uint64
INF = float("inf")


def pct(v):
    v = np.asarray(v, np.float64) * 1e6
    return {"median": round(float(np.median(v)), 1), "p10": round(float(np.quantile(v, 0.1)), 1), "p90": round(float(np.quantile(v, 0.9)), 1)}


def clock(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def embeddings(gen, T, K, D, dtype, noise=0.05):
    """[T * K][D] on the GPU: K noisy observations of T unit identities (track-major), and the identities."""
    ident = torch.nn.functional.normalize(torch.randn(T, D, generator=gen, device="cuda:0"), dim=1)
    obs = ident[:, None, :] + noise * torch.randn(T, K, D, generator=gen, device="cuda:0") / D ** 0.5
    return obs.reshape(T * K, D).to(dtype).contiguous(), ident


def threshold(kind, q, s, K, frac):
    """max_distance that keeps about `frac` of the (query, track) groups: from the best cell of every group of a sample of tracks."""
    s = s[: 400 * K].float()
    q = q.float()
    d = torch.cdist(q, s) if kind == "euclidean" else 1.0 - torch.nn.functional.normalize(q, dim=1) @ torch.nn.functional.normalize(s, dim=1).T
    best = d.reshape(q.shape[0] // K, K, -1, K).amin(dim=(1, 3))
    return float(torch.quantile(best.flatten(), frac))


def upsert_host(st, ids, n_obs, feats):
    st._chk(st.lib.sa_store_upsert(st.h, len(ids), _p(ids, C.c_uint64), _p(n_obs, C.c_uint32), _p(feats, C.c_float)))


def same_bits(a, b):
    return all((x is None) == (y is None) and (x is None or np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes())
               for x, y in zip(a, b))


def search_lines(eng, name, kind, elem, dtype, T, K, Kq, D, Q, topn, frac, rounds, gen, with_copy):
    """A host-fed search against sa_store_search_dev on one store."""
    rows, _ = embeddings(gen, T, K, D, dtype)
    q_rows, _ = embeddings(gen, Q, Kq, D, dtype)
    md = threshold(kind, q_rows[: Q * Kq], rows, K, frac) if frac else INF
    s_ids, s_n = np.arange(1, T + 1, dtype=u64), np.full(T, K, u32)
    q_ids, q_n = np.arange(T + 1, T + Q + 1, dtype=u64), np.full(Q, Kq, u32)
    q_host = np.ascontiguousarray(q_rows.float().cpu().numpy())
    torch.cuda.synchronize()
    prm = sa_topn_params(topn, 1, md, INF)
    out = {s: (np.zeros(Q, u32), np.zeros((Q, topn), u64), np.zeros((Q, topn), np.float64)) for s in ("host", "dev")}
    st = DeviceRowsStore(eng, kind, D, max(K, Kq), elem)
    try:
        with register_tensor(eng, rows), register_tensor(eng, q_rows):
            for t0 in range(0, T, 1000):
                st.upsert_rows(s_ids[t0:t0 + 1000], s_n[t0:t0 + 1000], DeviceRows.from_tensor(rows[t0 * K:(t0 + 1000) * K]))
            d = DeviceRows.from_tensor(q_rows).struct()

            def host(feats=q_host):
                o = out["host"]
                st._chk(st.lib.sa_store_search_topn(st.h, C.byref(prm), Q, _p(q_ids, C.c_uint64), _p(q_n, C.c_uint32), _p(feats, C.c_float),
                                                    _p(o[0], C.c_uint32), _p(o[1], C.c_uint64), _p(o[2], C.c_double), None))

            def host_with_copy():
                host(np.ascontiguousarray(q_rows.float().cpu().numpy()))

            def dev():
                o = out["dev"]
                st._chk(st.lib.sa_store_search_dev(st.h, C.byref(prm), 0, None, Q, _p(q_ids, C.c_uint64), _p(q_n, C.c_uint32), C.byref(d), None,
                                                   _p(o[0], C.c_uint32), _p(o[1], C.c_uint64), None, _p(o[2], C.c_double), None))

            calls = {"host": host, "dev": dev}
            if with_copy:
                calls["host_with_copy"] = host_with_copy
            for fn in calls.values():   # warm-up: buffers, the pool's growth
                fn()
            wall = {k: [] for k in calls}
            event = {k: [] for k in calls}
            for _ in range(rounds):
                for k, fn in calls.items():
                    wall[k].append(clock(fn))
                    event[k].append(st.last_stats()["call_ms"] * 1e-3)
            groups = st.last_stats()["groups"]
            stats = st.devrows_stats()
    finally:
        st.close()
    assert same_bits(out["host"], out["dev"]), "the host-fed call and the *_dev call differ"
    assert out["dev"][0].sum() > 0
    line = {"config": name, "kind": kind, "store": "f32" if elem == SA_ELEM_F32 else "f16", "source": str(dtype).rsplit(".", 1)[-1],
            "queries": Q, "query_observations": Kq, "tracks": T, "observations": K, "D": D, "rounds": rounds, "groups": groups, "same_bits": True,
            "devrows": stats}
    for k in calls:
        line[k] = {"wall_us": pct(wall[k]), "call_us": pct(event[k])}
    line["wall_gain"] = round(line["host"]["wall_us"]["median"] / line["dev"]["wall_us"]["median"], 3)
    if with_copy:
        line["wall_gain_with_copy"] = round(line["host_with_copy"]["wall_us"]["median"] / line["dev"]["wall_us"]["median"], 3)
    return line


def upsert_line(eng, T, K, D, rounds, gen, slice_tracks=1000):
    """Loading an f16 store from fp16 device rows, in slices of `slice_tracks` tracks on either side."""
    rows, _ = embeddings(gen, T, K, D, torch.float16)
    ids, n_obs = np.arange(1, T + 1, dtype=u64), np.full(T, K, u32)
    host_rows = np.ascontiguousarray(rows.float().cpu().numpy())
    torch.cuda.synchronize()
    slices = [(t0, min(t0 + slice_tracks, T)) for t0 in range(0, T, slice_tracks)]
    a, b = DeviceRowsStore(eng, "euclidean", D, K, SA_ELEM_F16), DeviceRowsStore(eng, "euclidean", D, K, SA_ELEM_F16)
    try:
        with register_tensor(eng, rows):
            def host(copy=False):
                for t0, t1 in slices:
                    feats = np.ascontiguousarray(rows[t0 * K:t1 * K].float().cpu().numpy()) if copy else host_rows[t0 * K:t1 * K]
                    upsert_host(b, ids[t0:t1], n_obs[t0:t1], feats)

            def dev():
                for t0, t1 in slices:
                    a.upsert_rows(ids[t0:t1], n_obs[t0:t1], DeviceRows.from_tensor(rows[t0 * K:t1 * K]))

            calls = {"host": host, "host_with_copy": lambda: host(True), "dev": dev}
            for fn in calls.values():
                fn()
            wall = {k: [] for k in calls}
            for _ in range(rounds):
                for k, fn in calls.items():
                    wall[k].append(clock(fn))
            stats = a.devrows_stats()
        sample = ids[:: max(1, T // 256)]
        assert np.array_equal(a.order(), b.order()) and same_bits(a.fetch_raw(sample), b.fetch_raw(sample)), "the two stores differ"
        q = [host_rows[i * K:(i + 1) * K] for i in range(4)]
        q_ids = np.arange(T + 1, T + 5, dtype=u64)
        assert same_bits(a.search_raw(q_ids, q, 5, INF), b.search_raw(q_ids, q, 5, INF)), "a search of the two stores differs"
    finally:
        a.close()
        b.close()
    line = {"config": "bulk_upsert", "kind": "euclidean", "store": "f16", "source": "float16", "tracks": T, "observations": K, "D": D,
            "slice_tracks": slice_tracks, "rounds": rounds, "same_bits": True, "devrows_last_slice": stats,
            "source_bytes": T * K * D * 2, "host_f32_bytes": T * K * D * 4}
    for k in calls:
        line[k] = {"wall_us": pct(wall[k])}
    line["wall_gain"] = round(line["host"]["wall_us"]["median"] / line["dev"]["wall_us"]["median"], 3)
    line["wall_gain_with_copy"] = round(line["host_with_copy"]["wall_us"]["median"] / line["dev"]["wall_us"]["median"], 3)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes (2000 tracks x 8, 128-d)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "devrows.jsonl"))
    args = ap.parse_args()
    rounds = max(1, args.rounds)
    T, K, D, Q = (2000, 8, 128, 16) if args.quick else (20000, 32, 512, 64)
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    eng = Engine(abi.make_config(device=0))
    try:
        with open(args.out, "w") as fh:
            for line in (
                lambda: search_lines(eng, "track_search", "euclidean", SA_ELEM_F32, torch.float32, 1000, 30, 30, 512, 1, 5, 0.1, rounds, gen, False),
                lambda: search_lines(eng, "reid", "euclidean", SA_ELEM_F16, torch.float16, T, K, K, D, Q, 10, 0.01, rounds, gen, True),
                lambda: upsert_line(eng, T, K, D, rounds, gen),
            ):
                text = json.dumps(line())
                print(text, flush=True)
                fh.write(text + "\n")
                fh.flush()
    finally:
        eng.close()


if __name__ == "__main__":
    main()
