"""sa_points_step (include/similari_points.h): T tracks x P keypoints stepped in one launch, against the same arithmetic on one host
core — similari_amd/csrc/sa_kalman_point.h through tests/emu_points, looped over the same points in the same run, which is how the
reference runs its point filters.  One JSON line per (size, source, order).

  sizes    1000 x 17 (a crowd with a pose network), 100 000 x 1 (the size of the reference's benches/kalman_2d_point.rs),
           20 000 x 17
  host     the points come from host memory as f32: they cross the bus with the slot table
  device   the points lie in device memory as f16 (a registered block): only the slot table and the row index cross the bus
  order    "bank": the call names the tracks in the bank's own order, which the host resolves by one comparison per id;
           "permuted": the same tracks in a fixed random order (a tracker's order after removals), every id through the hash look-ups

Times: wall_us is the HOST clock around the Python wrapper of the synchronous C call, median [p10, p90], and around the host core's
loop; kernel_us is k_points alone, from DEVICE events around its launch, with the bytes it moves (five 16-byte plane pieces and the
has byte in and out per point, the point, the output) and the rate they make.  Every round asserts that the bank's output is the host
core's bit for bit (for a device-fed bank: the host core fed the widened f16 values).

   python scripts/bench_points.py [--quick] [--rounds N] [--out profiles/points.jsonl]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from similari_amd import abi  # noqa: E402
from similari_amd.devrows import DeviceRows  # noqa: E402
from similari_amd.engine import Engine  # noqa: E402
from similari_amd.f16 import SA_ELEM_F16  # noqa: E402
from similari_amd.points import PointBank  # noqa: E402

f32, u8, u32, u64 = np.float32, np.uint8, np.uint32, np.uint64
PW, VW = f32(1) / f32(20), f32(1) / f32(160)


def pct(v):
    v = np.asarray(v, np.float64) * 1e6
    return {"median": round(float(np.median(v)), 1), "p10": round(float(np.quantile(v, 0.1)), 1), "p90": round(float(np.quantile(v, 0.9)), 1)}


def clock(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def same(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return bool(((a.view(u32) == b.view(u32)) | (np.isnan(a) & np.isnan(b))).all())


def config(eng, T, P, source, order, rounds, warm=2):
    import hipmem
    import points_emu as E

    rng = np.random.default_rng(T + P)
    ids = np.arange(1, T + 1, dtype=u64)
    pos = rng.uniform(0, 1000, (T, P, 2))
    vel = rng.uniform(-2, 2, (T, P, 2))
    has = np.zeros(T * P, u8)
    mean, cov = np.zeros((T * P, 4), f32), np.zeros((T * P, 16), f32)
    pres = np.ones(T * P, u8)
    wall, core, kern = [], [], []
    ptr = hipmem.malloc(T * P * 2 * 2) if source == "device" else 0
    perm = rng.permutation(T).astype(u32) if order == "permuted" else None
    bank = PointBank(eng, P)
    try:
        if ptr:
            eng.register_device_block(ptr, T * P * 2 * 2, 0)
        for r in range(warm + rounds):
            pos += vel + rng.normal(0, 0.5, pos.shape)
            z = pos.astype(f32)
            use = perm if perm is not None and r else None   # round 0 (a warm-up) creates the tracks in ascending order
            call_ids = ids if use is None else np.ascontiguousarray(ids[use])
            if ptr:
                half = z.astype(np.float16)
                hipmem.upload(ptr, half.view(np.uint16))
                z = half.astype(f32)   # widen: what the kernel reads
                t, xy = clock(lambda: bank.step(call_ids, rows=DeviceRows(ptr, T, P * 2, SA_ELEM_F16, use)))
            else:
                z_call = z if use is None else np.ascontiguousarray(z[use])
                t, xy = clock(lambda: bank.step(call_ids, z_call))
            st = bank.last()
            tc, want = clock(lambda: E.step(has, mean, cov, z, pres, PW, VW))
            want = want.reshape(T, P, 2)
            assert same(xy, want if use is None else want[use]), "round %d: the bank and the host core differ" % r
            assert st["launches"] == 1 and st["points"] == T * P
            if r >= warm:
                wall.append(t)
                core.append(tc)
                kern.append(st["device_ms"] * 1e-3)
        h, m, c = bank.state(int(ids[T // 2]))
        at = (T // 2) * P
        assert h.all(), "a point of track %d has no state" % ids[T // 2]
        for name, x, y in (("mean", m, mean[at: at + P]), ("cov", c.reshape(P, 16), cov[at: at + P])):
            if not same(x, y):
                bad = np.argwhere(x.view(u32) != y.view(u32))[:4]
                raise AssertionError("the states differ: %s at %s: %s against %s" % (name, bad.tolist(), [x[tuple(b)] for b in bad], [y[tuple(b)] for b in bad]))
        moved = T * P * (2 * (5 * 16 + 1) + (4 if ptr else 8) + 8 + 1) + T * 4 * (2 if ptr and perm is not None else 1)
        k = pct(kern)
        out = {"bank": {"wall_us": pct(wall)}, "one_host_core": {"wall_us": pct(core)}, "kernel_us": k, "kernel_bytes": moved,
               "kernel_GBps": round(moved / (k["median"] * 1e-6) / 1e9, 1) if k["median"] else None,
               "stats": {x: v for x, v in st.items() if x != "device_ms"}}
        out["wall_gain"] = round(out["one_host_core"]["wall_us"]["median"] / out["bank"]["wall_us"]["median"], 2)
        out["points_per_s"] = round(T * P / (out["bank"]["wall_us"]["median"] * 1e-6))
    finally:
        bank.close()
        if ptr:
            eng.unregister_device_block(ptr)
            hipmem.free(ptr)
    return {"config": "step", "tracks": T, "points": P, "source": "host f32" if not ptr else "device f16", "order": order, "rounds": rounds,
            "clock": "host (wall_us), device events (kernel_us)", "same_bits": True, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes (100 x 17, 1000 x 1)")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "points.jsonl"))
    args = ap.parse_args()
    sizes = [(100, 17), (1000, 1)] if args.quick else [(1000, 17), (100000, 1), (20000, 17)]
    eng = Engine(abi.make_config(device=0))
    try:
        with open(args.out, "w") as fh:
            for T, P in sizes:
                for source in ("host", "device"):
                    for order in ("bank", "permuted"):
                        text = json.dumps(config(eng, T, P, source, order, max(1, args.rounds)))
                        print(text, flush=True)
                        fh.write(text + "\n")
                        fh.flush()
    finally:
        eng.close()


if __name__ == "__main__":
    main()
