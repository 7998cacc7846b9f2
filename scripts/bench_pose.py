"""sa_points_associate (include/similari_pose.h): M poses against the T tracks of a point bank, the weight matrix and the vote in three
launches, against the only route there was before it: the same arithmetic on one host core — similari_amd/csrc/sa_pose.h over
sa_kalman_point.h through tests/emu_pose, looped over every (pose, track, point) — plus the oracle's kuhn_munkres on SortVoting's
dense M x (M + T) matrix, in the same run.  One JSON line per (size, source, scene).

  sizes    100 x 100, 500 x 500, 2000 x 2000, P = 17
  host     the poses come from host memory as f32: they cross the bus
  device   the poses lie in device memory as f16 (a registered block): nothing but the results crosses the bus
  sparse   people a gate apart and more: every pose keeps its greedy bid, the dense search has no root
  crowded  people in clusters tighter than the gate: several poses want one track, the dense search runs

Times: wall_us is the HOST clock around the Python wrapper of the synchronous C call, median [p10, p90]; kernel_us are k_pose_factor,
k_pose_tile and k_pose_assign, each from DEVICE events around its launch.  one_host_core: the host clock around the matrix loop and
around kuhn_munkres (the quantisation between them is numpy's and is not counted).  The host core runs in the first `--host-rounds`
measured rounds (all of them by default); every one of them asserts that the call's matches have kuhn_munkres's total.

   python scripts/bench_pose.py [--quick] [--rounds N] [--host-rounds N] [--out profiles/pose.jsonl]"""
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
from similari_amd.pose import PoseBank  # noqa: E402

f32, u8, u32, u64 = np.float32, np.uint8, np.uint32, np.uint64
PW = f32(1) / f32(20)
P = 17


def pct(v):
    v = np.asarray(v, np.float64) * 1e6
    return {"median": round(float(np.median(v)), 1), "p10": round(float(np.quantile(v, 0.1)), 1), "p90": round(float(np.quantile(v, 0.9)), 1)}


def clock(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def config(eng, n, source, crowd, rounds, host_rounds, warm=2):
    import hipmem
    import pose_emu as PE
    import pose_ref as PR

    rng = np.random.default_rng(n + crowd)
    ids = np.arange(1, n + 1, dtype=u64)
    centres = PR.people(rng, n, P, crowd, spacing=1.0, extent=float(np.sqrt(n)))   # small numbers: an f16 source keeps the gate's scale
    shown = PR.track_rounds(rng, centres)
    wall, kern, core_m, core_s = [], [[], [], []], [], []
    ptr = hipmem.malloc(n * P * 2 * 2) if source == "device" else 0
    bank = PoseBank(eng, P)
    try:
        if ptr:
            eng.register_device_block(ptr, n * P * 2 * 2, 0)
        for z, pres in shown:
            bank.step(ids, z, present=pres)
        has = np.zeros((n, P), bool)
        mean, cov = np.zeros((n, P, 4), f32), np.zeros((n, P, 4, 4), f32)
        for j, t in enumerate(ids):   # the host core starts from the bank's own states
            has[j], mean[j], cov[j] = bank.state(t)
        mean, cov = np.nan_to_num(mean), np.nan_to_num(cov)
        roots = matched = 0
        for r in range(warm + rounds):
            poses, pres = PR.poses_of(rng, centres, n)
            if ptr:
                half = poses.astype(np.float16)
                hipmem.upload(ptr, half.view(np.uint16))
                poses = half.astype(f32)   # widen: what the kernel reads
                t, (got, w) = clock(lambda: bank.associate(rows=DeviceRows(ptr, n, P * 2, SA_ELEM_F16), present=pres))
            else:
                t, (got, w) = clock(lambda: bank.associate(poses, present=pres))
            st = bank.last_associate()
            assert st["launches"] == 3
            if r >= warm:
                wall.append(t)
                for k in range(3):
                    kern[k].append(st["kernel_ms"][k] * 1e-3)
                roots, matched = st["roots"], st["matched"]
            if r >= warm + host_rounds:
                continue
            tm, wm = clock(lambda: PE.matrix(poses, pres, has, mean, cov, PW, 1))
            with np.errstate(invalid="ignore"):
                q = np.nan_to_num(wm * f32(1e6), nan=0.0).astype(np.int64)   # (w * 1e6f) as i64
            wq = np.zeros((n, 2 * n), np.int64)
            wq[:, n:] = q
            wq[np.arange(n), np.arange(n)] = 1000000
            ts, (total, ref) = clock(lambda: PR.solve(wq))
            col = np.where(got != 0, got.astype(np.int64) - 1, -1)
            assert PR.total_of(col, wq, 1000000) == total, "round %d: the call's matches miss kuhn_munkres's total" % r
            if r >= warm:
                core_m.append(tm)
                core_s.append(ts)
        names = ("k_pose_factor", "k_pose_tile", "k_pose_assign")
        out = {"call": {"wall_us": pct(wall)}, "kernel_us": {nm: pct(kern[k]) for k, nm in enumerate(names)},
               "one_host_core": {"matrix_us": pct(core_m), "kuhn_munkres_us": pct(core_s), "rounds": len(core_m)},
               "roots": roots, "matched": matched, "stats": {x: v for x, v in st.items() if x not in ("device_ms", "kernel_ms")}}
        host = out["one_host_core"]["matrix_us"]["median"] + out["one_host_core"]["kuhn_munkres_us"]["median"]
        out["one_host_core"]["wall_us_median"] = round(host, 1)
        out["wall_gain"] = round(host / out["call"]["wall_us"]["median"], 2)
    finally:
        bank.close()
        if ptr:
            eng.unregister_device_block(ptr)
            hipmem.free(ptr)
    return {"config": "associate", "poses": n, "tracks": n, "points": P, "source": "host f32" if not ptr else "device f16",
            "scene": "crowded" if crowd else "sparse", "rounds": rounds, "clock": "host (wall_us), device events (kernel_us)",
            "same_total_gain": True, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes (50, 200)")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--host-rounds", type=int, default=15)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pose.jsonl"))
    args = ap.parse_args()
    sizes = [50, 200] if args.quick else [100, 500, 2000]
    eng = Engine(abi.make_config(device=0))
    try:
        with open(args.out, "w") as fh:
            for n in sizes:
                for source in ("host", "device"):
                    for crowd in (False, True):
                        text = json.dumps(config(eng, n, source, crowd, max(1, args.rounds), max(1, min(args.host_rounds, args.rounds))))
                        print(text, flush=True)
                        fh.write(text + "\n")
                        fh.flush()
    finally:
        eng.close()


if __name__ == "__main__":
    main()
