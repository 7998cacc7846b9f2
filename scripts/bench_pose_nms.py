"""Pose NMS by OKS (include/similari_pose_nms.h) against what a user has without it: the host emulator of the same arithmetic
(tests/emu_pose_nms: similari_amd/csrc/sa_pose_nms.h compiled by g++, one core), and — for a batch — the S single calls.  One engine,
one process, the routes alternating round by round after a warm-up.  One JSON line per configuration: 1 x 200, 8 x 200 and 64 x 200
poses at P = 17 and one scene of 2000 poses, each fed from the host (f32) and fed f16 from device memory.

Times are HOST-clock microseconds around the Python wrappers of the synchronous calls (arrays are converted before the clock starts),
median [p10, p90]; device_us is the call's own device time, first launch to last, from device events (sa_pose_nms_stats.device_ms).
The emulator is fed the values the device reads (the f16 values widened), and every round asserts that all routes kept the same poses.

   python scripts/bench_pose_nms.py [--quick] [--rounds N] [--out profiles/pose_nms.jsonl]"""
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
from similari_amd import pose_nms as N  # noqa: E402
from similari_amd.devrows import DeviceRows  # noqa: E402
from similari_amd.engine import Engine  # noqa: E402
from similari_amd.f16 import SA_ELEM_F16  # noqa: E402

P, NMS_THR, SCORE_THR = 17, 0.7, 0.1


def pct(v):
    v = np.asarray(v, np.float64) * 1e6
    return {"median": round(float(np.median(v)), 1), "p10": round(float(np.quantile(v, 0.1)), 1), "p90": round(float(np.quantile(v, 0.9)), 1)}


def clock(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def config(eng, S, n, source, rounds, warm=3):
    import hipmem
    import pose_nms_emu as EMU
    import pose_nms_ref as NR

    sig = np.asarray(N.COCO_SIGMAS, np.float32)
    scenes = []
    for s in range(S):   # a third of the poses are people, the rest their jittered duplicates: what a pose network emits
        pts, scores, _ = NR.crowd(10000 * S + 10 * n + s, max(1, n // 3), n, P, jitter=0.02, size=60.0, spread=400.0)
        scenes.append((pts.astype(np.float16).astype(np.float32) if source == "device" else pts, scores))
    kw = dict(sigmas=sig, nms_threshold=NMS_THR, score_threshold=SCORE_THR)
    ptr, rows = 0, None
    try:
        if source == "device":
            image = np.concatenate([z for z, _ in scenes]).astype(np.float16).reshape(S * n, P * 2)
            ptr = hipmem.malloc(image.nbytes)
            hipmem.upload(ptr, image.view(np.uint16))
            eng.register_device_block(ptr, image.nbytes, 0)
            rows = DeviceRows(ptr, S * n, P * 2, SA_ELEM_F16)
            one = lambda s: N.pose_nms(eng, None, scenes[s][1], rows=DeviceRows(ptr + s * n * P * 4, n, P * 2, SA_ELEM_F16), **kw)
            batch = lambda: N.pose_nms_batch(eng, [(None, sc) for _, sc in scenes], rows=rows, **kw)
        else:
            one = lambda s: N.pose_nms(eng, scenes[s][0], scenes[s][1], **kw)
            batch = lambda: N.pose_nms_batch(eng, scenes, **kw)
        single = lambda: [one(s) for s in range(S)]
        if S == 1:
            batch = single   # one scene: the single call is the call
        host = lambda: [EMU.nms(z, sc, sig, NMS_THR, SCORE_THR) for z, sc in scenes]
        routes = [batch, host] if S == 1 else [batch, single, host]
        t = {fn: [] for fn in routes}
        dev, st = [], None
        for r in range(warm + rounds):
            res = {}
            for fn in routes[r % len(routes):] + routes[: r % len(routes)]:   # who goes first rotates
                dt, res[fn] = clock(fn)
                if fn is batch:
                    st = N.last(eng)
                if r >= warm:
                    t[fn].append(dt)
                    if fn is batch:
                        dev.append(st["device_ms"] * 1e-3)
            for fn in routes[1:]:
                assert all(np.array_equal(a, b) for a, b in zip(res[batch], res[fn]))
        kept = sum(len(k) for k in res[batch])
    finally:
        if ptr:
            eng.unregister_device_block(ptr)
            hipmem.free(ptr)
    line = {"scenes": S, "poses_per_scene": n, "points": P, "source": "host f32" if source == "host" else "device f16", "rounds": rounds,
            "call_us": pct(t[batch]), "device_us": pct(dev), "host_emulator_us": pct(t[host]),
            "single_calls_us": pct(t[single]) if S > 1 else None, "launches": st["launches"], "host_waits": st["host_waits"],
            "poses_on_device": st["poses"], "kept": kept, "bytes_h2d": st["bytes_h2d"], "bytes_d2h": st["bytes_d2h"], "src_bytes": st["src_bytes"]}
    line["ahead_of_host_emulator"] = "device" if line["call_us"]["median"] < line["host_emulator_us"]["median"] else "host"
    if S > 1:
        line["ahead_of_single_calls"] = "batch" if line["call_us"]["median"] < line["single_calls_us"]["median"] else "single calls"
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    eng = Engine(abi.make_config())
    lines = []
    try:
        for S, n in ((1, 200), (8, 200)) if a.quick else ((1, 200), (8, 200), (64, 200), (1, 2000)):
            for source in ("host", "device"):
                line = config(eng, S, n, source, 5 if a.quick else a.rounds)
                print(json.dumps(line), flush=True)
                lines.append(line)
    finally:
        eng.close()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
