"""Frame preprocessing for a whole batch (include/similari_frames.h) against the only route the calls before it offer: S single
calls — sa_own_areas or sa_nms, one per scene — against ONE sa_own_areas_batch / sa_nms_batch over the same S scenes, on one engine,
in one process, the routes alternating round by round after a warm-up.  One JSON line per configuration:
S in {8, 64} scenes x {100, 500, 1000} boxes, axis-aligned and oriented, own areas and NMS.

Times are HOST-clock microseconds around the Python wrappers of the synchronous C calls (the box arrays are converted before the clock
starts; the wrappers' own work — pointer arrays, result copies — is inside, on both routes), median [p10, p90].  device_us is the
batch call's own device time, first launch to last, from device events (sa_frames_stats.device_ms).  Every round asserts that both
routes agreed: NMS index for index, own areas to 1e-6 (the count of shares that differ in any bit is reported).

   python scripts/bench_frames.py [--quick] [--rounds N] [--out profiles/frames_batch.jsonl]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from similari_amd import abi, frames, synth  # noqa: E402
from similari_amd.engine import Engine  # noqa: E402


def pct(v):
    v = np.asarray(v, np.float64) * 1e6
    return {"median": round(float(np.median(v)), 1), "p10": round(float(np.quantile(v, 0.1)), 1), "p90": round(float(np.quantile(v, 0.9)), 1)}


def clock(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def scene(rng, n, oriented, nms):
    b = synth.dense_boxes(rng, n - n // 3 if nms else n, (1920.0, 1080.0), oriented=oriented)
    if nms:   # clusters of near-duplicates, as a detector emits them
        dup = synth.jitter_boxes(rng, b[: n // 3], 3.0, size_rel=0.05, angle_sigma=0.05 if oriented else 0.0)
        b = np.concatenate([b, dup])[rng.permutation(n)]
    return np.ascontiguousarray(b, abi.BOX_DTYPE)


def config(eng, what, S, n, oriented, rounds, warm=3):
    rng = np.random.default_rng(1000 * S + n + oriented)
    nms = what == "nms"
    scenes = [scene(rng, n, oriented, nms) for _ in range(S)]
    scores = [rng.uniform(0.0, 1.0, n).astype(np.float32) for _ in range(S)] if nms else None
    if nms:
        single = lambda: [eng.nms(b, s, 0.5, 0.2) for b, s in zip(scenes, scores)]
        batch = lambda: frames.nms_batch(eng, scenes, scores, 0.5, 0.2)
    else:
        single = lambda: [eng.own_areas(b) for b in scenes]
        batch = lambda: frames.own_areas_batch(eng, scenes)
    t_single, t_batch, dev, differ = [], [], [], 0
    for r in range(warm + rounds):
        order = (single, batch) if r & 1 else (batch, single)   # the routes alternate, and so does which one goes first
        res = {}
        for fn in order:
            dt, out = clock(fn)
            res[fn] = out
            if r >= warm:
                (t_single if fn is single else t_batch).append(dt)
            if fn is batch:
                st = frames.last_stats(eng)
                if r >= warm:
                    dev.append(st["device_ms"] * 1e-3)
        for a, b in zip(res[single], res[batch]):
            if nms:
                assert np.array_equal(a, b)
            else:
                assert np.abs(a - b).max() < 1e-6
                differ += int((a.view(np.uint32) != b.view(np.uint32)).sum())
    ts, tb = pct(t_single), pct(t_batch)
    return {"what": what, "scenes": S, "boxes_per_scene": n, "oriented": bool(oriented), "rounds": rounds,
            "single_calls_us": ts, "batch_call_us": tb, "batch_device_us": pct(dev), "speedup_median": round(ts["median"] / tb["median"], 2),
            "single_call_us_each": round(ts["median"] / S, 1), "launches": st["launches"], "host_waits": st["host_waits"],
            "boxes_on_device": st["boxes"], "spilled": st["spilled"], "bytes_h2d": st["bytes_h2d"], "bytes_d2h": st["bytes_d2h"],
            "shares_differing_in_any_bit": None if nms else differ}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    eng = Engine(abi.make_config())
    lines = []
    try:
        for what in ("own_areas", "nms"):
            for S in ((8,) if a.quick else (8, 64)):
                for n in ((100,) if a.quick else (100, 500, 1000)):
                    for oriented in (False, True):
                        line = config(eng, what, S, n, oriented, 5 if a.quick else a.rounds)
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
