"""sa_points_track / sa_points_track_batch (include/similari_pose_track.h): the keypoint frame loop — associate, step, coast — in ONE call,
against the route there was before it: PoseBank.track / track_batch, one associate, one step and one predict with the host between
them, on a twin bank in the same run and on the same frames.  One JSON line per (case, scene kind, source).

  cases    S in {1, 8, 64} scenes of 100 x 100, 8 scenes of 500 x 500; P = 17.  S = 1 is the single form against PoseBank.track
  sparse   people a gate apart and more: every pose keeps its greedy bid, the dense search has no root
  crowded  people in clusters tighter than the gate: several poses want one track, the dense search runs
  source   host f32: both routes are fed the poses from host memory.  dev f16: the one call reads the poses where they lie in device
           memory as f16; the three calls have no such path through track(), so the twin is fed the same values widened on the host

A fifth of the poses of a frame show somebody new, so every frame creates tracks; they are removed from both banks after the round
(outside the clocks), so that every round runs on S x n listed tracks.

Times: wall_us is the HOST clock around the Python wrapper of each route, median [p10, p90]; kernel_us are the five launches of the
one call (factor, tile, assign, scan, step), each from DEVICE events around its launch.  bytes: what each route sent over the bus, both
ways; the three calls' are summed over their records.  Every round asserts that the two routes gave every pose the same id and left
the same order and, bit for bit, the same states: on a sample of 128 tracks and all created ones, in the last round on every track.

   python scripts/bench_pose_track.py [--quick] [--rounds N] [--out profiles/pose_track.jsonl]"""
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
from similari_amd.pose_track import PoseTrackBank  # noqa: E402

f32, u64 = np.float32, np.uint64
P = 17
NAMES = ("k_pose_factor", "k_pose_tile", "k_pose_assign", "k_pose_scan", "k_pose_step")


def pct(v):
    v = np.asarray(v, np.float64) * 1e6
    return {"median": round(float(np.median(v)), 1), "p10": round(float(np.quantile(v, 0.1)), 1), "p90": round(float(np.quantile(v, 0.9)), 1)}


def clock(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def same(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


class Counted(PoseBank):
    """The yardstick, unchanged; it only adds up what its calls send over the bus."""

    bus = 0

    def _count(self, st):
        self.bus += st["bytes_h2d"] + st["bytes_d2h"]

    def associate(self, *a, **kw):
        out = super().associate(*a, **kw)
        self._count(self.last_associate())
        return out

    def associate_batch(self, *a, **kw):
        out = super().associate_batch(*a, **kw)
        self._count(self.last_associate_batch())
        return out

    def step(self, *a, **kw):
        out = super().step(*a, **kw)
        self._count(self.last())
        return out

    def predict(self, *a, **kw):
        out = super().predict(*a, **kw)
        self._count(self.last())
        return out


def config(eng, S, n, crowd, device, rounds, warm=2):
    import hipmem
    import pose_ref as PR

    rng = np.random.default_rng(1000 * S + n + crowd)
    ids = [np.arange(1, n + 1, dtype=u64) + u64(s * n) for s in range(S)]
    every = np.concatenate(ids)
    centres = [PR.people(rng, n, P, crowd, spacing=1.0, extent=float(np.sqrt(n))) for _ in range(S)]   # the scale of bench_pose.py
    shown = PR.track_rounds(rng, np.concatenate(centres))
    m = S * n
    next_id = 10 * m
    wall_one, wall_three, kern, bus_one, bus_three = [], [], [[] for _ in NAMES], [], []
    ptr = hipmem.malloc(m * P * 2 * 2) if device else None
    try:
        if device:
            eng.register_device_block(ptr, m * P * 2 * 2, 0)
        with PoseTrackBank(eng, P) as a, Counted(eng, P) as b:
            for z, pres in shown:
                a.step(every, z, present=pres)
                b.step(every, z, present=pres)
            for r in range(warm + rounds):
                frame = [PR.poses_of(rng, c, n) for c in centres]
                z, pres = np.concatenate([f[0] for f in frame]), np.concatenate([f[1] for f in frame])
                if device:   # the network's output: f16 in device memory; the twin gets what those bits widen to
                    half = z.astype(np.float16)
                    hipmem.upload(ptr, half.view(np.uint16))
                    z = half.astype(f32)
                    rows = DeviceRows(ptr, m, P * 2, SA_ELEM_F16)
                new = np.arange(next_id, next_id + m, dtype=u64)
                next_id += m
                b.bus = 0
                if S == 1:
                    t3, want = clock(lambda: [b.track(z, new, present=pres)])
                    if device:
                        t1, got = clock(lambda: [a.track(None, new, present=pres, rows=rows)])
                    else:
                        t1, got = clock(lambda: [a.track(z, new, present=pres)])
                else:
                    zs, ps = np.split(z, S), np.split(pres, S)
                    call = [(t, zz, pp) for t, zz, pp in zip(ids, zs, ps)]
                    t3, want = clock(lambda: b.track_batch(call, new))
                    if device:
                        t1, got = clock(lambda: a.track_batch(None, new, rows=rows, track_ids=ids, pose_counts=[n] * S, present=pres))
                    else:
                        t1, got = clock(lambda: a.track_batch(call, new))
                st = a.last_track()
                assert st["vote_launches"] == 3 and st["step_launches"] == (1 if S == 1 else 2) and st["scenes"] == S
                got, want = np.concatenate(got), np.concatenate(want)
                assert (got == want).all(), "round %d: the two routes gave a pose different ids" % r
                assert a.order().tolist() == b.order().tolist(), "round %d: the two banks are in different order" % r
                born = got[np.isin(got, new)]
                assert len(born) == st["created"]
                check = a.order() if r == warm + rounds - 1 else np.concatenate([rng.choice(every, min(128, len(every)), replace=False), born])
                for t in check:
                    x, y = a.state(t), b.state(t)
                    assert (x[0] == y[0]).all() and same(x[1], y[1]) and same(x[2], y[2]), "round %d, track %d: the two routes left different states" % (r, t)
                a.remove(born)
                b.remove(born)
                if r >= warm:
                    wall_one.append(t1)
                    wall_three.append(t3)
                    bus_one.append(st["bytes_h2d"] + st["bytes_d2h"])
                    bus_three.append(b.bus)
                    for k in range(5):
                        kern[k].append(st["kernel_ms"][k] * 1e-3)
    finally:
        if device:
            eng.unregister_device_block(ptr)
            hipmem.free(ptr)
    out = {"one_call": {"wall_us": pct(wall_one), "bus_bytes": int(np.median(bus_one))},
           "three_calls": {"wall_us": pct(wall_three), "bus_bytes": int(np.median(bus_three))},
           "kernel_us": {nm: pct(kern[k]) for k, nm in enumerate(NAMES)},
           "stats": {x: v for x, v in st.items() if x not in ("device_ms", "kernel_ms", "scene_roots")}}
    out["wall_gain"] = round(out["three_calls"]["wall_us"]["median"] / out["one_call"]["wall_us"]["median"], 2)
    return {"config": "track" if S == 1 else "track_batch", "scenes": S, "poses": n, "tracks": n, "points": P, "source": "dev f16" if device else "host f32",
            "scene": "crowded" if crowd else "sparse", "rounds": rounds, "clock": "host (wall_us), device events (kernel_us)", "equal_results": True, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small cases (1 x 20, 3 x 50)")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pose_track.jsonl"))
    args = ap.parse_args()
    cases = [(1, 20), (3, 50)] if args.quick else [(1, 100), (8, 100), (64, 100), (8, 500)]
    eng = Engine(abi.make_config(device=0))
    try:
        with open(args.out, "w") as fh:
            for S, n in cases:
                for crowd in (False, True):
                    for device in (False, True):
                        text = json.dumps(config(eng, S, n, crowd, device, max(1, args.rounds)))
                        print(text, flush=True)
                        fh.write(text + "\n")
                        fh.flush()
    finally:
        eng.close()


if __name__ == "__main__":
    main()
