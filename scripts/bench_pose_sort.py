"""sa_pose_sort_predict (include/similari_pose_sort.h): the keypoint tracker — epochs, expiry, the vote, the step, the coasting — in ONE
call, against the only route there was before it: PoseTrackBank.track_batch on a twin bank in the same run and on the same frames, with
the life cycle (epochs, idle expiry through remove(), the per-scene id lists, the id counter) kept in Python, numpy arrays per scene.
One JSON line per (case, scene kind, source).

  cases    S in {1, 8, 64} scenes of 100 x 100, 8 scenes of 500 x 500; P = 17; the shapes and conventions of scripts/bench_pose_track.py
  sparse / crowded, host f32 / dev f16: as there
  life     max_idle_epochs = 1.  A fifth of a frame's poses show somebody new and are never seen again, a fifth of the people are not
           shown: every frame creates tracks and, from the third on, expires some (k_points_gather and the compaction run)
  gated    a third tracker with constraints [(1, 1.0)] is fed the same frames: k_pose_circles and the GATE tile on the same frame
           (its refusals may make it create other tracks; it is timed, not compared)

Times: wall_us is the HOST clock around each route, median [p10, p90]; kernel_us are DEVICE events around each launch of the one call.
Every round asserts that the two routes gave every pose the same id, left the same order and, bit for bit, the same states on a sample
of 128 tracks, and that the wasted states are the twin's states of the frame before.

   python scripts/bench_pose_sort.py [--quick] [--rounds N] [--out profiles/pose_sort.jsonl]"""
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
from similari_amd.pose_sort import KeypointSort  # noqa: E402
from similari_amd.pose_track import PoseTrackBank  # noqa: E402

f32, u64 = np.float32, np.uint64
P = 17
NAMES = ("k_pose_factor", "k_pose_tile", "k_pose_assign", "k_pose_scan", "k_pose_step")


def pct(v, scale=1e6):
    v = np.asarray(v, np.float64) * scale
    return {"median": round(float(np.median(v)), 1), "p10": round(float(np.quantile(v, 0.1)), 1), "p90": round(float(np.quantile(v, 0.9)), 1)}


def same(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


class PythonSort:
    """The life cycle in Python around PoseTrackBank.track_batch: per scene an epoch, the ids in creation order (ascending: the counter
    only grows) and their last epochs."""

    def __init__(self, bank, S, max_idle):
        self.bank, self.max_idle, self.next_id = bank, max_idle, 1
        self.epoch = [0] * S
        self.ids = [np.zeros(0, u64) for _ in range(S)]
        self.last = [np.zeros(0, np.int64) for _ in range(S)]

    def predict(self, poses, present):
        """-> (ids per scene, the expired ids, seconds on the host clock).  The clock stops while up to eight of the leaving tracks'
        states are read for the comparison with wasted(): the yardstick does not pay for the check."""
        t0 = time.perf_counter()
        gone = []
        for s in range(len(self.ids)):
            self.epoch[s] += 1
            idle = self.epoch[s] - self.last[s] > self.max_idle
            if idle.any():
                gone.append(self.ids[s][idle])
                self.ids[s], self.last[s] = self.ids[s][~idle], self.last[s][~idle]
        gone = np.concatenate(gone) if gone else np.zeros(0, u64)
        t1 = time.perf_counter()
        self.final = {int(t): self.bank.state(t) for t in gone[:8]}
        t2 = time.perf_counter()
        if len(gone):
            self.bank.remove(gone)
        got = self.bank.track_batch([(t, z, p) for t, z, p in zip(self.ids, poses, present)], self.next_id)
        for s, g in enumerate(got):
            new = g >= self.next_id
            at = np.searchsorted(self.ids[s], g[~new])
            self.last[s][at] = self.epoch[s]
            self.ids[s] = np.concatenate([self.ids[s], g[new]])
            self.last[s] = np.concatenate([self.last[s], np.full(int(new.sum()), self.epoch[s], np.int64)])
        self.next_id += self.bank.last_track()["created"]
        return got, gone, (t1 - t0) + (time.perf_counter() - t2)


def config(eng, S, n, crowd, device, rounds, warm=2):
    import hipmem
    import pose_ref as PR

    rng = np.random.default_rng(1000 * S + n + crowd)
    centres = [PR.people(rng, n, P, crowd, spacing=1.0, extent=float(np.sqrt(n))) + 100.0 * s for s in range(S)]
    m = S * n
    scenes = list(range(1, S + 1))
    wall_one, wall_py, kern, gate, gather, tile_gated, tracks, expired = [], [], [[] for _ in NAMES], [], [], [], [], []
    ptr = hipmem.malloc(m * P * 2 * 2) if device else None
    try:
        if device:
            eng.register_device_block(ptr, m * P * 2 * 2, 0)
        with KeypointSort(eng, P, max_idle_epochs=1) as a, PoseTrackBank(eng, P) as twin, KeypointSort(eng, P, max_idle_epochs=1, constraints=[(1, 1.0)]) as g:
            b = PythonSort(twin, S, 1)
            for r in range(2 + warm + rounds):   # two frames fill the banks; the clocks start behind the warm-up
                frame = [PR.poses_of(rng, c, n) for c in centres]
                if r == 0:
                    frame = [((c + rng.normal(0, 0.03, c.shape)).astype(f32), np.ones((n, P), bool)) for c in centres]
                z, pres = np.concatenate([f[0] for f in frame]), np.concatenate([f[1] for f in frame])
                kw = {}
                if device:   # the network's output: f16 in device memory; the twin gets what those bits widen to
                    half = z.astype(np.float16)
                    hipmem.upload(ptr, half.view(np.uint16))
                    z = half.astype(f32)
                    kw = dict(rows=DeviceRows(ptr, m, P * 2, SA_ELEM_F16), pose_counts=[n] * S, present=pres)
                zs, ps = np.split(z, S), np.split(pres, S)
                want, gone, t_py = b.predict(zs, ps)
                t = time.perf_counter()
                got = a.predict(scenes, **kw) if device else a.predict({s: (x, y) for s, x, y in zip(scenes, zs, ps)})
                t_one = time.perf_counter() - t
                st = a.last()
                g.predict(scenes, **kw) if device else g.predict({s: (x, y) for s, x, y in zip(scenes, zs, ps)})
                sg = g.last()
                assert all((got[s]["id"] == w).all() for s, w in zip(scenes, want)), "round %d: the two routes gave a pose different ids" % r
                bank = a.bank()
                assert bank.order().tolist() == twin.order().tolist(), "round %d: the two banks are in different order" % r
                order = bank.order()
                for t_ in rng.choice(order, min(128, len(order)), replace=False):
                    x, y = bank.state(t_), twin.state(t_)
                    assert (x[0] == y[0]).all() and same(x[1], y[1]) and same(x[2], y[2]), "round %d, track %d: different states" % (r, t_)
                ws = a.wasted()
                assert [w.id for w in ws] == gone.tolist() and st["expired"] == len(gone)
                for w in ws[:8]:
                    y = b.final[w.id]
                    assert (w.has == y[0]).all() and same(w.mean, y[1]) and same(w.cov, y[2]), "round %d: a wasted state differs" % r
                g.wasted()
                if r >= 2 + warm:
                    assert st["vote_launches"] == 3 and st["gate_launches"] == 0 and sg["gate_launches"] == 1
                    wall_one.append(t_one)
                    wall_py.append(t_py)
                    for k in range(5):
                        kern[k].append(st["kernel_ms"][k] * 1e-3)
                    gather.append(st["gather_ms"] * 1e-3)
                    gate.append(sg["gate_ms"] * 1e-3)
                    tile_gated.append(sg["kernel_ms"][1] * 1e-3)
                    tracks.append(st["tracks"])
                    expired.append(st["expired"])
    finally:
        if device:
            eng.unregister_device_block(ptr)
            hipmem.free(ptr)
    out = {"one_call": {"wall_us": pct(wall_one)}, "python_life_cycle": {"wall_us": pct(wall_py)},
           "kernel_us": {**{nm: pct(kern[k]) for k, nm in enumerate(NAMES)}, "k_points_gather": pct(gather), "k_pose_circles": pct(gate),
                         "k_pose_tile_gated": pct(tile_gated)},
           "tracks": int(np.median(tracks)), "expired": int(np.median(expired)),
           "stats": {x: v for x, v in st.items() if x not in ("device_ms", "kernel_ms", "gate_ms", "gather_ms")}}
    out["wall_gain"] = round(out["python_life_cycle"]["wall_us"]["median"] / out["one_call"]["wall_us"]["median"], 2)
    return {"config": "pose_sort", "scenes": S, "poses": n, "people": n, "points": P, "source": "dev f16" if device else "host f32",
            "scene": "crowded" if crowd else "sparse", "rounds": rounds, "clock": "host (wall_us), device events (kernel_us)", "equal_results": True, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small cases (1 x 20, 3 x 50)")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pose_sort.jsonl"))
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
