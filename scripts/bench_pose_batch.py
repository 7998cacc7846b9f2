"""sa_points_associate_batch (include/similari_pose_batch.h): the poses of S scenes against the tracks of one point bank in ONE call of
three launches, against the only route there was before it: S calls of sa_points_associate, one per scene, on the same bank in the same
run.  One JSON line per (case, scene kind).

  cases    S in {1, 8, 64} scenes of 100 x 100, 8 scenes of 500 x 500; P = 17, the poses come from host memory as f32
  sparse   people a gate apart and more: every pose keeps its greedy bid, the dense search has no root
  crowded  people in clusters tighter than the gate: several poses want one track, the dense search runs

Times: wall_us is the HOST clock around the Python wrapper — around the one batch call, and around the loop of the S single calls —,
median [p10, p90]; kernel_us are the three launches of the batch call (k_pose_factor, k_pose_tile, k_pose_assign), each from
DEVICE events around its launch; singles_kernel_us are the same three summed over the S single calls of the round.  Every round asserts
that each scene's matches and weights are equal in the two routes.

   python scripts/bench_pose_batch.py [--quick] [--rounds N] [--out profiles/pose_batch.jsonl]"""
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
from similari_amd.engine import Engine  # noqa: E402
from similari_amd.pose import PoseBank  # noqa: E402

f32, u64 = np.float32, np.uint64
P = 17


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


def config(eng, S, n, crowd, rounds, warm=2):
    import pose_ref as PR

    rng = np.random.default_rng(1000 * S + n + crowd)
    ids = [np.arange(1, n + 1, dtype=u64) + u64(s * n) for s in range(S)]
    centres = [PR.people(rng, n, P, crowd, spacing=1.0, extent=float(np.sqrt(n))) for _ in range(S)]   # the scale of bench_pose.py
    shown = PR.track_rounds(rng, np.concatenate(centres))
    wall_b, wall_s, kern_b, kern_s = [], [], [[], [], []], [[], [], []]
    with PoseBank(eng, P) as bank:
        for z, pres in shown:
            bank.step(np.concatenate(ids), z, present=pres)
        for r in range(warm + rounds):
            frame = [PR.poses_of(rng, c, n) for c in centres]
            call = [(t, z, pres) for t, (z, pres) in zip(ids, frame)]
            tb, got = clock(lambda: bank.associate_batch(call))
            st = bank.last_associate_batch()
            assert st["launches"] == 3 and st["scenes"] == S

            def singles():
                out, ms, roots = [], [0.0, 0.0, 0.0], 0
                for t, z, pres in call:
                    out.append(bank.associate(z, present=pres, ids=t))
                    one = bank.last_associate()
                    roots += one["roots"]
                    for k in range(3):
                        ms[k] += one["kernel_ms"][k]
                return out, ms, roots

            ts, (ref, ms, roots) = clock(singles)
            for s in range(S):
                assert (got[s][0] == ref[s][0]).all() and same(got[s][1], ref[s][1]), "round %d, scene %d: the two routes differ" % (r, s)
            assert roots == st["roots"]
            if r >= warm:
                wall_b.append(tb)
                wall_s.append(ts)
                for k in range(3):
                    kern_b[k].append(st["kernel_ms"][k] * 1e-3)
                    kern_s[k].append(ms[k] * 1e-3)
    names = ("k_pose_factor", "k_pose_tile", "k_pose_assign")
    out = {"batch": {"wall_us": pct(wall_b)}, "singles": {"wall_us": pct(wall_s)},
           "kernel_us": {nm: pct(kern_b[k]) for k, nm in enumerate(names)}, "singles_kernel_us": {nm: pct(kern_s[k]) for k, nm in enumerate(names)},
           "roots": st["roots"], "matched": st["matched"], "stats": {x: v for x, v in st.items() if x not in ("device_ms", "kernel_ms", "scene_roots")}}
    out["wall_gain"] = round(out["singles"]["wall_us"]["median"] / out["batch"]["wall_us"]["median"], 2)
    return {"config": "associate_batch", "scenes": S, "poses": n, "tracks": n, "points": P, "source": "host f32", "scene": "crowded" if crowd else "sparse",
            "rounds": rounds, "clock": "host (wall_us), device events (kernel_us)", "equal_results": True, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small cases (2 x 20, 3 x 50)")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pose_batch.jsonl"))
    args = ap.parse_args()
    cases = [(2, 20), (3, 50)] if args.quick else [(1, 100), (8, 100), (64, 100), (8, 500)]
    eng = Engine(abi.make_config(device=0))
    try:
        with open(args.out, "w") as fh:
            for S, n in cases:
                for crowd in (False, True):
                    text = json.dumps(config(eng, S, n, crowd, max(1, args.rounds)))
                    print(text, flush=True)
                    fh.write(text + "\n")
                    fh.flush()
    finally:
        eng.close()


if __name__ == "__main__":
    main()
