"""The OKS metric (include/similari_pose_oks.h) against the Mahalanobis metric — the path there was before it, unchanged — on the same
frames in the same run: two keypoint trackers, one per metric, are fed every frame; each frame is first asked as a vote alone
(sa_pose_sort_peek: extents, factor, tile, assign) and then run (sa_pose_sort_predict: the vote, the step, the coasting).  One JSON line
per (case, scene kind).

  cases    S in {1, 8, 64} scenes of 100 x 100, 8 scenes of 500 x 500; P = 17, COCO's sigmas; host f32 poses; the shapes and conventions
           of scripts/bench_pose_sort.py
  sparse / crowded: as there (pose_ref.people)
  life     max_idle_epochs = 1, a fifth of a frame's poses show somebody new: every frame creates tracks and expires some
  threshold  1.0 for the Mahalanobis tracker, 0.3 for the OKS tracker: each metric's default.  The two trackers therefore hold different
           tracks after a few frames (the numbers are reported, with the assignment's search roots: the rows that lost their greedy
           bid); they are timed, not compared — tests/test_gpu_oks.py compares

Times: wall_us is the HOST clock around each call, median [p10, p90]; kernel_us are DEVICE events around each launch.  Under the
Mahalanobis metric without a limit there is no extents launch (k_pose_circles: null).  No ratio is asserted: the lines say what the in-loop
division and the polynomial cost in the tile, in whichever direction.

   python scripts/bench_pose_oks.py [--quick] [--rounds N] [--out profiles/pose_oks.jsonl]"""
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
from similari_amd.pose_oks import COCO_SIGMAS, OksMetric  # noqa: E402
from similari_amd.pose_sort import KeypointSort  # noqa: E402

f32 = np.float32
P = 17
VOTE = ("k_pose_circles", "k_pose_factor", "k_pose_tile", "k_pose_assign")
STEP = ("k_pose_scan", "k_pose_step")


def pct(v, scale=1e6):
    v = np.asarray(v, np.float64) * scale
    return {"median": round(float(np.median(v)), 1), "p10": round(float(np.quantile(v, 0.1)), 1), "p90": round(float(np.quantile(v, 0.9)), 1)}


class Clock:
    def __init__(self):
        self.peek_wall, self.frame_wall = [], []
        self.vote = {k: [] for k in VOTE}
        self.frame = {k: [] for k in VOTE + STEP}
        self.tracks, self.matched, self.roots, self.gate = [], [], [], []

    def peek(self, st, wall):
        self.peek_wall.append(wall)
        self.gate.append(st["gate_launches"])
        self.vote["k_pose_circles"].append(st["gate_ms"] * 1e-3)
        for k in range(3):
            self.vote[VOTE[1 + k]].append(st["kernel_ms"][k] * 1e-3)

    def predict(self, st, wall):
        self.frame_wall.append(wall)
        self.tracks.append(st["tracks"])
        self.matched.append(st["matched"])
        self.roots.append(st["roots"])
        self.frame["k_pose_circles"].append(st["gate_ms"] * 1e-3)
        for k, nm in enumerate(VOTE[1:] + STEP):
            self.frame[nm].append(st["kernel_ms"][k] * 1e-3)

    def report(self):
        extents = bool(np.median(self.gate))
        kern = lambda d: {nm: (pct(v) if nm != "k_pose_circles" or extents else None) for nm, v in d.items()}  # noqa: E731
        vote_sum = np.sum([self.vote[nm] for nm in VOTE], 0)
        return {"vote": {"wall_us": pct(self.peek_wall), "kernel_us": kern(self.vote), "kernels_sum_us": pct(vote_sum)},
                "frame": {"wall_us": pct(self.frame_wall), "kernel_us": kern(self.frame)},
                "tracks": int(np.median(self.tracks)), "matched": int(np.median(self.matched)), "roots": int(np.median(self.roots)),
                "extents_launches": int(extents)}


def config(eng, S, n, crowd, rounds, warm=2):
    import pose_ref as PR

    rng = np.random.default_rng(1000 * S + n + crowd)
    centres = [PR.people(rng, n, P, crowd, spacing=1.0, extent=float(np.sqrt(n))) + 100.0 * s for s in range(S)]
    scenes = list(range(1, S + 1))
    clocks = {"mahalanobis": Clock(), "oks": Clock()}
    with KeypointSort(eng, P, max_idle_epochs=1) as a, KeypointSort(eng, P, max_idle_epochs=1, metric=OksMetric(COCO_SIGMAS)) as b:
        trackers = {"mahalanobis": a, "oks": b}
        for r in range(2 + warm + rounds):   # two frames fill the banks; the clocks start behind the warm-up
            frame = [PR.poses_of(rng, c, n) for c in centres]
            if r == 0:
                frame = [((c + rng.normal(0, 0.03, c.shape)).astype(f32), np.ones((n, P), bool)) for c in centres]
            call = {s: f for s, f in zip(scenes, frame)}
            for name, trk in trackers.items():
                t = time.perf_counter()
                trk.peek(call)
                t_peek = time.perf_counter() - t
                sp = trk.last()
                t = time.perf_counter()
                trk.predict(call)
                t_frame = time.perf_counter() - t
                sf = trk.last()
                trk.wasted()
                if r >= 2 + warm:
                    assert sp["vote_launches"] == 3 and sp["gate_launches"] == sf["gate_launches"] == (1 if name == "oks" else 0)
                    clocks[name].peek(sp, t_peek)
                    clocks[name].predict(sf, t_frame)
    out = {name: c.report() for name, c in clocks.items()}
    ratio = lambda part, key: round(out["oks"][part][key]["median"] / max(out["mahalanobis"][part][key]["median"], 1e-9), 3)  # noqa: E731
    out["oks_over_mahalanobis"] = {"vote_kernels_sum": ratio("vote", "kernels_sum_us"), "vote_wall": ratio("vote", "wall_us"), "frame_wall": ratio("frame", "wall_us"),
                                   "tile": round(out["oks"]["vote"]["kernel_us"]["k_pose_tile"]["median"]
                                                 / max(out["mahalanobis"]["vote"]["kernel_us"]["k_pose_tile"]["median"], 1e-9), 3)}
    return {"config": "pose_oks", "scenes": S, "poses": n, "people": n, "points": P, "source": "host f32", "scene": "crowded" if crowd else "sparse",
            "rounds": rounds, "clock": "host (wall_us), device events (kernel_us)", **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small cases (1 x 20, 3 x 50)")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pose_oks.jsonl"))
    args = ap.parse_args()
    cases = [(1, 20), (3, 50)] if args.quick else [(1, 100), (8, 100), (64, 100), (8, 500)]
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
