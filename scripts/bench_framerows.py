"""A frame's feature rows read from device memory (include/similari_framerows.h) against what a caller does today, on one C2-sized
frame — 1000 detections x 1000 tracks, 512-d cosine + IoU(0.3), K = 1 — in one process, one JSON line per route:

  a   f32 rows in a registered device block, read in place: the best case the engine had before (no pass over the rows at all)
  b   the fp16 [1000, 512] output of a ReID head through sa_batch_add_dev: one widen launch behind the upload
  c   what a caller holding that fp16 tensor does without it: cast into a registered f32 buffer with the framework (one casting
      copy_, the cheapest form of tensor.float() into a buffer that is registered once), torch.cuda.synchronize(), then route a
  d   like b out of a [1024, 640] fp16 batch: a column slice (64 .. 576) and a permuted row index

All four routes see the same values (a reads widen(x) of the fp16 tensor), so ids and votes are compared bit for bit every round.
The routes alternate, 7 rounds after a warm-up of each; every round stages the frame anew (sa_batch_begin .. sa_batch_fetch), so the
upload is inside the clock.  Times are HOST-clock microseconds around synchronous calls that end in a synchronisation, median [p10, p90].
The widen launch's own duration comes from the engine's profile mode (the dispatch's begin / end timestamps) in extra rounds that are
not clocked.  The requirement: b's median <= c's median + c's own p10 - p90 spread.
   python scripts/bench_framerows.py [--rounds N] [--out profiles/framerows.jsonl]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
torch.zeros(1, device="cuda:0")   # torch's context first, as in a process that runs its ReID model before the tracker
from similari_amd import abi, framerows as FR, synth  # noqa: E402
from similari_amd.devrows import DeviceRows, register_tensor  # noqa: E402
from similari_amd.engine import Engine  # noqa: E402

N = T = 1000
D = 512
SCENE = 1


def pct(v):
    v = np.asarray(v, np.float64) * 1e6
    return {"median": round(float(np.median(v)), 1), "p10": round(float(np.quantile(v, 0.1)), 1), "p90": round(float(np.quantile(v, 0.9)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "framerows.jsonl"))
    args = ap.parse_args()
    rounds = max(1, args.rounds)
    rng = np.random.default_rng(0)
    sc = synth.visual_scene(rng, T, N, D, 1)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=D, max_observations=1,
                          visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1, max_idle_epochs=5, device=0)
    eng = Engine(cfg)
    try:
        eng.upsert(SCENE, abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"], feat_present=sc["track_present"]))
        t16 = torch.from_numpy(sc["det_feats"]).to("cuda:0").half().contiguous()          # the ReID head's output
        f32 = t16.float().contiguous()                                                   # route a: the same values as f32
        buf = torch.empty_like(f32)                                                      # route c: the caller's registered f32 buffer
        batch = torch.full((1024, 640), float("nan"), dtype=torch.float16, device="cuda:0")
        perm = torch.from_numpy(rng.permutation(1024)[:N].astype(np.int64)).to("cuda:0")
        batch[perm, 64:64 + D] = t16
        index = perm.cpu().numpy().astype(np.uint32)
        torch.cuda.synchronize()
        q = sc["det_quality"]
        bare = abi.make_detections(sc["det_boxes"], feat_quality=q)
        with register_tensor(eng, t16), register_tensor(eng, f32), register_tensor(eng, buf), register_tensor(eng, batch):
            det_a = abi.make_detections(sc["det_boxes"], feat_quality=q, feats_device_ptr=f32.data_ptr())
            det_c = abi.make_detections(sc["det_boxes"], feat_quality=q, feats_device_ptr=buf.data_ptr())
            rows_b = DeviceRows.from_tensor(t16)
            rows_d = DeviceRows.from_tensor(batch[:, 64:64 + D], index=index)

            def frame(det, rows=None):
                eng.batch_begin()
                slot = eng.batch_add(SCENE, 1, det) if rows is None else FR.batch_add_rows(eng, SCENE, 1, det, rows)
                eng.batch_run()
                eng.batch_sync()
                return eng.batch_fetch(slot, N)

            def route_c():
                buf.copy_(t16)
                torch.cuda.synchronize()
                return frame(det_c)

            calls = {"a_f32_in_place": lambda: frame(det_a), "b_f16_rows": lambda: frame(bare, rows_b), "c_cast_then_pointer": route_c,
                     "d_f16_slice_gather": lambda: frame(bare, rows_d)}
            want = None
            for fn in calls.values():   # warm-up: buffers, code objects
                for _ in range(2):
                    out = fn()
                want = out if want is None else want
            wall = {k: [] for k in calls}
            for _ in range(rounds):
                for k, fn in calls.items():
                    t0 = time.perf_counter()
                    ids, votes = fn()
                    wall[k].append(time.perf_counter() - t0)
                    assert np.array_equal(ids, want[0]) and np.array_equal(votes, want[1]), "route %s differs" % k
            assert (want[1] == abi.SA_VOTE_VISUAL).sum() > N // 2
            stats, widen = {}, {}
            eng.profile_enable(True)
            for k, rows in (("b_f16_rows", rows_b), ("d_f16_slice_gather", rows_d)):
                eng.profile_reset()
                for _ in range(rounds):
                    frame(bare, rows)
                n, ms = eng.profile_read()["k_widen_rows"]
                widen[k] = {"launches": int(n), "mean_us": round(ms * 1e3 / n, 2)}
                stats[k] = FR.framerows_stats(eng)
            eng.profile_enable(False)
        lines = []
        for k in calls:
            line = {"config": "c2_frame", "route": k, "detections": N, "tracks": T, "D": D, "rounds": rounds, "wall_us": pct(wall[k]), "same_ids_and_votes": True}
            if k in widen:
                line["widen_launch"] = widen[k]
                line["framerows"] = stats[k]
            lines.append(line)
        b, c = (next(l for l in lines if l["route"].startswith(p))["wall_us"] for p in ("b_", "c_"))
        bound = c["median"] + (c["p90"] - c["p10"])
        lines.append({"config": "c2_frame", "requirement": "b median <= c median + c's p10-p90 spread", "b_median_us": b["median"],
                      "c_median_us": c["median"], "c_spread_us": round(c["p90"] - c["p10"], 1), "bound_us": round(bound, 1), "met": bool(b["median"] <= bound)})
        with open(args.out, "w") as fh:
            for line in lines:
                text = json.dumps(line)
                print(text, flush=True)
                fh.write(text + "\n")
    finally:
        eng.close()


if __name__ == "__main__":
    main()
