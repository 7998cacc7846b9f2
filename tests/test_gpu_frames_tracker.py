"""The tracker facade computes the own-area shares of a request set in ONE sa_own_areas_batch call (include/similari_frames.h):
a BatchVisualSort whose own-area gates are armed and which gets no shares behaves, frame by frame, like its twin that is handed the
shares of per-scene Engine.own_areas calls made on another engine; a share the caller supplies still wins over the computed one."""
import numpy as np
import pytest

from similari_amd import abi, frames, synth
from similari_amd import trackers as T
from similari_amd.engine import Engine

pytestmark = pytest.mark.gpu
D = 16
SIZES = {0: 3, 1: 17, 2: 40, 3: 64, 4: 70}   # scene id -> objects


def tracker(device_upkeep):
    opts = (T.VisualSortOptions().max_idle_epochs(2).kept_history_length(3).visual_metric(T.VisualSortMetricType.cosine(0.5))
            .positional_metric(T.PositionalMetricType.iou(0.3)).visual_minimal_track_length(2).visual_minimal_area(500.0)
            .visual_minimal_quality_use(0.4).visual_minimal_quality_collect(0.6).visual_max_observations(3).visual_min_votes(1)
            .visual_minimal_own_area_percentage_use(0.55).visual_minimal_own_area_percentage_collect(0.7))
    return T.BatchVisualSort(opts=opts, feature_len=D, device_upkeep=device_upkeep)


def u2d(boxes):
    return [T.Universal2DBox(float(b["xc"]), float(b["yc"]), float(b["angle"]) if b["has_angle"] else None, float(b["aspect"]),
                             float(b["height"]), float(b["confidence"])) for b in boxes]


def predict(trk, worlds, feats, shares):
    """One frame of every scene; shares: scene -> per-observation share or None.  -> scene -> [SortTrack]"""
    req = T.PredictionBatchRequest()
    for s, w in worlds.items():
        for i, (bx, ft) in enumerate(zip(u2d(w), feats[s])):
            req.add(s, T.VisualSortObservation(ft, 0.9, bx, None, own_area=None if shares is None else shares[s][i]))
    return trk.predict(req)


def engine_of(trk):
    return Engine.borrowed(trk.lib, trk.lib.sa_tracker_engine(trk.h))


@pytest.mark.parametrize("device_upkeep", [False, True], ids=["host_upkeep", "device_upkeep"])
def test_gated_batch_tracker_equals_its_twin_with_supplied_shares(device_upkeep):
    rng = np.random.default_rng(61)
    a, b = tracker(device_upkeep), tracker(device_upkeep)
    other = Engine(abi.make_config())
    try:
        ident = {s: synth.reid_identities(rng, n, D) for s, n in SIZES.items()}
        worlds = {s: synth.dense_boxes(rng, n, (900.0, 700.0), oriented=bool(s & 1)) for s, n in SIZES.items()}
        gated = 0
        for f in range(6):
            worlds = {s: synth.jitter_boxes(rng, w, 2.0) for s, w in worlds.items()}
            if f == 3:   # some objects leave: their tracks end up wasted
                worlds = {s: w[: max(2, len(w) - 2)] for s, w in worlds.items()}
                ident = {s: i[: len(worlds[s])] for s, i in ident.items()}
            feats = {s: synth.observe(rng, ident[s], 0.01) for s in SIZES}
            shares = {s: [float(x) for x in other.own_areas(w)] for s, w in worlds.items()}
            gated += sum(x < 0.7 for sh in shares.values() for x in sh)
            ra = predict(a, worlds, feats, None)
            if f == 0:   # the facade took the batch route: one call for the five scenes
                st = frames.last_stats(engine_of(a))
                assert st["scenes"] == 5 and st["boxes"] == sum(SIZES.values()) and st["launches"] == 1 and st["host_waits"] == 1
            rb = predict(b, worlds, feats, shares)
            assert frames.last_stats(engine_of(b))["scenes"] == 0   # (every share supplied: nothing to compute)
            assert ra.keys() == rb.keys()
            for s in SIZES:
                assert ra[s] == rb[s], (f, s)   # ids, epochs, boxes, vote outcomes
            assert a.wasted() == b.wasted(), f
        assert gated > 20, "the gates must have something to bite on"
    finally:
        a.close(), b.close(), other.close()


def test_a_supplied_share_wins_over_the_computed_one():
    """One scene; every second observation carries a caller-supplied share, among them a deliberately wrong one: 0.0 on an isolated
    box (its true share is 1).  Tracker A gets those and computes the rest; its twin B gets every share spelled out — the supplied
    ones and, for the others, the per-scene call's.  Tracker C gets none: there the isolated box's features are collected."""
    rng = np.random.default_rng(62)
    n = 30
    a, b, c = tracker(False), tracker(False), tracker(False)
    other = Engine(abi.make_config())
    try:
        ident = synth.reid_identities(rng, n, D)
        world = synth.dense_boxes(rng, n, (900.0, 700.0))
        world[0]["xc"], world[0]["yc"] = 5000.0, 5000.0   # the isolated box
        for f in range(5):
            world = synth.jitter_boxes(rng, world, 2.0)
            feats = {0: synth.observe(rng, ident, 0.01)}
            true = [float(x) for x in other.own_areas(world)]
            assert true[0] > 0.999
            full = list(true)
            full[0] = 0.0
            half = [full[i] if i % 2 == 0 else None for i in range(n)]
            ra = predict(a, {0: world}, feats, {0: half})
            st = frames.last_stats(engine_of(a))
            assert st["scenes"] == 1 and st["boxes"] == n   # (the missing half made the facade compute the scene's shares)
            rb = predict(b, {0: world}, feats, {0: full})
            rc = predict(c, {0: world}, feats, None)
            assert ra[0] == rb[0], f
        collected = [t.track_info(r[0][0].id)["visual_features_collected_count"] for t, r in ((a, ra), (b, rb), (c, rc))]
        assert collected[0] == collected[1] < collected[2], collected
    finally:
        a.close(), b.close(), c.close(), other.close()
