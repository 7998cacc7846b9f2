"""The lazy first phase's contraction tile with helper waves (k_frame_visual's HELP form, sa_gemm.hip: visual_tile_helped).  A forced-lazy
frame runs it; a forced-eager frame runs the one-wave tile beside the positional tiles.  Both reduce the same cells into the vote words, so
the words must agree bit for bit, and both frames must give the oracle's ids and vote types (the words also under check_votes)."""
import numpy as np
import pytest

import oracle_lib as O
from similari_amd import abi, synth
from similari_amd.engine import Engine
import test_gpu_parity as P

pytestmark = pytest.mark.gpu
EAGER, LAZY = abi.SA_FLAG_EAGER_POSITIONAL, abi.SA_FLAG_LAZY_POSITIONAL


def config(d, **kw):
    base = dict(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=d, max_observations=1,
                visual_min_votes=1, visual_minimal_track_length=1, visual_minimal_quality_use=0.5, positional_min_confidence=0.1,
                max_idle_epochs=5)
    base.update(kw)
    return lambda: abi.make_config(**base)


def scene(seed, n, t, d=32):
    """About 15 % new objects and 15 % of the detections under the quality gate; the canvas grows with the frame."""
    rng = np.random.default_rng(seed)
    s = np.sqrt(max(n, t, 1) / 1000.0)
    sc = synth.visual_scene(rng, t, n, d, 1, canvas=(1920.0 * s, 1080.0 * s), new_fraction=0.15)
    sc["det_quality"][rng.uniform(size=n) < 0.15] = 0.3
    return sc


def tracks_of(sc):
    return abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"], feat_present=sc["track_present"])


def dets_of(sc):
    return abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"], own_area=sc.get("own_area"),
                               feat_present=sc.get("det_present"))


def frames_in_mode(make_cfg, sc, frames, mode):
    """Tapped frames of one engine in `mode`: [(ids, votes, tap_votes)] per (epoch, detection scene) of `frames`, each held to the oracle."""
    cfg = make_cfg()
    cfg.flags |= abi.SA_FLAG_TAP | P.POS_MODE_FLAGS[mode]
    tracks = tracks_of(sc)
    out = []
    eng = Engine(cfg)
    try:
        eng.upsert(0, tracks)
        for epoch, dsc in frames:
            det = dets_of(dsc)
            assert P.mode_of(cfg, det.n, tracks.n) == mode
            ref = O.associate(make_cfg(), tracks, epoch, det)
            ids, votes = eng.associate(0, epoch, det)
            np.testing.assert_array_equal(ids, ref["track_id"], err_msg=f"{mode} epoch {epoch}")
            np.testing.assert_array_equal(votes, ref["voting_type"], err_msg=f"{mode} epoch {epoch}")
            P.check_votes(cfg, eng, ref["visual"])
            out.append((ids, votes, eng.tap_votes(0)))
    finally:
        eng.close()
    return out


def same_words(make_cfg, sc, frames=None):
    """The lazy frames' vote words == the eager frames' bit for bit.  Returns the lazy frames' (ids, votes, tap_votes)."""
    frames = frames or [(1, sc)]
    lazy, eager = frames_in_mode(make_cfg, sc, frames, "lazy"), frames_in_mode(make_cfg, sc, frames, "eager")
    for f, (a, b) in enumerate(zip(lazy, eager)):
        for name, x, y in zip(("row weight", "row index", "column weight", "column index", "kind"), a[2], b[2]):
            np.testing.assert_array_equal(x, y, err_msg=f"frame {f}: {name}")
    return lazy


SIZES = [1, 33, 63, 64, 65, 127, 1000, 1024]
SHAPES = [(n, t) for n in SIZES for t in SIZES if n in (1, 64, 1024) or t in (1, 64, 1024) or n == t]


@pytest.mark.parametrize("n,t", SHAPES, ids=[f"{n}x{t}" for n, t in SHAPES])
def test_edge_tiles(n, t):
    same_words(config(32), scene(4000 + 7 * n + t, n, t))


def test_ties_within_rows_and_columns():
    """Duplicated track features (equal keys along a row: the lowest column wins) and duplicated candidates (equal keys down a column: the
    lowest row wins), inside one tile and across tiles."""
    n, t = 300, 280
    sc = scene(4100, n, t)
    for j1, j2 in ((3, 4), (5, 70), (10, 200), (64, 127)):
        sc["track_feats"][j2] = sc["track_feats"][j1]
    for i1, i2 in ((2, 3), (7, 90), (20, 257), (63, 64)):
        sc["det_feats"][i2] = sc["det_feats"][i1]
        sc["det_quality"][i1] = sc["det_quality"][i2] = 0.9
    (ids, votes, (rw, ri, cw, ci, _)), = same_words(config(32), sc)
    # the ties are there: a duplicated track shares its row weights with its twin, and a duplicated candidate its column weights
    tied_rows = [i for i in range(n) if ri[i] in (3, 5, 10, 64)]
    tied_cols = [j for j in range(t) if ci[j] in (2, 7, 20, 63)]
    assert tied_rows and tied_cols


def test_unusable_candidates():
    """No feature, a quality under the gate, an own area under the limit, a box under the area gate."""
    n, t = 400, 380
    rng = np.random.default_rng(4200)
    sc = scene(4200, n, t)
    sc["det_present"] = (rng.uniform(size=n) > 0.1).astype(np.uint8)
    own = rng.uniform(0.2, 1.0, n).astype(np.float32)
    own[::7] = np.nan
    sc["own_area"] = own
    sc["det_boxes"]["height"][rng.uniform(size=n) < 0.1] = 12.0
    (ids, votes, (rw, ri, cw, ci, _)), = same_words(config(32, visual_minimal_own_area_percentage_use=0.5, visual_minimal_area=400.0), sc)
    assert (ri < 0).sum() > 0.2 * n and (ri >= 0).sum() > 0.3 * n


def test_columns_failing_each_gate():
    """Tracks without a feature, tracks idle beyond max_idle_epochs, and (a frame of its own) a minimal track length no track reaches."""
    n, t = 350, 400
    rng = np.random.default_rng(4300)
    sc = scene(4300, n, t)
    sc["track_present"][rng.uniform(size=t) < 0.15] = 0
    sc["track_epochs"] = rng.integers(0, 9, t).astype(np.uint64)   # frame epoch 8: idle 0 .. 8 epochs, beyond 5 the column fails
    (_, _, (_, _, cw, ci, _)), = same_words(config(32), sc, frames=[(8, sc)])
    assert (ci < 0).sum() > 0.3 * t and (ci >= 0).sum() > 0.3 * t
    (_, votes, (_, ri, _, ci, _)), = same_words(config(32, visual_minimal_track_length=2), sc, frames=[(8, sc)])
    assert (ri < 0).all() and (ci < 0).all() and (votes == abi.SA_VOTE_POSITIONAL).sum() > 0


def test_spatio_temporal_constraints():
    n, t = 500, 560
    rng = np.random.default_rng(4400)
    sc = scene(4400, n, t)
    sc["track_epochs"] = rng.integers(3, 9, t).astype(np.uint64)
    same_words(config(32, positional_threshold=0.2, constraints=[(1, 0.3), (3, 1.0), (6, 2.0)]), sc, frames=[(8, sc)])


def test_back_to_back_frames():
    """Two frames on one engine (different detections, then the first ones again): the tail re-arms the vote words for the next frame."""
    sc = scene(4500, 600, 640, d=64)
    other = scene(4501, 600, 640, d=64)
    other.update({k: sc[k] for k in ("track_ids", "track_boxes", "track_epochs", "track_feats", "track_present")})
    same_words(config(64), sc, frames=[(1, sc), (2, other), (3, sc)])


@pytest.mark.parametrize("graph", [0, abi.SA_FLAG_GRAPH], ids=["eager_launches", "graph"])
def test_request_set_of_several_scenes(graph):
    """One request set (blockIdx.z = scene), ragged sizes: every slot's vote words lazy == eager, ids and vote types against the oracle."""
    shapes = [(1000, 1000), (33, 127), (64, 65), (1024, 1024), (1, 1)]
    scs = [scene(4600 + s, n, t) for s, (n, t) in enumerate(shapes)]
    trs = [abi.make_tracks(sc["track_ids"] + 10000 * s, sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"],
                           feat_present=sc["track_present"]) for s, sc in enumerate(scs)]
    dets = [dets_of(sc) for sc in scs]
    make_cfg = config(32)
    refs = [O.associate(make_cfg(), trs[s], 1, dets[s]) for s in range(len(scs))]
    words = {}
    for mode in ("lazy", "eager"):
        cfg = make_cfg()
        cfg.flags |= abi.SA_FLAG_TAP | P.POS_MODE_FLAGS[mode] | graph
        eng = Engine(cfg)
        try:
            for s in range(len(scs)):
                eng.upsert(500 + s, trs[s])
            for rep in range(2):
                eng.batch_begin()
                slots = [eng.batch_add(500 + s, 1, dets[s]) for s in range(len(scs))]
                eng.batch_run()
                eng.batch_sync()
                for s in range(len(scs)):
                    ids, votes = eng.batch_fetch(slots[s], dets[s].n)
                    np.testing.assert_array_equal(ids, refs[s]["track_id"], err_msg=f"{mode} scene {s} run {rep}")
                    np.testing.assert_array_equal(votes, refs[s]["voting_type"], err_msg=f"{mode} scene {s} run {rep}")
                    P.check_votes(cfg, eng, refs[s]["visual"], slot=slots[s])
                    words[mode, s, rep] = eng.tap_votes(slots[s])
        finally:
            eng.close()
    for key in [k for k in words if k[0] == "lazy"]:
        for x, y in zip(words[key], words[("eager",) + key[1:]]):
            np.testing.assert_array_equal(x, y, err_msg=str(key))
