"""A lazy VisualSORT frame in ONE launch (k_frame_visual's HELP + TAIL form, sa_gemm.hip): the scene's last-arriving block runs the
one-workgroup tail behind its tile.  Every case runs twice, forced lazy, on engines that ask for the form (SA_FLAG_ONE_LAUNCH): as they
are, and with SA_FLAG_SEPARATE_TAIL on top (the tail as a launch of its own).  Both must give the oracle's ids and vote types, the same tapped vote words bit for bit, and the
launch counts the plan promises: one against two wherever the set brings at most one block per compute unit."""
import numpy as np
import pytest

import oracle_lib as O
from similari_amd import abi, synth
from similari_amd.engine import Engine
import test_gpu_parity as P
import test_lazy_positional as L
import test_lazy_vote_tile as V

pytestmark = pytest.mark.gpu
SEPARATE = abi.SA_FLAG_SEPARATE_TAIL
D = 32
make_cfg = V.config(D)
_refs = {}


def blocks_of(shapes):
    """Blocks of the helped launch: the 64 x 64 tiles of the widest scene rounded up to the eight XCD chunks, per scene."""
    tiles = -(-max(n for n, _ in shapes) // 64) * -(-max(t for _, t in shapes) // 64)
    return 8 * -(-tiles // 8) * len(shapes)


def launches(eng, shapes, separate):
    """What the plan promises on the engine's device: one launch where the set brings at most one block per compute unit."""
    return 2 if separate or blocks_of(shapes) > eng.compute_units() else 1


def oracle(key, tracks, epoch, det):
    """The oracle's answer, computed once per (scene, frame) and shared by the runs that are held to it."""
    if key not in _refs:
        _refs[key] = O.associate(make_cfg(), tracks, epoch, det)
    return _refs[key]


def engine(extra=0):
    cfg = make_cfg()
    cfg.flags |= abi.SA_FLAG_TAP | abi.SA_FLAG_LAZY_POSITIONAL | abi.SA_FLAG_ONE_LAUNCH | extra
    return cfg, Engine(cfg)


def same_words(a, b, what):
    for name, x, y in zip(("row weight", "row index", "column weight", "column index", "kind"), a, b):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {name}")


def single_scene_frames(key, sc, frames, graph=0):
    """`frames` = [(epoch, detection scene)] through sa_associate on one engine per form; returns the one-launch form's answers."""
    tracks = V.tracks_of(sc)
    got = {}
    for separate in (0, SEPARATE):
        cfg, eng = engine(separate | graph)
        try:
            eng.upsert(0, tracks)
            for f, (epoch, dsc) in enumerate(frames):
                det = V.dets_of(dsc)
                ref = oracle((key, f), tracks, epoch, det)
                ids, votes = eng.associate(0, epoch, det)
                assert eng.last_frame_launches() == launches(eng, [(det.n, tracks.n)], separate), (separate, f)
                np.testing.assert_array_equal(ids, ref["track_id"], err_msg=f"separate={separate} frame {f}")
                np.testing.assert_array_equal(votes, ref["voting_type"], err_msg=f"separate={separate} frame {f}")
                P.check_votes(cfg, eng, ref["visual"])
                got[separate, f] = (ids, votes, eng.tap_votes(0))
        finally:
            eng.close()
    for f in range(len(frames)):
        np.testing.assert_array_equal(got[0, f][0], got[SEPARATE, f][0])
        np.testing.assert_array_equal(got[0, f][1], got[SEPARATE, f][1])
        same_words(got[0, f][2], got[SEPARATE, f][2], f"frame {f}")
    return [got[0, f] for f in range(len(frames))]


# 1 x 1: one tile, the other blocks of the XCD chunk idle | 64 x 65: two tiles | 130 x 190: 9 tiles, most shards with one arrival |
# 1000 x 1000: 256 tiles, every shard full | 1024 x 1: sixteen tiles in one column
SHAPES = [(1, 1), (64, 65), (130, 190), (1000, 1000), (1024, 1)]


@pytest.mark.parametrize("n,t", SHAPES, ids=[f"{n}x{t}" for n, t in SHAPES])
def test_shapes_with_leftover_rows(n, t):
    """The builder's scenes (15 % new objects, 15 % of the detections under the quality gate): the lazy phase and the solvers run inside
    the launch.  The frame runs twice on the same engine: the second run finds the ticket reset and the words re-armed by the first."""
    sc = V.scene(7000 + 7 * n + t, n, t, d=D)
    (ids, votes, (_, ri, _, _, _)), _ = single_scene_frames(("shape", n, t), sc, [(1, sc), (1, sc)])
    if n >= 64 and t >= 64:
        assert (ri < 0).any() and (votes == abi.SA_VOTE_VISUAL).any()


def test_frame_the_vote_decides_whole():
    """No new object, every detection usable: no leftover row, the tail's fast exit."""
    n = t = 1000
    rng = np.random.default_rng(7100)
    sc = synth.visual_scene(rng, t, n, D, 1, canvas=(1920.0, 1080.0), new_fraction=0.0)
    (ids, votes, (_, ri, _, _, _)), = single_scene_frames("decided", sc, [(1, sc)])
    assert (ri >= 0).all() and (votes == abi.SA_VOTE_VISUAL).sum() > 0.9 * n


def test_three_different_frames_back_to_back():
    sc = V.scene(7200, 600, 640, d=D)
    other = V.scene(7201, 600, 640, d=D)
    other.update({k: sc[k] for k in ("track_ids", "track_boxes", "track_epochs", "track_feats", "track_present")})
    single_scene_frames("three", sc, [(1, sc), (2, other), (3, sc)])


def test_graph_replay():
    sc = V.scene(7300, 130, 190, d=D)
    single_scene_frames("graph", sc, [(1, sc), (1, sc), (1, sc)], graph=abi.SA_FLAG_GRAPH)


def test_survivor_list_overflows():
    """A 600 x 640 crowd with every detection under the quality gate: every row is left over, and more cells survive the lazy screen than
    its list holds (the oracle's present cells on leftover rows x non-excluded columns are a subset of the survivors) — the batched
    re-screen, the edge pool in the tile's LDS, and the solvers inside the launch."""
    sc = L.crowd(7600, 600, 640, (350.0, 230.0), d=D, visual=0.0)
    tracks, det = V.tracks_of(sc), V.dets_of(sc)
    ref = oracle(("overflow", 0), tracks, 1, det)
    assert L.present_in_lazy_set(ref, make_cfg()) > P.LZ_CAP
    (ids, votes, _), = single_scene_frames("overflow", sc, [(1, sc)])
    assert (votes == abi.SA_VOTE_POSITIONAL).sum() > 0.5 * det.n and (votes == abi.SA_VOTE_VISUAL).sum() == 0


# the first set brings 4 x 104 blocks — on a part of 256 compute units more than one each: two launches in both runs, i.e. the set only
# holds the plan to its limit there; the second (4 x 32 blocks) runs ragged scenes through the one-launch kernel
SETS = [[(130, 190), (1, 1), (600, 640), (64, 65)], [(130, 190), (1, 1), (300, 320), (64, 65)]]


@pytest.mark.parametrize("shapes", SETS, ids=["600x640_widest_416_blocks_past_the_limit", "300x320_widest_128_blocks_one_launch"])
def test_request_set_of_ragged_scenes(shapes):
    """One request set (blockIdx.z = scene, a ticket block per scene), staged once and run three times without restaging."""
    scs = [V.scene(7400 + 10 * shapes[2][0] + s, n, t, d=D) for s, (n, t) in enumerate(shapes)]
    trs = [abi.make_tracks(sc["track_ids"] + 10000 * s, sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"],
                           feat_present=sc["track_present"]) for s, sc in enumerate(scs)]
    dets = [V.dets_of(sc) for sc in scs]
    refs = [oracle(("set", shapes[2], s), trs[s], 1, dets[s]) for s in range(len(scs))]
    words = {}
    for separate in (0, SEPARATE):
        cfg, eng = engine(separate)
        try:
            for s in range(len(scs)):
                eng.upsert(500 + s, trs[s])
            eng.batch_begin()
            slots = [eng.batch_add(500 + s, 1, dets[s]) for s in range(len(scs))]
            for rep in range(3):
                eng.batch_run()
                eng.batch_sync()
                assert eng.last_frame_launches() == launches(eng, shapes, separate), (separate, rep)
                for s in range(len(scs)):
                    ids, votes = eng.batch_fetch(slots[s], dets[s].n)
                    np.testing.assert_array_equal(ids, refs[s]["track_id"], err_msg=f"separate={separate} scene {s} run {rep}")
                    np.testing.assert_array_equal(votes, refs[s]["voting_type"], err_msg=f"separate={separate} scene {s} run {rep}")
                    P.check_votes(cfg, eng, refs[s]["visual"], slot=slots[s])
                    words[separate, s, rep] = eng.tap_votes(slots[s])
        finally:
            eng.close()
    for (separate, s, rep), w in words.items():
        if not separate:
            same_words(w, words[SEPARATE, s, rep], f"scene {s} run {rep}")


def test_pipelined_round_with_completion_words():
    """One sa_pipe_submit / sa_pipe_wait round: the launch that holds the tail reports each scene's end by its completion word."""
    sc = V.scene(7500, 130, 190, d=D)
    tracks, det = V.tracks_of(sc), V.dets_of(sc)
    ref = oracle(("pipe", 0), tracks, 1, det)
    for separate in (0, SEPARATE):
        cfg = make_cfg()
        cfg.flags |= abi.SA_FLAG_LAZY_POSITIONAL | abi.SA_FLAG_ONE_LAUNCH | separate
        eng = Engine(cfg)
        try:
            eng.upsert(3, tracks)
            for _ in range(2):
                req, res, outs = Engine.make_requests([(3, 1, det)])
                eng.pipe_wait(eng.pipe_submit(req), res)
                assert eng.last_frame_launches() == launches(eng, [(det.n, tracks.n)], separate)
                np.testing.assert_array_equal(outs[0][0], ref["track_id"])
                np.testing.assert_array_equal(outs[0][1], ref["voting_type"])
        finally:
            eng.close()
