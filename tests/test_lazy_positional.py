"""The positional stage's two modes (similari_amd/csrc/sa_lazy.h).  Eager: the first phase evaluates every positional cell.  Lazy: it
evaluates none, and the one-workgroup tail evaluates the cells of the rows the visual vote leaves over (rows without a visual group x
tracks no visual winner took).  Both must give the oracle's ids and vote types; the lazy edges must be the oracle's quantised cells on
exactly those rows and columns."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from similari_amd import abi, synth
from similari_amd.engine import Engine
from test_gpu_parity import thr_q_of

CSRC = __import__("pathlib").Path(__file__).resolve().parent.parent / "similari_amd" / "csrc"
EAGER, LAZY = abi.SA_FLAG_EAGER_POSITIONAL, abi.SA_FLAG_LAZY_POSITIONAL


def test_mode_decision(tmp_path):
    """sa_lazy_positional on its own (host-only): the form decides first, then the forcing bits, then the scenes' hint."""
    src = tmp_path / "mode.cpp"
    src.write_text('#include "sa_lazy.h"\nextern "C" int lazy(int possible, unsigned flags, unsigned left) '
                   "{ return sa_lazy_positional(possible != 0, flags, left) ? 1 : 0; }\n")
    so = tmp_path / "libmode.so"
    subprocess.run(["g++", "-std=c++17", "-fPIC", "-shared", "-I", str(CSRC), "-o", str(so), str(src)], check=True)
    f = C.CDLL(str(so)).lazy
    f.argtypes = [C.c_int, C.c_uint32, C.c_uint32]
    lmax = int(next(line.split()[2].rstrip("u") for line in (CSRC / "sa_lazy.h").read_text().splitlines()
                    if line.startswith("#define SA_LAZY_MAX_LEFT")))
    tap = abi.SA_FLAG_TAP
    assert f(1, 0, 0) == 1 and f(1, 0, lmax) == 1 and f(1, 0, lmax + 1) == 0
    assert f(0, 0, 0) == 0 and f(0, LAZY, 0) == 0          # no lazy phase on this form, whatever is asked
    assert f(1, EAGER, 0) == 0 and f(1, LAZY, 1000) == 1
    assert f(1, tap, 0) == 0 and f(1, tap | LAZY, 1000) == 1   # the taps see eager edges unless lazy is asked for
    assert f(1, abi.SA_FLAG_GRAPH | abi.SA_FLAG_PROFILE, 3) == 1


def frame(seed, n, t, d, left, oriented=False):
    """A 1-observation VisualSORT frame in which about `left` of the detections find no visual group: half of them new objects, half
    with a feature below the quality gate."""
    rng = np.random.default_rng(seed)
    sc = synth.visual_scene(rng, t, n, d, 1, canvas=(4000.0, 3000.0), oriented=oriented, new_fraction=left / 2)
    low = rng.uniform(size=n) < left / 2
    sc["det_quality"][low] = 0.3
    return sc


def config(d, flags=0):
    return abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=d,
                           max_observations=1, visual_min_votes=1, visual_minimal_track_length=1, visual_minimal_quality_use=0.5,
                           positional_min_confidence=0.1, max_idle_epochs=5, flags=flags)


def inputs(sc):
    tracks = abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"], feat_present=sc["track_present"])
    det = abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"])
    return tracks, det


def run(cfg, sc, epoch=1):
    tracks, det = inputs(sc)
    eng = Engine(cfg)
    try:
        eng.upsert(0, tracks)
        return eng.associate(0, epoch, det)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("left", [0.0, 0.1, 0.5, 1.0])
def test_full_size_frames_in_every_mode(left):
    d = 512
    sc = frame(700 + int(left * 100), 1000, 1000, d, left)
    tracks, det = inputs(sc)
    ref = O.associate(config(d), tracks, 1, det)
    out = {}
    for name, flags in (("default", 0), ("lazy", LAZY), ("eager", EAGER)):
        ids, votes = run(config(d, flags), sc)
        np.testing.assert_array_equal(ids, ref["track_id"], err_msg=name)
        np.testing.assert_array_equal(votes, ref["voting_type"], err_msg=name)
        out[name] = (ids, votes)
    if left > 0:
        assert (out["lazy"][1] == abi.SA_VOTE_POSITIONAL).sum() > 0


def leftover_edges(cfg, sc):
    """Edges under forced lazy + the tap, against the oracle's quantised cells on leftover rows x non-excluded columns."""
    tracks, det = inputs(sc)
    ref = O.associate(cfg, tracks, 1, det)
    cfg.flags |= abi.SA_FLAG_TAP | LAZY
    eng = Engine(cfg)
    try:
        eng.upsert(0, tracks)
        ids, votes = eng.associate(0, 1, det)
        counts, cols, gains = eng.tap_edges(0)
        _, ri, _, ci, _ = eng.tap_votes(0)
    finally:
        eng.close()
    np.testing.assert_array_equal(ids, ref["track_id"])
    np.testing.assert_array_equal(votes, ref["voting_type"])
    left = ri < 0                                         # no visual group
    excl = np.zeros(len(ci), bool)
    has = ci >= 0
    excl[has] = ri[ci[has]] == np.nonzero(has)[0]         # the candidate best in the column takes it iff the column is its own best
    gain_ref = ref["quantised"].astype(np.int64) - int(thr_q_of(cfg))
    mask = (gain_ref > 0) & left[:, None] & ~excl[None, :]
    np.testing.assert_array_equal(counts, mask.sum(axis=1).astype(np.uint32))
    rows = np.repeat(np.arange(len(counts)), counts)
    order = np.lexsort((cols, rows))
    ref_rows, ref_cols = np.nonzero(mask)
    np.testing.assert_array_equal(rows[order], ref_rows)
    np.testing.assert_array_equal(cols[order], ref_cols.astype(np.uint32))
    np.testing.assert_array_equal(gains[order], gain_ref[mask])
    return int(left.sum()), int(mask.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("left", [0.1, 0.5])
def test_lazy_edges_are_the_oracles_cells_on_leftover_rows(left):
    rows, edges = leftover_edges(config(512), frame(710 + int(left * 100), 1000, 1000, 512, left))
    assert rows > 0 and edges > 0


@pytest.mark.gpu
def test_lazy_edges_of_oriented_boxes_and_idle_tracks():
    sc = frame(731, 600, 700, 64, 0.3, oriented=True)
    sc["track_epochs"][::7] = 100                        # beyond max_idle_epochs of the frame's epoch: incompatible
    rows, edges = leftover_edges(config(64), sc)
    assert rows > 0 and edges > 0


@pytest.mark.gpu
def test_mahalanobis_frames_stay_correct():
    """Mahalanobis has no lazy phase: the engine keeps such frames eager, also when lazy is asked for."""
    rng = np.random.default_rng(740)
    sc = frame(740, 200, 220, 64, 0.3)
    from test_gpu_parity import kf_states
    tb, m5, c25 = kf_states(rng, sc["track_boxes"])
    tracks = abi.make_tracks(sc["track_ids"], tb, sc["track_epochs"], feats=sc["track_feats"], feat_present=sc["track_present"],
                             kf_mean=m5, kf_cov=c25)
    det = abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"])
    cfg = abi.make_config(positional="maha", visual="cosine", visual_threshold=0.2, feature_len=64, visual_minimal_quality_use=0.5,
                          max_idle_epochs=5)
    ref = O.associate(cfg, tracks, 1, det)
    for flags in (0, LAZY):
        cfg.flags = flags
        eng = Engine(cfg)
        try:
            eng.upsert(0, tracks)
            ids, votes = eng.associate(0, 1, det)
        finally:
            eng.close()
        np.testing.assert_array_equal(ids, ref["track_id"])
        np.testing.assert_array_equal(votes, ref["voting_type"])


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, abi.SA_FLAG_GRAPH], ids=["eager_launches", "graph"])
def test_mode_follows_the_hint_across_frames(graph):
    """One engine, one scene, frames whose leftover fraction goes 0 -> 60 % -> 0 -> 100 % -> 0: every frame right, whichever mode the
    previous frame's hint chose (a frame with many leftovers after a lazy one runs lazily; the one after it eagerly)."""
    d = 256
    cfg = config(d, graph)
    eng = Engine(cfg)
    try:
        for f, left in enumerate([0.0, 0.6, 0.0, 1.0, 0.0, 0.0]):
            sc = frame(750 + f, 900, 1000, d, left)
            tracks, det = inputs(sc)
            ref = O.associate(config(d), tracks, 1, det)
            eng.upsert(0, tracks)
            ids, votes = eng.associate(0, 1, det)
            np.testing.assert_array_equal(ids, ref["track_id"], err_msg=f"frame {f}")
            np.testing.assert_array_equal(votes, ref["voting_type"], err_msg=f"frame {f}")
    finally:
        eng.close()
