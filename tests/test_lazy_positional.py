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
import test_gpu_parity as P
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


def leftover_edges(cfg, sc, epoch=1, pos_mode="lazy", prove=True):
    """One tapped frame with the positional mode forced: edges under check_edges' mode-aware gate (lazy: the oracle's cells on leftover
    rows x non-excluded columns; outside lazy_form: every cell), vote words under check_votes, ids and vote types against the oracle.
    prove=False: the caller states that the frame cannot tell the modes apart.  Returns (leftover rows, edges checked, oracle ref)."""
    tracks, det = inputs(sc)
    ref = O.associate(cfg, tracks, epoch, det)
    cfg.flags |= abi.SA_FLAG_TAP | P.POS_MODE_FLAGS[pos_mode]
    eng = Engine(cfg)
    try:
        eng.upsert(0, tracks)
        ids, votes = eng.associate(0, epoch, det)
        mode = P.mode_of(cfg, det.n, tracks.n)
        edges = P.check_edges(eng, ref["quantised"], thr_q_of(cfg), mode=mode, prove=prove, pos_ref=ref["positional"])
        P.check_votes(cfg, eng, ref["visual"])
        _, ri, _, _, _ = eng.tap_votes(0)
    finally:
        eng.close()
    np.testing.assert_array_equal(ids, ref["track_id"])
    np.testing.assert_array_equal(votes, ref["voting_type"])
    return int((ri < 0).sum()), edges, ref


@pytest.mark.gpu
@pytest.mark.parametrize("left", [0.1, 0.5])
def test_lazy_edges_are_the_oracles_cells_on_leftover_rows(left):
    rows, edges, _ = leftover_edges(config(512), frame(710 + int(left * 100), 1000, 1000, 512, left))
    assert rows > 0 and edges > 0


@pytest.mark.gpu
def test_lazy_edges_of_oriented_boxes_and_idle_tracks():
    sc = frame(731, 600, 700, 64, 0.3, oriented=True)
    sc["track_epochs"][::7] = 100                        # beyond max_idle_epochs of the frame's epoch: incompatible
    rows, edges, _ = leftover_edges(config(64), sc)
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


# ---- the lazy phase's overflow re-screen ---------------------------------------------------------------------------------------
# More than LZ_CAP screen survivors: the tail screens again in batches of LZ_CAP / T rows.  The oracle's present cells on leftover rows x
# non-excluded columns are a subset of the survivors, so a frame with more than LZ_CAP of them takes that branch.
def crowd(seed, n, t, canvas, d=32, visual=0.06):
    """Detections piled over the tracks (a crowd on a small canvas): all but about `visual` of them below the quality gate, so nearly
    every row is left over; the few that vote visually keep the frame able to tell lazy from eager."""
    rng = np.random.default_rng(seed)
    sc = synth.visual_scene(rng, t, n, d, 1, canvas=canvas, pos_sigma=3.0)
    sc["det_quality"][rng.uniform(size=n) >= visual] = 0.05
    return sc


def present_in_lazy_set(ref, cfg):
    """The oracle's present cells on leftover rows x non-excluded columns, the vote taken from the oracle's own visual matrix."""
    w = np.where(np.isnan(ref["visual"][:, :, 0]), np.inf, ref["visual"][:, :, 0].astype(np.float64))
    n, t = w.shape
    if n == 0 or t == 0:
        return 0
    ri = np.where(np.isfinite(w.min(axis=1)), w.argmin(axis=1), -1)
    ci = np.where(np.isfinite(w.min(axis=0)), w.argmin(axis=0), -1)
    excl = np.zeros(t, bool)
    has = ci >= 0
    excl[has] = ri[ci[has]] == np.nonzero(has)[0]
    return int((~np.isnan(ref["positional"]) & (ri < 0)[:, None] & ~excl[None, :]).sum())


# (n, t): canvas, fraction of detections that vote visually (a pile over 37 tracks: a few, or they would take most of its columns)
OVERFLOW = {(1000, 1000): ((450.0, 300.0), 0.06), (1024, 1024): ((450.0, 300.0), 0.06), (1000, 37): ((60.0, 50.0), 0.01),
            (300, 1024): ((300.0, 200.0), 0.06)}


@pytest.mark.gpu
@pytest.mark.parametrize("n,t", list(OVERFLOW), ids=[f"{n}x{t}" for n, t in OVERFLOW])
def test_overflow_rescreen_against_the_oracle(n, t):
    """Crowds whose leftover rows x non-excluded columns hold more than LZ_CAP present cells: the batched re-screen (1024 x 1024:
    three rows a batch, the last batch one row short; 1000 x 37: 83 rows a batch; 300 x 1024: three)."""
    cfg = config(32)
    canvas, visual = OVERFLOW[(n, t)]
    rows, edges, ref = leftover_edges(cfg, crowd(900 + n + t, n, t, canvas, visual=visual))
    assert present_in_lazy_set(ref, cfg) > P.LZ_CAP
    assert rows > 0.85 * n and edges > 0


@pytest.mark.gpu
def test_lazy_set_just_under_the_survivor_list():
    """A frame whose present cells in the lazy set sit just under LZ_CAP: either branch may run (the screen's survivors are a superset);
    the boundary of the gate, not a proof of the branch."""
    cfg = config(32)
    rows, edges, ref = leftover_edges(cfg, crowd(931, 700, 700, (504.0, 324.0)))
    assert P.LZ_CAP - 200 < present_in_lazy_set(ref, cfg) <= P.LZ_CAP


# ---- cells at the threshold -------------------------------------------------------------------------------------------------
# The lazy screen applies sa_aa_quick_reject to every cell (eager tiles only to tiles with more than 64 survivors): it must only drop
# cells the reference does not have.  Pairs of equal axis-aligned boxes shifted along x have IoU (w - dx) / (w + dx); dx is solved for
# IoU x confidence at the threshold, at one and two f32 ulp of it, and one and two steps of the x1e6 quantiser either side of gain 0,
# and then the detection's centre is also moved by a few f32 ulp: whatever those cells come to, the kernel's edges must be the oracle's.
def threshold_scene(seed, thr, min_conf, dense=False, d=32):
    rng = np.random.default_rng(seed)
    f32 = np.float32
    e_targets = [thr * (1 + k * 6e-8) for k in (-2, -1, 0, 1, 2)] + [thr + k * 1e-6 for k in (-2, -1, 1, 2, 3)]
    tb, db = [], []
    visual_pairs = []
    y = 0.0
    for mag in (1e1, 1e2, 1e3, 1e4, 1e5, 1e6):
        for k in range(24):
            h = float(np.exp(rng.uniform(np.log(1e-2), np.log(min(1e4, mag / 8)))))
            a = float(np.exp(rng.uniform(np.log(1e-3), np.log(1e3))))
            a = min(a, mag / 8 / h)                       # the box stays smaller than its coordinates
            w = a * h
            conf = [0.5 * min_conf, min_conf, 1.0, 0.75][k % 4]   # (above 1 the ABI refuses the box: bbox.rs:123-126)
            ce = max(conf, min_conf)
            r = e_targets[k % len(e_targets)] / ce
            if r >= 1.0:
                r = 0.95
            dx = w * (1 - r) / (1 + r)
            xc, yc = mag, mag + y
            y += 4 * max(w, h) + 1.0
            angle = [None, 0.0, -0.0][k % 3]
            for ulp in (-2, 0, 3):
                dxc = np.nextafter(f32(xc + dx), f32(np.inf) if ulp > 0 else f32(-np.inf))
                dxc = f32(xc + dx) if ulp == 0 else dxc
                for _ in range(abs(ulp) - 1):
                    dxc = np.nextafter(dxc, f32(np.inf) if ulp > 0 else f32(-np.inf))
                tb.append((xc, yc + 0 * ulp, a, h, 1.0, angle))
                db.append((float(dxc), yc, a, h, conf, angle))
                yc += 4 * max(w, h) + 1.0
                y += 4 * max(w, h) + 1.0
            # one pair that the visual vote decides (its detection sees its track's feature) and that also overlaps positionally
            visual_pairs.append(len(tb))
            tb.append((xc, yc, a, h, 1.0, None))
            db.append((xc + 0.05 * w, yc, a, h, 1.0, None))
            y += 4 * max(w, h) + 1.0
    if dense:   # a pile: positional tiles with more than 64 survivors, where the eager tiles use the quick reject too
        pile_t = synth.dense_boxes(rng, 200, (300.0, 200.0), h=(20.0, 60.0))
        pile_d = synth.jitter_boxes(rng, pile_t, 6.0)
        for b in pile_t:
            tb.append((float(b["xc"]) - 5e3, float(b["yc"]) - 5e3, float(b["aspect"]), float(b["height"]), 1.0, None))
        for b in pile_d:
            db.append((float(b["xc"]) - 5e3, float(b["yc"]) - 5e3, float(b["aspect"]), float(b["height"]), float(rng.uniform(0.2, 1.0)), None))

    def boxes(rows):
        b = abi.make_boxes([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows],
                           confidence=[r[4] for r in rows])
        for i, r in enumerate(rows):
            if r[5] is not None:
                b["has_angle"][i], b["angle"][i] = 1, r[5]
        return b

    n = len(db)
    feats = synth.reid_identities(rng, n, d).astype(np.float32)
    quality = np.full(n, 0.05, np.float32)
    quality[visual_pairs] = 0.9
    perm = rng.permutation(n)                            # the detections in another order than their tracks
    return dict(track_ids=np.arange(1, n + 1, dtype=np.uint64), track_boxes=boxes(tb), track_epochs=np.zeros(n, np.uint64),
                track_feats=feats[:, None, :].copy(), track_present=np.ones((n, 1), np.uint8),
                det_boxes=boxes(db)[perm], det_feats=feats[perm], det_quality=quality[perm])


@pytest.mark.gpu
@pytest.mark.parametrize("pos_mode", ["eager", "lazy"])
@pytest.mark.parametrize("dense", [False, True], ids=["pairs", "pairs_and_pile"])
@pytest.mark.parametrize("min_conf", [0.1, 0.5])
def test_threshold_cells_against_the_oracle(min_conf, dense, pos_mode):
    """Constructed pairs at and around the threshold (threshold_scene), coordinates 1e1 .. 1e6, heights 1e-2 .. 1e4, aspects 1e-3 .. 1e3,
    confidence below / at positional_min_confidence, 0.75 and 1, has_angle with angle 0.0 and -0.0; with a pile beside them whose
    eager tiles take the quick-reject branch.  min_conf 0.5 lifts the confidence of the low ones to it before the product."""
    thr = 0.3
    cfg = abi.make_config(positional="iou", positional_threshold=thr, visual="cosine", visual_threshold=0.2, feature_len=32,
                          max_observations=1, visual_min_votes=1, visual_minimal_track_length=1, visual_minimal_quality_use=0.5,
                          positional_min_confidence=min_conf, max_idle_epochs=5)
    rows, edges, ref = leftover_edges(cfg, threshold_scene(5, thr, min_conf, dense), pos_mode=pos_mode)
    gain = ref["quantised"].astype(np.int64) - thr_q_of(cfg)
    pres = ~np.isnan(ref["positional"])
    cells = ref["positional"][pres]
    # the frame reaches the edges it is built for: cells at gain 0 (present, no edge), 1 and 2, and cells within 0.1 % above the threshold
    assert all(((gain == g) & pres).sum() > 0 for g in (0, 1, 2))
    assert ((cells >= np.float32(thr)) & (cells < np.float32(thr) / np.float32(0.999))).sum() > 20
    assert rows > 0 and edges > 0


# ---- what the screen reads ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pos_mode", ["eager", "lazy"])
def test_screen_inputs_against_the_oracle(pos_mode):
    """Spatio-temporal constraints (three), tracks idle beyond max_idle_epochs, tracks without a feature, the quality and area gates,
    and pairs whose centres sit at the too_far radius (sum of the half diagonals, corner to corner)."""
    rng = np.random.default_rng(960)
    n, t, d = 500, 560, 32
    sc = synth.visual_scene(rng, t, n, d, 1, canvas=(1400.0, 900.0), new_fraction=0.15, pos_sigma=6.0)
    sc["det_quality"][rng.uniform(size=n) < 0.15] = 0.3                       # below the quality gate
    sc["track_epochs"] = rng.integers(0, 9, t).astype(np.uint64)              # frame epoch 8: idle 0 .. 8 epochs, beyond 5 incompatible
    sc["track_present"][rng.uniform(size=t) < 0.1] = 0                       # tracks without a feature
    small = rng.uniform(size=n) < 0.1                                         # detections under the area gate
    sc["det_boxes"]["height"][small] = 12.0
    # the too_far radius: the last 20 rows / columns are pairs of equal boxes touching corner to corner
    for k in range(20):
        i, j = n - 1 - k, t - 1 - k
        b = sc["track_boxes"][j]
        b["xc"], b["yc"], b["height"], b["aspect"] = 3000.0 + 100.0 * k, 3000.0, 40.0, 0.5
        r = np.float32(np.hypot(10.0, 20.0))
        c = sc["det_boxes"][i]
        c["xc"], c["yc"], c["height"], c["aspect"] = b["xc"] + np.float32(2 * r / np.sqrt(5.0)), b["yc"] + np.float32(4 * r / np.sqrt(5.0)), 40.0, 0.5
        sc["track_epochs"][j] = 8
    cfg = abi.make_config(positional="iou", positional_threshold=0.2, visual="cosine", visual_threshold=0.2, feature_len=d,
                          max_observations=1, visual_min_votes=1, visual_minimal_track_length=1, visual_minimal_quality_use=0.5,
                          visual_minimal_area=400.0, positional_min_confidence=0.1, max_idle_epochs=5,
                          constraints=[(1, 0.3), (3, 1.0), (6, 2.0)])
    rows, edges, ref = leftover_edges(cfg, sc, epoch=8, pos_mode=pos_mode)
    assert rows > 0.2 * n and edges > 0
    assert ref["compatible"].sum() < ref["compatible"].size and (ref["voting_type"] == abi.SA_VOTE_POSITIONAL).sum() > 0


# ---- the tail's shapes ----------------------------------------------------------------------------------------------------------
def shaped(seed, n, t, d=32):
    """A frame whose density does not depend on its size: about 30 % of the rows left over (new objects, features below the gate)."""
    rng = np.random.default_rng(seed)
    s = np.sqrt(max(n, t, 1) / 1000.0)
    sc = synth.visual_scene(rng, t, n, d, 1, canvas=(1920.0 * s, 1080.0 * s), new_fraction=0.15)
    sc["det_quality"][rng.uniform(size=n) < 0.15] = 0.3
    if n == 1:
        sc["det_quality"][:] = 0.3       # the one row is left over
    return sc


SHAPES = [(1, 1), (1, 1024), (1024, 1), (63, 65), (65, 63), (1023, 1024), (1024, 1024), (1024, 1025), (1025, 1024)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,t", SHAPES, ids=[f"{n}x{t}" for n, t in SHAPES])
def test_lazy_tail_shapes_against_the_oracle(n, t):
    """Forced lazy from one row or column to the tail's limit; one past it (1024 x 1025, 1025 x 1024) the engine stays eager — the mode
    proof holds it to the eager edges.  A frame of one detection cannot tell the modes apart (it has a visual verdict or a leftover
    row, not both): no proof there.  A frame of one track sees it taken visually: no lazy edge at all."""
    cfg = config(32)
    rows, edges, ref = leftover_edges(cfg, shaped(970 + n + 3 * t, n, t), prove=n > 1)
    assert rows > 0
    if n > 1 and t > 1:
        assert edges > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n,t", [(0, 50), (40, 0), (0, 0)], ids=["no_detections", "no_tracks", "neither"])
def test_lazy_empty_frames(n, t):
    sc = shaped(990, n, t)
    tracks, det = inputs(sc)
    ref = O.associate(config(32), tracks, 1, det)
    ids, votes = run(config(32, LAZY), sc)
    assert len(ids) == n
    np.testing.assert_array_equal(ids, ref["track_id"])
    np.testing.assert_array_equal(votes, ref["voting_type"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["euclidean", "three_observations", "two_votes", "mahalanobis", "bestfit_tile", "separate_resolve",
                                  "general_tail"])
def test_forced_lazy_outside_the_form_stays_eager(case):
    """Every branch of lazy_form that excludes a frame: forced lazy, the edges are every cell's (check_edges' eager proof: the frame has
    edges outside the lazy set).  visual_min_votes 2 over one observation leaves no row a visual group: lazy and eager edges coincide,
    so that case compares edges, ids and votes without the proof."""
    from test_gpu_parity import check_votes, kf_states, mode_of, thr_q_of as thr
    rng = np.random.default_rng(1000)
    k = 3 if case == "three_observations" else 1
    sc = synth.visual_scene(rng, 420, 400, 64, k, canvas=(1200.0, 800.0), new_fraction=0.15)
    sc["det_quality"][rng.uniform(size=400) < 0.15] = 0.3
    kw = dict(positional="maha") if case == "mahalanobis" else dict(positional="iou", positional_threshold=0.3)
    flags = {"bestfit_tile": abi.SA_FLAG_BESTFIT_TILE, "separate_resolve": abi.SA_FLAG_SEPARATE_RESOLVE,
             "general_tail": abi.SA_FLAG_GENERAL_TAIL}.get(case, 0)
    cfg = abi.make_config(visual="euclidean" if case == "euclidean" else "cosine", visual_threshold=0.5 if case == "euclidean" else 0.2,
                          feature_len=64, max_observations=k, visual_min_votes=2 if case == "two_votes" else 1,
                          visual_minimal_track_length=1, visual_minimal_quality_use=0.5, positional_min_confidence=0.1, max_idle_epochs=5,
                          flags=flags | abi.SA_FLAG_TAP | LAZY, **kw)
    assert mode_of(cfg, 400, 420) == "eager"
    tb, tkw = sc["track_boxes"], {}
    if case == "mahalanobis":
        tb, m5, c25 = kf_states(rng, sc["track_boxes"])
        tkw = dict(kf_mean=m5, kf_cov=c25)
    tracks = abi.make_tracks(sc["track_ids"], tb, sc["track_epochs"], feats=sc["track_feats"], feat_present=sc["track_present"], **tkw)
    det = abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"])
    ref = O.associate(cfg, tracks, 1, det)
    eng = Engine(cfg)
    try:
        eng.upsert(0, tracks)
        ids, votes = eng.associate(0, 1, det)
        assert P.check_edges(eng, ref["quantised"], thr(cfg), mode="eager", prove=case != "two_votes") > 0
        if case == "euclidean":
            check_votes(cfg, eng, ref["visual"], tol_abs=0.0, tol_rel=1e-5)
        else:
            check_votes(cfg, eng, ref["visual"])
    finally:
        eng.close()
    np.testing.assert_array_equal(ids, ref["track_id"])
    np.testing.assert_array_equal(votes, ref["voting_type"])


# ---- request sets, mode switches, pipelined tickets --------------------------------------------------------------------------------
def ragged_set():
    """(label, scene) of one request set: C2-sized with leftovers, a tiny one, one without detections, the tail's full size, an
    all-but-leftover pile, and one whose every row finds a visual group."""
    return [("c2", frame(1100, 1000, 1000, 32, 0.3)), ("tiny", shaped(1101, 3, 5)), ("empty", shaped(1102, 0, 40)),
            ("full", shaped(1103, 1024, 1024)), ("pile", crowd(1104, 600, 37, (60.0, 50.0), visual=0.01)),
            ("no_leftovers", frame(1105, 500, 520, 32, 0.0))]


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, abi.SA_FLAG_GRAPH], ids=["eager_launches", "graph"])
def test_ragged_request_set_forced_lazy(graph):
    """Six ragged scenes in ONE request set (blockIdx.z = scene through the lazy tail), forced lazy with the tap: every slot's edges under
    the mode-aware gate, its vote words, ids and vote types; twice, so that a captured graph is also replayed.  The tiny scene cannot
    tell the modes apart (no proof there)."""
    scenes = ragged_set()
    cfg = config(32, abi.SA_FLAG_TAP | LAZY | graph)
    assert P.mode_of(cfg, 1024, 1024) == "lazy"
    trs = [abi.make_tracks(sc["track_ids"] + 10000 * s, sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"],
                           feat_present=sc["track_present"]) for s, (_, sc) in enumerate(scenes)]
    dets = [abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"]) for _, sc in scenes]
    refs = [O.associate(config(32), trs[s], 1, dets[s]) for s in range(len(scenes))]
    eng = Engine(cfg)
    try:
        for s in range(len(scenes)):
            eng.upsert(300 + s, trs[s])
        for rep in range(2):
            eng.batch_begin()
            slots = [eng.batch_add(300 + s, 1, dets[s]) for s in range(len(scenes))]
            eng.batch_run()
            eng.batch_sync()
            for s, (label, _) in enumerate(scenes):
                ids, votes = eng.batch_fetch(slots[s], dets[s].n)
                np.testing.assert_array_equal(ids, refs[s]["track_id"], err_msg=f"{label} run {rep}")
                np.testing.assert_array_equal(votes, refs[s]["voting_type"], err_msg=f"{label} run {rep}")
                if dets[s].n == 0:
                    continue
                P.check_edges(eng, refs[s]["quantised"], thr_q_of(cfg), slot=slots[s], mode="lazy", prove=label != "tiny",
                              pos_ref=refs[s]["positional"])
                P.check_votes(cfg, eng, refs[s]["visual"], slot=slots[s])
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, abi.SA_FLAG_GRAPH], ids=["eager_launches", "graph"])
def test_request_set_switches_mode_by_its_scenes_hints(graph):
    """Default mode, three scenes over six frames whose leftover fractions disagree — the set goes lazy only when every scene's newest
    hint is small, so it switches back and forth (and a graph is captured for each mode): ids and vote types every frame."""
    d = 32
    cfg = config(d, graph)
    plan = [(0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.4), (0.0, 0.0, 0.0), (0.3, 0.3, 0.0), (0.0, 0.0, 0.0)]
    eng = Engine(cfg)
    try:
        for f, lefts in enumerate(plan):
            scs = [frame(1200 + 10 * f + s, 400 + 50 * s, 450, d, left) for s, left in enumerate(lefts)]
            trs = [inputs(sc)[0] for sc in scs]
            dets = [inputs(sc)[1] for sc in scs]
            for s in range(3):
                eng.upsert(400 + s, trs[s])
            eng.batch_begin()
            slots = [eng.batch_add(400 + s, 1, dets[s]) for s in range(3)]
            eng.batch_run()
            eng.batch_sync()
            for s in range(3):
                ref = O.associate(config(d), trs[s], 1, dets[s], want_matrices=False)
                ids, votes = eng.batch_fetch(slots[s], dets[s].n)
                np.testing.assert_array_equal(ids, ref["track_id"], err_msg=f"frame {f} scene {s}")
                np.testing.assert_array_equal(votes, ref["voting_type"], err_msg=f"frame {f} scene {s}")
    finally:
        eng.close()


@pytest.mark.gpu
def test_pipelined_tickets_read_the_hint_of_frames_in_flight():
    """Default mode through sa_pipe_submit with three tickets in flight, leftover fractions alternating 0 / 60 %: each set's mode comes
    from hints of frames that may not have retired yet; every ticket's ids and vote types against the oracle."""
    d = 32
    cfg = config(d)
    rng = np.random.default_rng(1300)
    sc = frame(1300, 500, 520, d, 0.0)
    tracks, _ = inputs(sc)
    dets = []
    for f in range(9):
        p = rng.permutation(500)[: 500 - 9 * f]
        q = sc["det_quality"].copy()
        if f % 2:
            q[rng.uniform(size=500) < 0.6] = 0.05          # 60 % of the rows left over: the next set's hint says eager
        dets.append(abi.make_detections(sc["det_boxes"][p], feats=sc["det_feats"][p], feat_quality=q[p]))
    eng = Engine(cfg)
    try:
        eng.upsert(7, tracks)
        reqs = [Engine.make_requests([(7, 1, det)]) for det in dets]
        tickets = []
        for f, (req, res, outs) in enumerate(reqs):
            tickets.append(eng.pipe_submit(req))
            if f >= 2:
                eng.pipe_wait(tickets[f - 2], reqs[f - 2][1])
        eng.pipe_wait(tickets[-2], reqs[-2][1])
        eng.pipe_wait(tickets[-1], reqs[-1][1])
    finally:
        eng.close()
    for f, det in enumerate(dets):
        ref = O.associate(cfg, tracks, 1, det, want_matrices=False)
        np.testing.assert_array_equal(reqs[f][2][0][0], ref["track_id"], err_msg=f"ticket {f}")
        np.testing.assert_array_equal(reqs[f][2][0][1], ref["voting_type"], err_msg=f"ticket {f}")
        if f % 2:
            assert (ref["voting_type"] == abi.SA_VOTE_POSITIONAL).sum() > 0


# ---- the tracker facade under SA_POSITIONAL --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["eager", "lazy"])
def test_facade_sequences_under_a_forced_mode(mode, monkeypatch):
    """The facade's one-observation VisualSORT sequences with SA_POSITIONAL set before the trackers (and their engines) are created: the
    facade builds its config without abi.make_config, so the variable is what forces the mode there."""
    import test_trackers as TT

    monkeypatch.setenv("SA_POSITIONAL", mode)
    for backend in ("gpu", "gpu_dev"):
        TT.test_visual_cosine_single_observation_sequence_matches_oracle(backend)
    TT.test_batch_visual_sort_single_observation_scenes_match_oracle()


# ---- the lazy gates ran -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lazy_gates_ran():
    """check_edges counted the lazy frames it held to the oracle (module-wide, this file's tests alone reach every count): frames,
    leftover rows, edges, and frames that took the overflow re-screen."""
    print("lazy gates:", P.LAZY_GATES)
    assert all(P.LAZY_GATES[k] > 0 for k in ("frames", "rows", "edges", "overflow")), P.LAZY_GATES
