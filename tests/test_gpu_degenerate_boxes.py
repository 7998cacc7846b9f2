"""The GPU clippers on constructed degenerate pairs of oriented boxes (tests/degenerate_boxes.py): touching, collinear, concentric and
almost parallel boxes at coordinates up to 1e6, where the reference's Sutherland-Hodgman clip returns NaN, IoU above 1 or rounding
noise.  Everything is compared bit for bit with the oracle computed here: no tolerance, no golden file.

  sparse scene   every 16 x 64 positional tile has at most 32 surviving cells: clip_area_lanes<8>; the dense tap runs the serial
                 sa_clip_area_ws at stride 64
  mid scene      three huge "umbrella" tracks per 64 columns lift every tile that holds a pair to 33 .. 64 survivors: clip_area_lanes<4>
                 without the emptiness proof
  crowded scene  five umbrellas: more than 64 survivors, so sa_clip_is_empty runs first, then clip_area_lanes<4>
  lazy tail      the same pairs behind a visual vote that leaves their rows over: clip_area_lanes<8> of the one-workgroup tail
  NMS            k_nms_mask's serial clip and its `metric > threshold`, cluster by cluster (a base box and all its partners)"""
import functools

import numpy as np
import pytest

import degenerate_boxes as D
import oracle_lib as O
from similari_amd import abi, synth
from similari_amd.engine import Engine
from test_gpu_parity import check_sort, thr_q_of
from test_lazy_positional import leftover_edges

N_PAIRS = 608          # 38 full blocks of 16 detection rows
TI, TJ = 16, 64        # the positional tile of frames this size (sa_launch_frame: 16 x 256 only from 256 such tiles on)


def umbrella(k):
    """A track without an angle whose bounding circle holds every box of the scenes (coordinates up to 1e6): no cell of its column is
    too_far, none reaches a threshold (IoU below 1e-8)."""
    return (1000.0 * k, -1000.0 * k, None, 1.0, 4e6 * (1.0 + 0.01 * k))


@functools.lru_cache(maxsize=None)
def scene(umbrellas, lead="example"):
    """Track j of the pairs gets one box, detection perm(j) its partner; `umbrellas` umbrella tracks lead every block of 64 columns.
    Returns (scene dict, families, pair of each detection row, column of each pair's track, not-too_far matrix from or_too_far)."""
    tr, dt, fam = D.placed_pairs(N_PAIRS, lead=lead)
    rng = np.random.default_rng(77)
    perm = rng.permutation(N_PAIRS)
    per = TJ - umbrellas
    rows, col_of = [], np.zeros(N_PAIRS, np.int64)
    for p in range(N_PAIRS):
        if umbrellas and p % per == 0:
            rows += [umbrella(k) for k in range(umbrellas)]
        col_of[p] = len(rows)
        rows.append(tr[p])
    tb = D.to_boxes(rows)
    db = D.to_boxes(dt)[perm]
    db["confidence"] = rng.choice(np.array([1.0, 0.9, 0.6], np.float32), N_PAIRS)
    n, t = len(db), len(tb)
    assert -(-t // 256) * -(-n // TI) < 256, "the frame would take the 16 x 256 tiles"
    L = O.lib()
    near = np.zeros((n, t), bool)
    for i in range(n):
        pi = O.box_ptr(db, i)
        for j in range(t):
            near[i, j] = not L.or_too_far(pi, O.box_ptr(tb, j))
    sc = dict(track_ids=np.arange(1, t + 1, dtype=np.uint64), track_boxes=tb, track_epochs=np.zeros(t, np.uint64), det_boxes=db)
    return sc, fam, perm, col_of, near


def check_layout(umbrellas, lo, hi, lead="example"):
    """Every detection is within too_far reach of its partner only (and of every umbrella); the tiles that hold a pair have lo .. hi
    surviving cells.  Returns the scene."""
    sc, fam, perm, col_of, near = scene(umbrellas, lead)
    n, t = near.shape
    is_umbrella = np.ones(t, bool)
    is_umbrella[col_of] = False
    assert is_umbrella.sum() == umbrellas * -(-N_PAIRS // (TJ - umbrellas)) if umbrellas else not is_umbrella.any()
    assert near[:, is_umbrella].all()
    partner = np.zeros((n, t), bool)
    partner[np.arange(n), col_of[perm]] = True
    assert not (near & ~partner & ~is_umbrella[None, :]).any(), "a detection reaches a box of another pair"
    assert (near & partner).sum() > 0.8 * N_PAIRS
    pad_n, pad_t = -(-n // TI) * TI, -(-t // TJ) * TJ
    padded = np.zeros((pad_n, pad_t), np.int64)
    padded[:n, :t] = near
    per_tile = padded.reshape(pad_n // TI, TI, pad_t // TJ, TJ).sum(axis=(1, 3))
    holds = np.zeros_like(per_tile, bool)
    holds[np.arange(n) // TI, col_of[perm] // TJ] = True
    assert lo <= per_tile[holds].min() and per_tile[holds].max() <= hi, (per_tile[holds].min(), per_tile[holds].max())
    if not umbrellas:
        assert per_tile.max() <= hi
    # what the scene is for: the NaN family, identical boxes, the touching families, the pair the proof used to drop, results of 12 and of 13 vertices
    kinds = [f.split(":")[0] for f in fam]
    assert kinds.count("aspect") >= 4 and kinds.count("same") >= 1 and kinds.count("twelve") == 3 and kinds.count("example") + kinds.count("thirteen") == 4
    assert kinds.count("shift") + kinds.count("other") > 500
    return sc


def run_sort(sc, thr):
    cfg = abi.make_config(positional="iou", positional_threshold=thr, positional_min_confidence=0.05, max_idle_epochs=5)
    # (a detection has at most one cell that is not too_far or an umbrella's, and no umbrella's cell reaches a threshold: the optimum is unique)
    ids, ref = check_sort(cfg, sc, require_ids=True)
    present = ~np.isnan(ref["positional"])
    assert present.sum() >= 40 and (ref["quantised"][present] > thr_q_of(cfg)).sum() >= 40 and (ids != 0).sum() >= 40
    assert (ref["positional"][present] > 1.0).sum() >= 1, "no cell with IoU above 1"
    return ref


@pytest.mark.gpu
@pytest.mark.paths("general", "never_lean")
@pytest.mark.parametrize("thr", [0.0, 0.05, 0.3])
def test_sparse_scene_eight_lane_and_serial_clippers(thr):
    """(threshold 0.0: every cell whose reference intersection is neither 0.0 nor NaN is present and compared in bits, noise included)"""
    ref = run_sort(check_layout(0, 0, 32), thr)
    sc, fam, perm, col_of, near = scene(0)
    example = int(np.nonzero(perm == fam.index("example"))[0][0])
    assert ref["positional"][example, col_of[fam.index("example")]] > 0.3     # the reference's IoU of 0.558 x confidence for two disjoint slivers


@pytest.mark.gpu
@pytest.mark.paths("general", "never_lean")
@pytest.mark.parametrize("thr", [0.0, 0.05])
def test_mid_scene_four_lane_clipper_without_the_proof(thr):
    run_sort(check_layout(3, 33, 64), thr)


@pytest.mark.gpu
@pytest.mark.paths("general", "never_lean")
@pytest.mark.parametrize("thr", [0.0, 0.05])
def test_crowded_scene_proof_then_four_lane_clipper(thr):
    ref = run_sort(check_layout(5, 65, TI * TJ), thr)
    sc, fam, perm, col_of, near = scene(5)
    example = int(np.nonzero(perm == fam.index("example"))[0][0])
    assert ref["positional"][example, col_of[fam.index("example")]] > 0.3     # (the proof must not drop it)
    # the proof has pairs to drop: cells that are not too_far and absent in the reference, between oriented boxes
    partner = np.zeros_like(near)
    partner[np.arange(len(perm)), col_of[perm]] = True
    assert (near & partner & np.isnan(ref["positional"])).sum() > 50


@pytest.mark.gpu
@pytest.mark.parametrize("umbrellas,lo,hi", [(0, 0, 32), (3, 33, 64), (5, 65, TI * TJ)], ids=["eight_lanes", "four_lanes", "proof_then_four_lanes"])
def test_thirteen_vertex_pair_leaves_the_lane_clippers(umbrellas, lo, hi):
    """The same three scenes with one pair exchanged: where the example stood, two concentric boxes of 0.01 px at (1e6, 1e6) whose clip
    result has 13 vertices, one more than clip_area_lanes' lists hold.  The reference's IoU is -1.43, so the cell is absent; with the
    13th vertex lost it came to 21.88, an edge.  The lane clippers hand such a pair to the serial one."""
    ref = run_sort(check_layout(umbrellas, lo, hi, lead="thirteen"), 0.0)
    sc, fam, perm, col_of, near = scene(umbrellas, "thirteen")
    row = int(np.nonzero(perm == fam.index("thirteen"))[0][0])
    assert near[row, col_of[0]] and np.isnan(ref["positional"][row, col_of[0]])


@functools.lru_cache(maxsize=None)
def lazy_scene(d=32):
    """The sparse scene behind a cosine vote: every pair's detection has a feature below the quality gate (no visual verdict: its row is
    left over), and eight ordinary overlapping pairs vote visually, so that the frame can tell the positional modes apart."""
    sc, fam, perm, col_of, near = scene(0)
    rng = np.random.default_rng(78)
    extra = 8
    xs = -5000.0 - 300.0 * np.arange(extra)
    tb = np.concatenate([sc["track_boxes"], abi.make_boxes(xs, np.full(extra, -5000.0), np.full(extra, 0.5), np.full(extra, 60.0))])
    db = np.concatenate([sc["det_boxes"], abi.make_boxes(xs + 3.0, np.full(extra, -5000.0), np.full(extra, 0.5), np.full(extra, 60.0))])
    n = len(tb)
    feats = synth.reid_identities(rng, n, d).astype(np.float32)
    order = np.concatenate([perm, np.arange(N_PAIRS, n)])           # detection i shows the feature of its own track
    quality = np.full(n, 0.05, np.float32)
    quality[N_PAIRS:] = 0.9
    return dict(track_ids=np.arange(1, n + 1, dtype=np.uint64), track_boxes=tb, track_epochs=np.zeros(n, np.uint64),
                track_feats=feats[:, None, :].copy(), track_present=np.ones((n, 1), np.uint8),
                det_boxes=db, det_feats=feats[order], det_quality=quality)


@pytest.mark.gpu
@pytest.mark.parametrize("pos_mode", ["eager", "lazy"])
def test_lazy_tail_clipper(pos_mode):
    check_layout(0, 0, 32)
    cfg = abi.make_config(positional="iou", positional_threshold=0.05, visual="cosine", visual_threshold=0.2, feature_len=32,
                          max_observations=1, visual_min_votes=1, visual_minimal_track_length=1, visual_minimal_quality_use=0.5,
                          positional_min_confidence=0.05, max_idle_epochs=5)
    rows, edges, ref = leftover_edges(cfg, lazy_scene(), pos_mode=pos_mode)
    assert rows > 0 and edges > 0
    assert rows >= N_PAIRS and edges > 100


# ---- NMS ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clusters():
    """A base box and all its partners (the NaN family and identical oriented boxes among them), for every eighth base of the generator."""
    out = []
    for mag, a, h, theta in D.bases()[::8]:
        rows = [(D.r32(mag), D.r32(mag), theta, a, h)] + [box for _, box in D.partners(mag, mag, a, h, theta)]
        out.append(D.to_boxes(rows))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("with_scores", [False, True])
def test_nms_clusters(with_scores):
    """sa_nms equals the oracle index for index on every cluster (one call per cluster: its rank order — height, or score — is then
    settled by the stable sort alone), at thresholds 0.5, 0.3, 1.0 and -1.0: `metric > threshold` with NaN and IoU-above-1 metrics."""
    rng = np.random.default_rng(79)
    eng = Engine(abi.make_config())
    suppressed = nan_pairs = 0
    L = O.lib()
    try:
        for b in clusters():
            s = None
            if with_scores:
                s = rng.uniform(0, 1, len(b)).astype(np.float32)
                s[::11] = np.nan
            for thr in (0.5, 0.3, 1.0, -1.0):
                got = eng.nms(b, s, thr, None)
                want = O.nms(b, s, thr, None)
                np.testing.assert_array_equal(got, want)
            suppressed += len(b) - len(O.nms(b, s, 0.5, None))
            nan_pairs += sum(np.isnan(L.or_intersection(O.box_ptr(b, 0), O.box_ptr(b, j))) + np.isnan(L.or_intersection(O.box_ptr(b, j), O.box_ptr(b, 0)))
                             for j in range(1, 16))
    finally:
        eng.close()
    assert suppressed > 100 and nan_pairs >= 3
