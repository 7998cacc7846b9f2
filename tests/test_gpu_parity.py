"""GPU parity: the HIP path (through the C ABI) against the CPU oracle on the same seeded inputs.

Gates: positional f32 cells bit-identical with identical present/absent masks; IoU-quantised i64
matrix bit-exact; cosine |d| <= 1e-5 abs, euclid 1e-5 rel; BestFit winners identical; assignment indices identical
(unique optima: random f32 weights) and always equal total weight."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from similari_amd import abi, synth
from similari_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

PW, VW = np.float32(1 / 20), np.float32(1 / 160)


def kf_states(rng, boxes, steps=3):
    """Realistic track Kalman states: initiate + `steps` oracle predict/update cycles.
    Returns (state boxes, mean5, cov25)."""
    L = O.lib()
    n = len(boxes)
    out_boxes = boxes.copy()
    m5 = np.zeros((n, 5), np.float32)
    c25 = np.zeros((n, 25), np.float32)
    for i in range(n):
        m = np.zeros(10, np.float32)
        c = np.zeros(100, np.float32)
        b = boxes[i : i + 1].copy()
        sb = np.zeros(1, abi.BOX_DTYPE)
        L.or_make_prediction(PW, VW, 0, O.fptr(m), O.fptr(c), O.box_ptr(b), O.box_ptr(sb))
        for _ in range(steps - 1):
            b["xc"] += np.float32(rng.normal(0, 1.5))
            b["yc"] += np.float32(rng.normal(0, 1.5))
            L.or_make_prediction(PW, VW, 1, O.fptr(m), O.fptr(c), O.box_ptr(b), O.box_ptr(sb))
        out_boxes[i] = sb[0]
        m5[i] = m[:5]
        c25[i] = c.reshape(10, 10)[:5, :5].ravel()
    return out_boxes, m5, c25


def total_gain(res_ids, quant, track_ids, thr_q):
    col = {int(t): j for j, t in enumerate(track_ids)}
    g = 0
    for i, t in enumerate(res_ids):
        if t:
            g += int(quant[i, col[int(t)]]) - thr_q
    return g


def positional_optimum_is_unique(res_ids, quant, track_ids, thr_q):
    """Is the optimum of SortVoting's problem (sort/voting.rs:30-100: max sum of (weight - threshold) over a matching that only uses edges
    above the threshold) attained by ONE matching?  Perturb-and-resolve: every usable edge OUTSIDE the given optimal matching gets a bonus
    too small to outweigh one unit of gain; if the re-solved optimum collects any of it, another matching ties with the given one.
    (scipy's solver works in doubles: gains <= 1e8 scaled by 512 over <= a few hundred rows stay exact.)"""
    from scipy.optimize import linear_sum_assignment

    n, t = quant.shape
    if n == 0 or t == 0:
        return True
    gain = np.maximum(quant.astype(np.int64) - int(thr_q), 0)
    col = {int(tid): j for j, tid in enumerate(track_ids)}
    chosen = np.zeros((n, t), bool)
    for i, tid in enumerate(res_ids):
        if tid:
            chosen[i, col[int(tid)]] = True
    S = 512
    assert n < S and int(gain.max()) * S * max(n, 1) < 2 ** 52
    pert = gain * S + ((gain > 0) & ~chosen)
    dense = np.zeros((n, t + n), np.float64)        # n dummy columns: a row may stay unmatched at gain 0
    dense[:, :t] = pert
    r, c = linear_sum_assignment(dense, maximize=True)
    total = int(dense[r, c].sum())
    base = int(gain[chosen].sum())
    assert total // S == base, "the given matching is not optimal"
    return total % S == 0


# ---- the timed launches themselves under the gates ---------------------------------------------------------------------
# The matrix taps above RECOMPUTE the positional / visual matrices on demand (dense kernels on padded rows); the product path never
# writes them.  With SA_FLAG_TAP the assignment tail copies out what the frame's OWN launches produced before it consumes it — the
# edge records of the positional tiles and the BestFit vote words (or per-tile partials) of the first phase — and these two helpers
# hold THAT to the same gates: edges bit for bit, vote weights within the distance tolerance.
#
# The positional stage runs in one of two modes (similari_amd/csrc/sa_lazy.h).  Eager: the positional tiles emit every cell's edge.
# Lazy: the tail emits the cells of leftover rows (no visual group) x non-excluded columns only, after the vote.  SA_FLAG_TAP alone
# means eager, and SA_POSITIONAL does not reach tapped engines, so the tests pick a mode with these flags.
POS_MODE_FLAGS = {"eager": abi.SA_FLAG_EAGER_POSITIONAL, "lazy": abi.SA_FLAG_LAZY_POSITIONAL}
LZ_CAP = 3072   # the lazy phase's survivor list (k_assign_small<.., LAZY>): more survivors than this and it screens again in row batches
LAZY_GATES = {"frames": 0, "rows": 0, "edges": 0, "overflow": 0}   # lazy frames under check_edges; test_lazy_gates_ran reads them


def lazy_form(cfg, max_n, max_t):
    """The engine's `possible` (bank_launch with bf_partials of sa_engine_create): the frames that have a lazy phase at all."""
    f = cfg.flags
    return (cfg.visual_kind == abi.SA_VIS_COSINE and cfg.max_observations == 1 and cfg.visual_min_votes <= 1
            and cfg.positional_kind == abi.SA_POS_IOU
            and not f & (abi.SA_FLAG_BESTFIT_TILE | abi.SA_FLAG_SEPARATE_RESOLVE | abi.SA_FLAG_GENERAL_TAIL)
            and max_n <= 1024 and max_t <= 1024)


def mode_of(cfg, max_n, max_t):
    """The mode a tapped engine runs a frame in: lazy only where it is forced and the form has it."""
    return "lazy" if cfg.flags & abi.SA_FLAG_LAZY_POSITIONAL and lazy_form(cfg, max_n, max_t) else "eager"


def check_edges(eng, quant_ref, thr_q, slot=0, mode="eager", prove=False, pos_ref=None):
    """Edge set == the oracle's survivor set {(i, j): quantised[i, j] - threshold > 0}, every gain == the oracle's quantised cell.
    mode="lazy": the survivors on leftover rows x non-excluded columns only (both from the tapped vote words, which check_votes holds
    to the oracle).  prove: the frame tells the modes apart — lazy: a row with a visual verdict has an oracle edge (which the lazy
    phase must not emit); eager: an oracle edge lies outside the lazy set (which the lazy phase would not emit).  pos_ref (the oracle's
    positional cells, NaN = absent): lazy frames with more than LZ_CAP present cells in the lazy set are counted as overflow frames —
    present cells are a subset of the lazy screen's survivors."""
    counts, cols, gains = eng.tap_edges(slot)
    gain_ref = quant_ref.astype(np.int64) - int(thr_q)
    mask = gain_ref > 0
    if mode == "lazy" or prove:
        _, ri, _, ci, _ = eng.tap_votes(slot)
        left = ri < 0                                         # no visual group
        excl = np.zeros(len(ci), bool)
        has = ci >= 0
        excl[has] = ri[ci[has]] == np.nonzero(has)[0]         # the candidate best in the column takes it iff the column is its own best
        lazy_set = left[:, None] & ~excl[None, :]
        if prove and mode == "lazy":
            assert (mask & ~left[:, None]).any(), "no row with a visual verdict has an edge: the frame cannot tell lazy from eager"
        if prove and mode == "eager":
            assert (mask & ~lazy_set).any(), "every edge lies on a leftover row x non-excluded column: the frame cannot tell the modes apart"
        if mode == "lazy":
            mask &= lazy_set
            LAZY_GATES["frames"] += 1
            LAZY_GATES["rows"] += int(left.sum())
            LAZY_GATES["edges"] += int(mask.sum())
            if pos_ref is not None and int((~np.isnan(pos_ref) & lazy_set).sum()) > LZ_CAP:
                LAZY_GATES["overflow"] += 1
    else:
        assert mode == "eager", mode
    np.testing.assert_array_equal(counts, mask.sum(axis=1).astype(np.uint32))
    rows = np.repeat(np.arange(len(counts)), counts)
    order = np.lexsort((cols, rows))
    ref_rows, ref_cols = np.nonzero(mask)
    np.testing.assert_array_equal(rows[order], ref_rows)
    np.testing.assert_array_equal(cols[order], ref_cols.astype(np.uint32))
    np.testing.assert_array_equal(gains[order], gain_ref[mask])
    return int(mask.sum())


def thr_q_of(cfg):
    return 1000000 if cfg.positional_kind == abi.SA_POS_MAHALANOBIS else int(O.lib().or_quantise(cfg.positional_threshold))


def check_votes(cfg, eng, ref_visual, tol_abs=1e-5, tol_rel=0.0, slot=0):
    """The BestFit vote as the first phase reduced it against the oracle's weight matrix ref_visual[N, T, K] (NaN = absent):
    every row's / column's winning weight within the distance tolerance of the oracle's best, the winning index (near-)optimal in
    the oracle's matrix — exactly the argmin / argmax wherever the runner-up is more than 2 tolerances away.  A cell within
    tolerance of the is_ok threshold may exist on one side only: a winner that IS such a cell (or a row whose oracle best is one)
    is excused and counted."""
    rw, ri, cw, ci, kind = eng.tap_votes(slot)
    rv = ref_visual
    n, t, k = rv.shape
    present = ~np.isnan(rv)
    thr_w = (1.0 - cfg.visual_threshold) if cfg.visual_kind == abi.SA_VIS_COSINE else float(cfg.visual_threshold)
    excused = 0
    if kind == 1:
        assert k == 1
        w = np.where(present[:, :, 0], rv[:, :, 0].astype(np.float64), np.inf)   # lightest weight wins
        tol = lambda x: tol_abs + tol_rel * abs(x)                              # noqa: E731
        near_thr = lambda x: abs(x - thr_w) <= 2 * tol(thr_w)                    # noqa: E731
        for axis, (gw, gi) in enumerate(((rw, ri), (cw, ci))):
            m = w if axis == 0 else w.T
            best = m.min(axis=1)
            for q in range(m.shape[0]):
                if gi[q] < 0:
                    if np.isfinite(best[q]):
                        assert near_thr(best[q]), (axis, q, best[q])
                        excused += 1
                    continue
                if not np.isfinite(best[q]) or abs(gw[q] - best[q]) > tol(best[q]):
                    # the kernel's winner may be a threshold cell the oracle does not have, or the oracle's best one the kernel lacks
                    assert near_thr(gw[q]) or (np.isfinite(best[q]) and near_thr(best[q])), (axis, q, gw[q], best[q])
                    excused += 1
                    continue
                assert m[q, gi[q]] <= best[q] + 2 * tol(best[q]), (axis, q, gi[q], m[q, gi[q]], best[q])
    else:
        # deeper banks: W[q, t] = sum_k f64(max_dist - w_k) over the present k (>= min_votes of them), max_dist = the frame's largest
        # present weight (voting/best.rs:59); heaviest group wins.  The kernel's max_dist and every w_k carry the distance tolerance.
        if not present.any():
            assert (ri < 0).all() and (ci < 0).all()
            return 0
        max_dist = np.float32(np.nanmax(rv))
        diff = (max_dist - rv).astype(np.float32).astype(np.float64)   # f32 subtraction, then f64 (the reference's order)
        cnt = present.sum(axis=2)
        W = np.where(present, diff, 0.0).sum(axis=2)
        ok = (cnt >= 1) & (cnt >= cfg.visual_min_votes)
        W = np.where(ok, W, -np.inf)
        tolw = 4 * k * (tol_abs + tol_rel * float(max_dist)) + 1e-9   # k weights + k times the frame-wide max_dist, each within tolerance
        thr_cells = present & (np.abs(rv - thr_w) <= 2 * (tol_abs + tol_rel * abs(thr_w)))
        thr_any = thr_cells.any(axis=2)
        for axis, (gw, gi) in enumerate(((rw, ri), (cw, ci))):
            m = W if axis == 0 else W.T
            ta = thr_any if axis == 0 else thr_any.T
            best = m.max(axis=1)
            for q in range(m.shape[0]):
                on_threshold = bool(ta[q].any())   # a cell of this row / column may exist on one side only
                if gi[q] < 0:
                    if np.isfinite(best[q]):
                        assert on_threshold, (axis, q, best[q])
                        excused += 1
                    continue
                good = np.isfinite(best[q]) and abs(gw[q] - best[q]) <= tolw and m[q, gi[q]] >= best[q] - 2 * tolw
                if not good:
                    assert on_threshold, (axis, q, gw[q], best[q], gi[q])
                    excused += 1
    assert excused <= 2 + 1e-3 * (n + t), f"{excused} vote winners sit on the is_ok threshold"
    return excused


UNIQUE_CHECKS = {"frames": 0, "unique": 0}   # frames whose ids were compared only because their optimum proved unique


def check_sort(cfg, sc, epoch=1, kf=None, require_ids=True):
    tb = sc["track_boxes"]
    kw = {}
    if kf is not None:
        tb, m5, c25 = kf
        kw = dict(kf_mean=m5, kf_cov=c25)
    tracks = abi.make_tracks(sc["track_ids"], tb, sc["track_epochs"], **kw)
    det = abi.make_detections(sc["det_boxes"])
    ref = O.associate(cfg, tracks, epoch, det)
    cfg.flags |= abi.SA_FLAG_TAP
    eng = Engine(cfg)
    try:
        eng.upsert(0, tracks)
        ids, votes = eng.associate(0, epoch, det)
        check_edges(eng, ref["quantised"], thr_q_of(cfg))  # what the timed positional tiles emitted (before any tap re-launches a kernel)
        pos = eng.tap_positional()
        q = eng.tap_quantised()
    finally:
        eng.close()
    # identical present/absent mask and bit-identical f32 cells
    np.testing.assert_array_equal(np.isnan(pos), np.isnan(ref["positional"]))
    np.testing.assert_array_equal(pos.view(np.uint32)[~np.isnan(pos)], ref["positional"].view(np.uint32)[~np.isnan(pos)])
    np.testing.assert_array_equal(q, ref["quantised"])
    thr_q = 1000000 if cfg.positional_kind == abi.SA_POS_MAHALANOBIS else int(O.lib().or_quantise(cfg.positional_threshold))
    g_gpu = total_gain(ids, q, sc["track_ids"], thr_q)
    g_ref = total_gain(ref["track_id"], ref["quantised"], sc["track_ids"], thr_q)
    assert g_gpu == g_ref, "assignment totals differ"
    if not require_ids and len(ids) and q.shape[1] and len(ids) < 512:
        # equal totals always; identical ids whenever the oracle's optimum is the only one (a Mahalanobis frame ties wherever cells sit
        # beyond the chi-square bound at cost 0 — but where it does not, the assignment is as determined as an IoU frame's)
        require_ids = positional_optimum_is_unique(ref["track_id"], ref["quantised"], sc["track_ids"], thr_q)
        UNIQUE_CHECKS["frames"] += 1
        UNIQUE_CHECKS["unique"] += int(require_ids)
    if require_ids:
        np.testing.assert_array_equal(ids, ref["track_id"])
        np.testing.assert_array_equal(votes, ref["voting_type"])
    return ids, ref


@pytest.mark.paths("general", "never_lean")
@pytest.mark.parametrize("oriented", [False, True])
@pytest.mark.parametrize("n,t", [(257, 300), (64, 64), (1, 1), (130, 65)])
def test_sort_iou_parity(oriented, n, t):
    rng = np.random.default_rng(100 + n + 7 * t + oriented)
    sc = synth.sort_scene(rng, t, n, canvas=(1500.0, 900.0), oriented=oriented)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, max_idle_epochs=5)
    ids, ref = check_sort(cfg, sc)
    if n > 60:
        assert (ids != 0).sum() > 0.5 * min(n, t)
        assert (ids == sc["truth"]).mean() > 0.9


def test_general_assignment_tail_matches_oracle_too():
    """Frames with more than 1024 candidates leave the one-workgroup tail for the two-kernel one (component lists + one solver
    thread per component).  Here at a size that needs it; forced onto the small frames of the other parity tests by the `general`
    path of their `paths` marker (SA_FLAG_GENERAL_TAIL, tests/conftest.py)."""
    rng = np.random.default_rng(5)
    sc = synth.sort_scene(rng, 1500, 1300, canvas=(6000.0, 4000.0), oriented=True)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, max_idle_epochs=5)
    ids, ref = check_sort(cfg, sc)
    assert (ids != 0).sum() > 900


def test_random_crowd_frames_beyond_1024_tracks_match_the_oracle():
    """The many-workgroup tail's MIDDLE tier on what it is for: crowds beyond 1024 tracks under thresholds from 0.1 to 0.3, i.e. dozens
    to a hundred components of 3 to 60 rows per frame — gathered from the per-root row lists, built one edge per lane (up to 64
    edges) or through the hash table (more), served as their queue entries land.  Random sizes, canvases and jitter; every frame's ids
    against the oracle, and two reruns of the staged frame (the state a frame leaves behind must be as clean as it found it)."""
    rng = np.random.default_rng(2024)
    for it in range(12):
        n, t = int(rng.integers(300, 1500)), int(rng.integers(1030, 2600))
        canvas = (float(rng.uniform(700, 2600)), float(rng.uniform(600, 1600)))
        thr = float(rng.choice([0.1, 0.15, 0.2, 0.3]))
        sc = synth.sort_scene(rng, t, n, canvas=canvas, pos_sigma=float(rng.uniform(4.0, 14.0)))
        # (up to 2048 detections x 2048 tracks the default engine takes the ONE-workgroup tail — two columns, beyond 1024 detections also two
        # rows per thread: those frames run on both tails)
        both = ((n <= 2048 and t <= 2048) or (n <= 1024 and t <= 4096)) and not (abi.EXTRA_FLAGS & abi.SA_FLAG_GENERAL_TAIL)
        ref = None
        for flags in ((0, abi.SA_FLAG_GENERAL_TAIL) if both else (0,)):
          cfg = abi.make_config(positional="iou", positional_threshold=thr, max_idle_epochs=5, flags=flags)
          eng = Engine(cfg)
          try:
            tracks = abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"])
            eng.upsert(0, tracks)
            det = abi.make_detections(sc["det_boxes"])
            ids, votes = eng.associate(0, 1, det)
            if ref is None:
                ref = O.associate(cfg, tracks, 1, det, want_matrices=False)
            np.testing.assert_array_equal(ids, ref["track_id"], err_msg=f"frame {it}: {n} x {t}, threshold {thr}, flags {flags:#x}")
            np.testing.assert_array_equal(votes, ref["voting_type"])
            for _ in range(2):
                eng.batch_run()
                eng.batch_sync()
                np.testing.assert_array_equal(eng.batch_fetch(0, n)[0], ids, err_msg=f"frame {it} rerun")
          finally:
            eng.close()


@pytest.mark.paths("general")
def test_state_kept_clean_across_frames_of_changing_size():
    """Edge counters, row duals and the union-find forest are not reset at the start of a frame: the assignment tail leaves
    them clean (k_slot_init only after a reallocation).  One engine, one slot, frames whose N and T grow, shrink and cross
    the 1024-row boundary between the two tails: every frame must match the oracle."""
    rng = np.random.default_rng(77)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, max_idle_epochs=5)
    eng = Engine(cfg)
    try:
        prev_t = 0
        for f, (n, t) in enumerate([(300, 320), (1300, 1200), (90, 1200), (1100, 1250), (1024, 1250), (5, 1250), (700, 1300)]):
            sc = synth.sort_scene(rng, t, n, canvas=(5000.0, 3000.0), oriented=(f % 2 == 1))
            # tracks accumulate in the engine's table: upsert only the new ids, replace the boxes of the old ones
            tracks = abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"])
            eng.upsert(0, tracks)
            assert eng.count(0) == max(prev_t, t)
            if t < prev_t:
                eng.remove(0, np.arange(t + 1, prev_t + 1, dtype=np.uint64))
            prev_t = t
            det = abi.make_detections(sc["det_boxes"])
            ids, votes = eng.associate(0, 1, det)
            ref = O.associate(cfg, tracks, 1, det)
            np.testing.assert_array_equal(ids, ref["track_id"], err_msg=f"frame {f} ({n} x {t})")
            np.testing.assert_array_equal(votes, ref["voting_type"])
            # and again on the same staged frame: a second run must find the state as clean as the first
            eng.batch_run()
            eng.batch_sync()
            ids2, _ = eng.batch_fetch(0, n)
            np.testing.assert_array_equal(ids2, ref["track_id"], err_msg=f"frame {f} rerun")
    finally:
        eng.close()


@pytest.mark.paths("separate_resolve", "euclid_valu", "euclid_mfma")
@pytest.mark.parametrize("visual,thr", [("cosine", 0.2), ("euclidean", 0.5)])
def test_vote_words_rearmed_across_frames(visual, thr):
    """One observation per track, at most 1024 candidates and tracks: the contraction reduces the BestFit vote into one 64-bit word
    per candidate and per track (atomic minima; the euclidean kernel does the same) and the one-workgroup tail reads AND re-arms
    them; bigger frames go through the per-tile partials (euclidean: the weight matrix and k_bestfit_tile) and the resolve launch.  One engine, frames that cross both boundaries in both directions, every frame run
    twice: each answer must match the oracle (a word left dirty would leak a verdict into the next frame)."""
    rng = np.random.default_rng(4242)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual=visual, visual_threshold=thr, feature_len=96,
                          max_observations=1, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                          max_idle_epochs=5)
    eng = Engine(cfg)
    try:
        prev_t = 0
        for f, (n, t) in enumerate([(200, 220), (1100, 300), (300, 320), (400, 1100), (64, 1100), (1024, 1024), (10, 700), (900, 1000)]):
            sc = synth.visual_scene(rng, t, n, 96, 1, canvas=(2400.0, 1600.0), new_fraction=0.15)
            tracks = abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"], feat_present=sc["track_present"])
            det = abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"])
            eng.upsert(0, tracks)
            if t < prev_t:
                eng.remove(0, np.arange(t + 1, prev_t + 1, dtype=np.uint64))
            prev_t = t
            assert eng.count(0) == t
            ids, votes = eng.associate(0, 1, det)
            ref = O.associate(cfg, tracks, 1, det)
            np.testing.assert_array_equal(ids, ref["track_id"], err_msg=f"frame {f} ({n} x {t})")
            np.testing.assert_array_equal(votes, ref["voting_type"])
            eng.batch_run()
            eng.batch_sync()
            ids2, votes2 = eng.batch_fetch(0, n)
            np.testing.assert_array_equal(ids2, ref["track_id"], err_msg=f"frame {f} rerun")
            np.testing.assert_array_equal(votes2, ref["voting_type"])
    finally:
        eng.close()


def test_two_engines_of_one_process_run_different_paths():
    """The path switches are bits of sa_config.flags, not process-wide environment: a default engine (one-workgroup tail, lean frames,
    vote words) and one pinned to the general tail + preparation blocks + a separate resolve launch live side by side, take turns
    frame by frame, show different launches in their profiles and give the oracle's answers both."""
    rng = np.random.default_rng(808)
    mk = lambda flags: abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=64,  # noqa: E731
                                       max_observations=1, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                                       max_idle_epochs=5, flags=flags | abi.SA_FLAG_PROFILE)
    cfg_a = mk(0)
    cfg_b = mk(abi.SA_FLAG_GENERAL_TAIL | abi.SA_FLAG_NEVER_LEAN | abi.SA_FLAG_SEPARATE_RESOLVE)
    ea, eb = Engine(cfg_a), Engine(cfg_b)
    try:
        for f in range(3):
            sc = synth.visual_scene(rng, 230 + 10 * f, 200, 64, 1, canvas=(1600.0, 900.0), new_fraction=0.15)
            tracks = abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"], feat_present=sc["track_present"])
            det = abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"])
            ref = O.associate(cfg_a, tracks, 1, det)
            for eng in (ea, eb):
                eng.upsert(0, tracks)
                ids, votes = eng.associate(0, 1, det)
                np.testing.assert_array_equal(ids, ref["track_id"])
                np.testing.assert_array_equal(votes, ref["voting_type"])
        pa, pb = ea.profile_read(), eb.profile_read()
        if abi.EXTRA_FLAGS == 0:
            assert "k_assign_small" in pa and "k_assign_solve" not in pa and "k_bestfit_resolve" not in pa
        assert "k_assign_solve" in pb and "k_assign_label" in pb and "k_assign_small" not in pb and "k_bestfit_resolve" in pb
    finally:
        ea.close()
        eb.close()


def test_features_from_a_pinned_block_give_the_same_answers():
    """sa_host_alloc: a feats pointer inside such a block is DMA'd in place (no staging copy).  Same answers as from pageable
    memory, frame after frame, also when the block is rewritten between frames and when only part of it is used."""
    rng = np.random.default_rng(31)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=64,
                          max_observations=1, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                          max_idle_epochs=5)
    eng = Engine(cfg)
    block = eng.host_block((400, 64))
    try:
        for n, t in [(300, 320), (400, 320), (17, 330)]:
            sc = synth.visual_scene(rng, t, n, 64, 1, canvas=(1600.0, 900.0), new_fraction=0.1)
            tracks = abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"], feat_present=sc["track_present"])
            eng.upsert(0, tracks)
            block[:n] = sc["det_feats"]
            pinned = abi.make_detections(sc["det_boxes"], feats=block[:n], feat_quality=sc["det_quality"])
            pageable = abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"])
            ids_p, votes_p = eng.associate(0, 1, pinned)
            ids, votes = eng.associate(0, 1, pageable)
            ref = O.associate(cfg, tracks, 1, pageable)
            np.testing.assert_array_equal(ids_p, ref["track_id"])
            np.testing.assert_array_equal(votes_p, ref["voting_type"])
            np.testing.assert_array_equal(ids, ids_p)
            np.testing.assert_array_equal(votes, votes_p)
    finally:
        eng.host_free(block)
        eng.close()


@pytest.mark.parametrize("k", [2, 1])
def test_graph_replay_gives_the_same_answers(k):
    """SA_FLAG_GRAPH: the per-frame launches are captured once and replayed while the staged set is unchanged, re-captured when
    it changes (new frame size, re-allocated buffers).  Same answers as the eager pipeline, frame after frame.  k = 1: the vote
    words (re-armed by the tail inside the captured graph) instead of partials + resolve."""
    rng = np.random.default_rng(9)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=64,
                          max_observations=k, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                          max_idle_epochs=5, flags=abi.SA_FLAG_GRAPH)
    eng = Engine(cfg)
    try:
        for n, t in [(120, 150), (120, 150), (300, 310), (80, 310)]:
            sc = synth.visual_scene(rng, t, n, 64, k, canvas=(1200.0, 800.0), new_fraction=0.1)
            tracks = abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"], feat_present=sc["track_present"])
            det = abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"])
            eng.upsert(0, tracks)
            ids, votes = eng.associate(0, 1, det)
            ref = O.associate(cfg, tracks, 1, det)
            np.testing.assert_array_equal(ids, ref["track_id"])
            np.testing.assert_array_equal(votes, ref["voting_type"])
            for _ in range(3):  # replays of the captured graph
                eng.batch_run()
            eng.batch_sync()
            ids2, votes2 = eng.batch_fetch(0, n)
            np.testing.assert_array_equal(ids2, ref["track_id"])
    finally:
        eng.close()


def test_graph_replay_with_device_upkeep_of_a_visual_engine():
    """SA_FLAG_GRAPH on a VisualSORT engine whose frames are LEAN (one observation per track, vote words: the preparation blocks stay
    out of the first phase) with sa_tracks_apply after every frame: the feature-bank step reads the candidates' padded rows and norms,
    which a replayed lean frame has NOT prepared — the engine must prepare them on demand on EVERY frame, replays included (round 2
    skipped that from the second replay on and wrote the norms of an older frame into the bank).  Against an eager engine fed the same
    frames: ids, predicted boxes and the banks' rows + squared norms (through the next frame's cosines) identical."""
    import ctypes as C

    rng = np.random.default_rng(41)
    d, n = 64, 90
    engines = []
    try:
        for flags in (abi.SA_FLAG_GRAPH, 0):
            cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.3, feature_len=d,
                                  max_observations=1, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                                  max_idle_epochs=5, flags=flags)
            engines.append((cfg, Engine(cfg)))
        ident = synth.reid_identities(rng, n, d)
        world = synth.dense_boxes(rng, n, (1500.0, 1000.0))
        u64p, bp = C.POINTER(C.c_uint64), C.POINTER(abi.sa_box)
        next_id = 1
        for frame in range(7):
            world = synth.jitter_boxes(rng, world, 1.5)
            feats = synth.observe(rng, ident, 0.02) * np.float32(1.0 + 0.1 * frame)  # the norms change from frame to frame
            det = abi.make_detections(world, feats=feats, feat_quality=np.full(n, 0.9, np.float32))
            outs = []
            for cfg, eng in engines:
                ids, votes = eng.associate(7, frame + 1, det)
                new_ids = np.where(ids == 0, next_id + np.arange(n), 0).astype(np.uint64)
                pred = np.zeros(n, abi.BOX_DTYPE)
                rc = eng.lib.sa_tracks_apply(eng.h, 0, new_ids.ctypes.data_as(u64p), C.cast(pred.ctypes.data, bp))
                assert rc == 0, eng.lib.sa_last_error(eng.h)
                outs.append((ids, votes, pred, eng.order(7)))
            next_id += n
            (ia, va, pa, oa), (ib, vb, pb, ob) = outs
            np.testing.assert_array_equal(ia, ib, err_msg=f"frame {frame}")
            np.testing.assert_array_equal(va, vb)
            np.testing.assert_array_equal(pa, pb)
            np.testing.assert_array_equal(oa, ob)
            if frame >= 2:
                assert (va == abi.SA_VOTE_VISUAL).sum() > 0.8 * n   # the banks work: the visual vote decides
        # the banks themselves, row for row
        fp = C.POINTER(C.c_float)
        for tid in engines[0][1].order(7)[:40]:
            rows = []
            for cfg, eng in engines:
                ft = np.zeros((1, d), np.float32)
                assert eng.lib.sa_tracks_get_state(eng.h, 7, int(tid), None, None, None, None, ft.ctypes.data_as(fp)) == 0
                rows.append(ft)
            np.testing.assert_array_equal(rows[0], rows[1])
    finally:
        for _, eng in engines:
            eng.close()


def test_device_upkeep_refuses_tracks_without_state():
    """sa_tracks_apply steps the Kalman filter of the winner: a track that was upserted with the 5 x 5 projection only has no
    full state on the device — the call must say so instead of stepping garbage; after sa_tracks_set_state it works."""
    import ctypes as C

    rng = np.random.default_rng(3)
    sc = synth.sort_scene(rng, 20, 20, canvas=(600.0, 400.0))
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, max_idle_epochs=5)
    eng = Engine(cfg)
    try:
        eng.upsert(0, abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"]))
        ids, _ = eng.associate(0, 1, abi.make_detections(sc["det_boxes"]))
        assert (ids != 0).sum() > 10
        new_ids = np.where(ids == 0, 1000 + np.arange(20), 0).astype(np.uint64)
        pred = np.zeros(20, abi.BOX_DTYPE)
        u64p, bp, fp = C.POINTER(C.c_uint64), C.POINTER(abi.sa_box), C.POINTER(C.c_float)
        rc = eng.lib.sa_tracks_apply(eng.h, 0, new_ids.ctypes.data_as(u64p), C.cast(pred.ctypes.data, bp))
        assert rc == abi.SA_ERR_STATE and b"without a Kalman state" in eng.lib.sa_last_error(eng.h)
        # seed every track with a state (initiate from its box: mean = box, diagonal covariance), then the same call goes through
        for tid, b in zip(sc["track_ids"], sc["track_boxes"]):
            mean = np.array([b["xc"], b["yc"], 0.0, b["aspect"], b["height"], 0, 0, 0, 0, 0], np.float32)
            cov = np.diag(np.full(10, 4.0, np.float32)).astype(np.float32)
            assert eng.lib.sa_tracks_set_state(eng.h, 0, int(tid), mean.ctypes.data_as(fp), cov.ctypes.data_as(fp), None) == 0
        rc = eng.lib.sa_tracks_apply(eng.h, 0, new_ids.ctypes.data_as(u64p), C.cast(pred.ctypes.data, bp))
        assert rc == 0, eng.lib.sa_last_error(eng.h)
        assert eng.count(0) == 20 + int((ids == 0).sum())
        # a merged track's predicted box sits between its old box and the detection that continued it
        k = int(np.nonzero(ids != 0)[0][0])
        tb = sc["track_boxes"][int(ids[k]) - 1]
        lo, hi = min(tb["xc"], sc["det_boxes"][k]["xc"]) - 1e-3, max(tb["xc"], sc["det_boxes"][k]["xc"]) + 1e-3
        assert lo <= pred[k]["xc"] <= hi
    finally:
        eng.close()


@pytest.mark.paths("general")
def test_sort_iou_constraints_and_idle_epochs():
    rng = np.random.default_rng(7)
    sc = synth.sort_scene(rng, 200, 220, canvas=(1200.0, 800.0))
    sc["track_epochs"] = rng.integers(0, 9, 200).astype(np.uint64)
    cfg = abi.make_config(positional="iou", positional_threshold=0.2, max_idle_epochs=4, constraints=[(1, 0.05), (2, 0.5), (5, 1.5)])
    check_sort(cfg, sc, epoch=8)


@pytest.mark.paths("general", "never_lean")
def test_sort_maha_parity():
    rng = np.random.default_rng(21)
    sc = synth.sort_scene(rng, 180, 200, canvas=(1500.0, 900.0))
    kf = kf_states(rng, sc["track_boxes"])
    sc["det_boxes"] = synth.jitter_boxes(rng, kf[0], 2.0)[rng.permutation(180)]
    sc["det_boxes"] = np.concatenate([sc["det_boxes"], synth.dense_boxes(rng, 20, (1500.0, 900.0))])
    cfg = abi.make_config(positional="maha", positional_min_confidence=0.05, max_idle_epochs=5)
    ids, ref = check_sort(cfg, sc, kf=kf)
    assert (ids != 0).sum() > 100


def random_spd(rng, diag, corr=0.7):
    """A symmetric positive definite matrix with the given diagonal and real off-diagonal mass: D^1/2 R D^1/2, R a random correlation
    matrix whose off-diagonal entries reach +-corr (f32, symmetric bit for bit)."""
    n = len(diag)
    g = rng.standard_normal((n, n + 2))
    r = g @ g.T
    d = np.sqrt(np.diag(r))
    r = r / d[:, None] / d[None, :]
    r = np.eye(n) + corr * (r - np.eye(n))
    sd = np.sqrt(np.asarray(diag, np.float64))
    c = (sd[:, None] * r * sd[None, :]).astype(np.float32)
    return np.triu(c) + np.triu(c, 1).T


@pytest.mark.paths("general", "never_lean")
def test_sort_maha_off_diagonal_covariances():
    """The 5 x 5 Cholesky + forward substitution behind every Mahalanobis cell (kalman_2d_box.rs:150-170) on covariances WITH
    off-diagonal mass — the reference's own filter keeps them diagonal, so every other test multiplies zeros in the inner
    loops of sa_maha_prepare / sa_maha_cell, but sa_tracks_upsert accepts any kf_cov: cells bit-identical to or_positional_metric; a
    covariance whose pivot is not positive poisons its track's cells with NaN on both sides (the reference panics there)."""
    rng = np.random.default_rng(211)
    sc = synth.sort_scene(rng, 180, 200, canvas=(1500.0, 900.0))
    boxes, m5, c25 = kf_states(rng, sc["track_boxes"])
    c25 = c25.copy()
    for i in range(len(c25)):
        base = c25[i].reshape(5, 5)
        c25[i] = random_spd(rng, np.diag(base) * rng.uniform(0.5, 4.0, 5), corr=rng.uniform(0.2, 0.9)).ravel()
    off = c25.reshape(-1, 5, 5) - np.stack([np.diag(np.diag(c.reshape(5, 5))) for c in c25])
    assert (np.abs(off) > 0).mean() > 0.7
    for i in (5, 77, 140):
        c25[i] = (-1.0e6 * np.eye(5, dtype=np.float32)).ravel()      # a non-positive first pivot
    c25[33] = random_spd(rng, np.full(5, 4.0), corr=0.5).ravel()
    c25[33].reshape(5, 5)[2, 2] = -1.0e4                             # ... and one that fails at the third
    sc["det_boxes"] = synth.jitter_boxes(rng, boxes, 2.0)[rng.permutation(180)]
    sc["det_boxes"] = np.concatenate([sc["det_boxes"], synth.dense_boxes(rng, 20, (1500.0, 900.0))])
    cfg = abi.make_config(positional="maha", positional_min_confidence=0.05, max_idle_epochs=5)
    ids, ref = check_sort(cfg, sc, kf=(boxes, m5, c25), require_ids=False)
    assert (ids != 0).sum() > 60
    # the poisoned tracks: their whole column is NaN wherever the pair passes too_far (checked against the oracle above), and nobody wins them
    bad = sc["track_ids"][[5, 77, 140, 33]]
    assert not np.isin(ids, bad).any()


def test_device_upkeep_steps_full_covariances_like_the_oracle():
    """sa_tracks_set_state with full 10 x 10 covariances carrying position-position AND position-velocity cross terms, one
    association, the device-side Kalman step (sa_tracks_apply: predict + update, kalman_2d_box.rs:122-148 / 186-232), then the next
    frame's Mahalanobis cells: bit-identical to the oracle's filter stepped on the same states."""
    L = O.lib()
    rng = np.random.default_rng(212)
    n = 60
    sc = synth.sort_scene(rng, n, n, canvas=(900.0, 700.0))
    ids0 = sc["track_ids"]
    boxes, m5, _ = kf_states(rng, sc["track_boxes"])
    mean = np.zeros((n, 10), np.float32)
    cov = np.zeros((n, 100), np.float32)
    for i in range(n):
        mean[i, :5] = m5[i]
        mean[i, 5:] = rng.normal(0, 0.5, 5).astype(np.float32)
        h = float(m5[i, 4])
        d = np.array([(h / 20) ** 2 * 4] * 2 + [1e-3, 1e-3, (h / 20) ** 2 * 4] + [(h / 160) ** 2 * 8] * 2 + [1e-5, 1e-5, (h / 160) ** 2 * 8])
        cov[i] = random_spd(rng, d, corr=0.6).ravel()
    cfg = abi.make_config(positional="maha", positional_min_confidence=0.05, max_idle_epochs=5)
    det1 = synth.jitter_boxes(rng, boxes, 1.5)
    det2 = synth.jitter_boxes(rng, det1, 1.5)
    fp, u64p, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(abi.sa_box)
    eng = Engine(cfg)
    try:
        tr = abi.make_tracks(ids0, boxes, sc["track_epochs"], kf_mean=mean[:, :5].copy(), kf_cov=cov.reshape(n, 10, 10)[:, :5, :5].reshape(n, 25).copy())
        eng.upsert(0, tr)
        for i, tid in enumerate(ids0):
            assert eng.lib.sa_tracks_set_state(eng.h, 0, int(tid), mean[i].ctypes.data_as(fp), cov[i].ctypes.data_as(fp), None) == 0
        ids1, _ = eng.associate(0, 1, abi.make_detections(det1))
        ref1 = O.associate(cfg, tr, 1, abi.make_detections(det1))
        pos1 = eng.tap_positional()
        m1 = ~np.isnan(pos1)
        np.testing.assert_array_equal(np.isnan(pos1), np.isnan(ref1["positional"]))
        np.testing.assert_array_equal(pos1.view(np.uint32)[m1], ref1["positional"].view(np.uint32)[m1])
        assert (ids1 != 0).sum() > n // 2
        new_ids = np.where(ids1 == 0, 5000 + np.arange(n), 0).astype(np.uint64)
        pred = np.zeros(n, abi.BOX_DTYPE)
        assert eng.lib.sa_tracks_apply(eng.h, 0, new_ids.ctypes.data_as(u64p), C.cast(pred.ctypes.data, bp)) == 0, eng.lib.sa_last_error(eng.h)
        # the oracle's filter on the same states: winners step (predict + update with their detection), the others stay, new tracks start
        row = {int(t): k for k, t in enumerate(ids0)}
        t_ids, t_boxes, t_ep = list(ids0), boxes.copy(), np.asarray(sc["track_epochs"], np.uint64).copy()
        t_mean, t_cov = mean.copy(), cov.copy()
        add_ids, add_boxes, add_mean, add_cov = [], [], [], []
        for i in range(n):
            sb = np.zeros(1, abi.BOX_DTYPE)
            ob = det1[i : i + 1].copy()
            if ids1[i]:
                k = row[int(ids1[i])]
                L.or_make_prediction(PW, VW, 1, O.fptr(t_mean[k]), O.fptr(t_cov[k]), O.box_ptr(ob), O.box_ptr(sb))
                t_boxes[k] = sb[0]
                t_ep[k] = 1
                for f in ("xc", "yc", "aspect", "height"):
                    assert pred[i][f] == sb[0][f], (i, f)
            else:
                m, c = np.zeros(10, np.float32), np.zeros(100, np.float32)
                L.or_make_prediction(PW, VW, 0, O.fptr(m), O.fptr(c), O.box_ptr(ob), O.box_ptr(sb))
                add_ids.append(int(new_ids[i])); add_boxes.append(sb[0]); add_mean.append(m); add_cov.append(c)
        all_ids = np.array(t_ids + add_ids, np.uint64)
        all_boxes = np.concatenate([t_boxes, np.array(add_boxes, abi.BOX_DTYPE)]) if add_ids else t_boxes
        all_ep = np.concatenate([t_ep, np.ones(len(add_ids), np.uint64)])
        all_mean = np.concatenate([t_mean, np.array(add_mean, np.float32).reshape(-1, 10)])
        all_cov = np.concatenate([t_cov, np.array(add_cov, np.float32).reshape(-1, 100)])
        t2 = len(all_ids)
        tr2 = abi.make_tracks(all_ids, all_boxes, all_ep, kf_mean=all_mean[:, :5].copy(),
                              kf_cov=all_cov.reshape(t2, 10, 10)[:, :5, :5].reshape(t2, 25).copy())
        ids2, _ = eng.associate(0, 2, abi.make_detections(det2))
        ref2 = O.associate(cfg, tr2, 2, abi.make_detections(det2))
        pos2 = eng.tap_positional()
        np.testing.assert_array_equal(np.isnan(pos2), np.isnan(ref2["positional"]))
        m2 = ~np.isnan(pos2)
        assert m2.sum() > n
        np.testing.assert_array_equal(pos2.view(np.uint32)[m2], ref2["positional"].view(np.uint32)[m2])
    finally:
        eng.close()


def test_sort_maha_oriented_parity():
    rng = np.random.default_rng(22)
    sc = synth.sort_scene(rng, 90, 90, canvas=(900.0, 900.0), oriented=True)
    kf = kf_states(rng, sc["track_boxes"])
    sc["det_boxes"] = synth.jitter_boxes(rng, kf[0], 2.0, angle_sigma=0.01)
    cfg = abi.make_config(positional="maha", max_idle_epochs=5)
    check_sort(cfg, sc, kf=kf)


def visual_run(cfg, sc, epoch=1, kf=None, own_area=None, det_present=None, pos_mode=None):
    """pos_mode None: the tapped engine's own mode (eager) under today's gate; "eager" / "lazy": that mode forced, its edges under
    check_edges' mode proof (forced lazy outside lazy_form: eager edges)."""
    tb = sc["track_boxes"]
    kw = {}
    if kf is not None:
        tb, m5, c25 = kf
        kw = dict(kf_mean=m5, kf_cov=c25)
    tracks = abi.make_tracks(sc["track_ids"], tb, sc["track_epochs"], feats=sc["track_feats"], feat_present=sc["track_present"], **kw)
    det = abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"], own_area=own_area, feat_present=det_present)
    ref = O.associate(cfg, tracks, epoch, det)
    cfg.flags |= abi.SA_FLAG_TAP | POS_MODE_FLAGS.get(pos_mode, 0)
    eng = Engine(cfg)
    try:
        eng.upsert(0, tracks)
        ids, votes = eng.associate(0, epoch, det)
        # the timed launches' own output first (the matrix taps below re-launch kernels)
        check_edges(eng, ref["quantised"], thr_q_of(cfg), mode=mode_of(cfg, det.n, tracks.n), prove=pos_mode is not None,
                    pos_ref=ref["positional"])
        euclid = cfg.visual_kind == abi.SA_VIS_EUCLIDEAN
        check_votes(cfg, eng, ref["visual"], tol_abs=0.0 if euclid else 1e-5, tol_rel=1e-5 if euclid else 0.0)
        pos = eng.tap_positional()
        vis = eng.tap_visual()
    finally:
        eng.close()
    return ids, votes, pos, vis, ref


# Borderline bookkeeping of check_visual: a visual cell within tolerance of the is_ok threshold may be present on one side and absent
# on the other; the vote can then legitimately differ in the rows / columns that cell touches.  Every such case is counted, bounded
# per frame, and the id comparison is narrowed to the untouched rows instead of being skipped (test_borderline_cells_stay_rare).
BORDERLINE = {"frames": 0, "frames_with_borderline": 0, "cells": 0, "rows_excused": 0, "rows_checked": 0}


def compare_visual(cfg, ids, votes, pos, vis, ref, tol_abs=1e-5, tol_rel=0.0):
    np.testing.assert_array_equal(np.isnan(pos), np.isnan(ref["positional"]))
    np.testing.assert_array_equal(pos.view(np.uint32)[~np.isnan(pos)], ref["positional"].view(np.uint32)[~np.isnan(pos)])
    rv = ref["visual"]
    both = ~np.isnan(vis) & ~np.isnan(rv)
    err = np.abs(vis[both] - rv[both])
    assert (err <= tol_abs + tol_rel * np.abs(rv[both])).all(), err.max()
    # cells present on one side only must sit within tolerance of the is_ok threshold
    mism = np.isnan(vis) != np.isnan(rv)
    BORDERLINE["frames"] += 1
    n = len(ids)
    excused = np.zeros(n, bool)
    if mism.any():
        thr_w = 1.0 - cfg.visual_threshold if cfg.visual_kind == abi.SA_VIS_COSINE else cfg.visual_threshold
        v = np.where(np.isnan(vis), rv, vis)[mism]
        assert (np.abs(v - thr_w) <= 2 * tol_abs + tol_rel * abs(thr_w)).all(), "present/absent mask differs away from the threshold"
        cells = int(mism.sum())
        assert cells <= 2 + 1e-5 * mism.size, f"{cells} borderline cells of {mism.size}: the threshold is not a tolerance problem any more"
        BORDERLINE["frames_with_borderline"] += 1
        BORDERLINE["cells"] += cells
        # a borderline cell (row q, track t) may move the verdict of row q, of every row whose winner (on either side) is t, and
        # — through the exclusion of t from the positional vote — of the rows of t's positional component: excuse the rows that
        # touch the cell's row or column on either side; everything else must still be identical
        rows, cols = np.nonzero(mism.any(axis=2) if mism.ndim == 3 else mism)
        excused[np.unique(rows)] = True
        for c in np.unique(cols):
            tid = ref["_track_ids"][c]
            excused |= (ids == tid) | (ref["track_id"] == tid)
            excused |= ~np.isnan(pos[:, c])
    BORDERLINE["rows_excused"] += int(excused.sum())
    BORDERLINE["rows_checked"] += int((~excused).sum())
    np.testing.assert_array_equal(ids[~excused], ref["track_id"][~excused])
    np.testing.assert_array_equal(votes[~excused], ref["voting_type"][~excused])


def check_visual(cfg, sc, tol_abs=1e-5, tol_rel=0.0, **kw):
    ids, votes, pos, vis, ref = visual_run(cfg, sc, **kw)
    ref["_track_ids"] = sc["track_ids"]
    compare_visual(cfg, ids, votes, pos, vis, ref, tol_abs, tol_rel)
    return ids, votes, ref


@pytest.mark.paths("general", "never_lean", "bestfit_tile", "separate_resolve", "row_tiles", "xcd_tiles", "staged_loop", "no_yield")
@pytest.mark.parametrize("fused", [abi.SA_FLAG_SEPARATE_FRAME, abi.SA_FLAG_FUSED_FRAME, 0], ids=["separate_launches", "fused_frame_launch", "default"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("n,t,d", [(150, 170, 512), (70, 33, 100), (129, 257, 36), (300, 280, 64)])
def test_visual_cosine_parity(k, n, t, d, fused):
    _visual_cosine_parity(k, n, t, d, fused, "eager" if k == 1 else None)


@pytest.mark.paths("general", "never_lean", "bestfit_tile", "separate_resolve", "row_tiles", "xcd_tiles", "staged_loop", "no_yield")
@pytest.mark.parametrize("fused", [abi.SA_FLAG_SEPARATE_FRAME, abi.SA_FLAG_FUSED_FRAME, 0], ids=["separate_launches", "fused_frame_launch", "default"])
@pytest.mark.parametrize("n,t,d", [(150, 170, 512), (70, 33, 100), (129, 257, 36), (300, 280, 64)])
def test_visual_cosine_parity_lazy(n, t, d, fused):
    """test_visual_cosine_parity's one-observation frames with the positional stage forced lazy (general, bestfit_tile and
    separate_resolve have no lazy phase: eager edges, by check_edges' mode proof)."""
    _visual_cosine_parity(1, n, t, d, fused, "lazy")


def _visual_cosine_parity(k, n, t, d, fused, pos_mode):
    rng = np.random.default_rng(1000 + n + t + d + k)
    sc = synth.visual_scene(rng, t, n, d, k, canvas=(1500.0, 900.0), new_fraction=0.1)
    # ragged banks: some observations missing, some tracks too short, some candidates unusable
    pres = sc["track_present"]
    pres[rng.uniform(size=pres.shape) < 0.15] = 0
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=d,
                          max_observations=k, visual_min_votes=1, visual_minimal_track_length=1 if k == 1 else 2,
                          visual_minimal_quality_use=0.55, visual_minimal_area=3000.0, positional_min_confidence=0.1,
                          max_idle_epochs=5, flags=fused)
    ids, votes, ref = check_visual(cfg, sc, pos_mode=pos_mode)
    assert (votes == abi.SA_VOTE_VISUAL).sum() > 0
    assert (votes == abi.SA_VOTE_POSITIONAL).sum() > 0


@pytest.mark.paths("general", "never_lean", "row_tiles", "xcd_tiles", "no_yield")
@pytest.mark.parametrize("n,t,d", [(150, 170, 512), (70, 33, 96), (129, 257, 64), (300, 280, 64), (64, 96, 32), (65, 97, 32), (5, 3, 32), (200, 700, 32)])
def test_visual_cosine_parity_on_64x96_tiles(n, t, d):
    _visual_cosine_parity_on_64x96_tiles(n, t, d, "eager")


@pytest.mark.paths("general", "never_lean", "row_tiles", "xcd_tiles", "no_yield")
@pytest.mark.parametrize("n,t,d", [(150, 170, 512), (70, 33, 96), (129, 257, 64), (300, 280, 64), (64, 96, 32), (65, 97, 32), (5, 3, 32), (200, 700, 32)])
def test_visual_cosine_parity_on_64x96_tiles_lazy(n, t, d):
    _visual_cosine_parity_on_64x96_tiles(n, t, d, "lazy")


def _visual_cosine_parity_on_64x96_tiles(n, t, d, pos_mode):
    """The fused first phase's 64 x 96 tiles (what frames of 1.0 .. 1.5 rounds of 64 x 64 tiles take: sa_launch_frame_visual), pinned
    on small frames (gemm_plan 19): ragged edges in both directions, tiles whose third column block is empty or partial, the vote words
    of the timed launch against the oracle's matrix (check_votes inside visual_run), ids and vote types."""
    rng = np.random.default_rng(1900 + n + t + d)
    sc = synth.visual_scene(rng, t, n, d, 1, canvas=(1500.0, 900.0), new_fraction=0.1)
    pres = sc["track_present"]
    pres[rng.uniform(size=pres.shape) < 0.15] = 0
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=d,
                          max_observations=1, visual_min_votes=1, visual_minimal_track_length=1, visual_minimal_quality_use=0.55,
                          visual_minimal_area=3000.0, positional_min_confidence=0.1, max_idle_epochs=5, gemm_plan=19)
    ids, votes, ref = check_visual(cfg, sc, pos_mode=pos_mode)
    if n >= 64:
        assert (votes == abi.SA_VOTE_VISUAL).sum() > 0


def test_visual_cosine_1000_x_1500_takes_the_64x96_tiles_by_itself():
    """c2t's shape (384 tiles of 64 x 64 = one and a half rounds of the chip: the launch picks 256 tiles of 64 x 96), full size against
    the oracle; and the same frame with the 64 x 64 tiles pinned (gemm_plan 9): the same ids and vote types."""
    rng = np.random.default_rng(1501)
    n, t, d = 1000, 1500, 512
    sc = synth.visual_scene(rng, t, n, d, 1)
    out = []
    for plan in (None, 9):
        cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=d,
                              max_observations=1, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                              max_idle_epochs=5, gemm_plan=plan)
        ids, votes, pos, vis, ref = _full_size_visual(cfg, sc)
        compare_visual(cfg, ids, votes, pos, vis, ref)
        out.append((ids.copy(), votes.copy()))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])


@pytest.mark.paths("general", "bestfit_tile")
@pytest.mark.parametrize("n,t,d,k", [(1200, 1500, 64, 3), (900, 2300, 64, 2), (1500, 1100, 32, 5)])
def test_class_words_beyond_the_small_frames(n, t, d, k):
    """Banks of 2..5 observations (class words) on frames of more than 1024 detections or more than 2048 tracks: the one-workgroup tail's
    wider forms read a row's / column's K words twice (k_assign_small2) instead of holding them across the barrier — the timed launch's
    own votes, ids and vote types against the oracle; by the path markers also on the many-workgroup tail and through the weight matrix."""
    rng = np.random.default_rng(7000 + n + t + k)
    sc = synth.visual_scene(rng, t, n, d, k, canvas=(4000.0, 3000.0), new_fraction=0.1)
    pres = sc["track_present"]
    pres[rng.uniform(size=pres.shape) < 0.15] = 0
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=d,
                          max_observations=k, visual_min_votes=1, visual_minimal_track_length=2, visual_minimal_quality_use=0.55,
                          visual_minimal_area=3000.0, positional_min_confidence=0.1, max_idle_epochs=5)
    ids, votes, ref = check_visual(cfg, sc)
    assert (votes == abi.SA_VOTE_VISUAL).sum() > 100
    assert (votes == abi.SA_VOTE_POSITIONAL).sum() > 0


@pytest.mark.paths("general", "separate_resolve")
def test_visual_cosine_more_than_1024_detections():
    """N > 1024 (1100 detections, a fifth of them without a feature, against 900 tracks): the one-workgroup tail with two rows per thread
    (k_assign_small2) behind the fused first phase — or, by the path markers, its verdict-array form and the many-workgroup tail."""
    rng = np.random.default_rng(1300)
    sc = synth.visual_scene(rng, 900, 1100, 64, 1, canvas=(3000.0, 2000.0), new_fraction=0.15)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=64,
                          max_observations=1, visual_min_votes=1, visual_minimal_track_length=1, visual_minimal_quality_use=0.5,
                          positional_min_confidence=0.1, max_idle_epochs=5)
    dp = (rng.uniform(size=1100) > 0.2).astype(np.uint8)   # a fifth of the detections come without a feature: positional vote
    ids, votes, ref = check_visual(cfg, sc, det_present=dp)
    assert (votes == abi.SA_VOTE_VISUAL).sum() > 300
    assert (votes == abi.SA_VOTE_POSITIONAL).sum() > 50


@pytest.mark.paths("euclid_valu", "euclid_mfma", "staged_loop")
def test_visual_euclid_parity():
    rng = np.random.default_rng(77)
    sc = synth.visual_scene(rng, 120, 140, 256, 3, canvas=(1500.0, 900.0), new_fraction=0.1)
    cfg = abi.make_config(positional="iou", visual="euclidean", visual_threshold=0.6, feature_len=256, max_observations=3,
                          visual_min_votes=2, visual_minimal_track_length=1, positional_min_confidence=0.1, max_idle_epochs=5)
    check_visual(cfg, sc, tol_abs=1e-6, tol_rel=1e-5)


@pytest.mark.paths("euclid_valu", "euclid_mfma")
def test_visual_euclid_reference_bench_distribution():
    # features = 10*idx +- 0.01 (benches/simple_visual_sort_tracker.rs:135-141): the case a GEMM expansion cannot hold
    rng = np.random.default_rng(78)
    t = n = 100
    d = 128
    sc = synth.visual_scene(rng, t, n, d, 3, canvas=(3000.0, 3000.0))
    base = (10.0 * np.arange(t, dtype=np.float32))[:, None, None]
    sc["track_feats"] = (base + rng.uniform(-0.01, 0.01, (t, 3, d))).astype(np.float32)
    perm = (sc["truth"].astype(np.int64) - 1)
    sc["det_feats"] = (10.0 * perm[:, None] + rng.uniform(-0.01, 0.01, (n, d))).astype(np.float32)
    cfg = abi.make_config(positional="iou", visual="euclidean", visual_threshold=3.4e38, feature_len=d, max_observations=3,
                          visual_min_votes=1, positional_min_confidence=0.1, max_idle_epochs=5)
    ids, votes, ref = check_visual(cfg, sc, tol_abs=0.0, tol_rel=1e-5)
    np.testing.assert_array_equal(ids, sc["truth"])


def test_reference_default_visual_options():
    """The literal defaults of the reference (visual_sort/metric/builder.rs:26-42, options.rs:194-205): euclidean metric with threshold
    f32::MAX — EVERY cell with a usable feature pair is present and every (candidate, track) pair is a group of the BestFit vote —
    five observations per track, visual_minimal_track_length 3, one vote.  Ragged banks: a fifth of the observations missing, so some
    tracks are too short to vote at all."""
    rng = np.random.default_rng(83)
    n, t, d, k = 300, 280, 128, 5
    sc = synth.visual_scene(rng, t, n, d, k, canvas=(1500.0, 900.0), new_fraction=0.1)
    pres = sc["track_present"]
    pres[rng.uniform(size=pres.shape) < 0.2] = 0
    pres[:12] = 0
    pres[:12, :2] = 1  # twelve tracks with two observations: below the minimal track length
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="euclidean", visual_threshold=3.4028234663852886e38, feature_len=d,
                          max_observations=k, visual_min_votes=1, visual_minimal_track_length=3, positional_min_confidence=0.1, max_idle_epochs=2)
    ids, votes, ref = check_visual(cfg, sc, tol_abs=1e-6, tol_rel=1e-5)
    assert (votes == abi.SA_VOTE_VISUAL).sum() > 0.5 * n
    short = set(sc["track_ids"][:12].tolist())
    assert not (set(ids[votes == abi.SA_VOTE_VISUAL].tolist()) & short)  # a track below the minimal length wins nothing visually


def test_euclidean_engine_leaves_the_matrix_cores_when_the_expansion_is_ill_conditioned():
    """The matrix-core path for euclidean distances recomputes directly every cell its f32 expansion cannot hold to 1e-5; on the
    reference's own bench distribution (features 10 * idx +- 0.01: norms ~ 10^4 x the spread) that is nearly every cell, the frame
    reports it, and the engine runs the next frames on the vector-pipe kernel.  Every frame — the slow first one too — gives the
    oracle's distances and ids; and an ordinary ReID-like scene on a fresh engine stays on the matrix cores."""
    rng = np.random.default_rng(79)
    t = n = 192
    d = 128
    sc = synth.visual_scene(rng, t, n, d, 1, canvas=(3000.0, 3000.0))
    base = (10.0 * np.arange(t, dtype=np.float32))[:, None, None]
    sc["track_feats"] = (base + rng.uniform(-0.01, 0.01, (t, 1, d))).astype(np.float32)
    perm = (sc["truth"].astype(np.int64) - 1)
    cfg = abi.make_config(positional="iou", visual="euclidean", visual_threshold=3.4e38, feature_len=d, max_observations=1,
                          visual_min_votes=1, positional_min_confidence=0.1, max_idle_epochs=5, flags=abi.SA_FLAG_PROFILE)
    tracks = abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"], feat_present=sc["track_present"])
    eng = Engine(cfg)
    try:
        eng.upsert(0, tracks)
        kernels = []
        for f in range(4):
            sc["det_feats"] = (10.0 * perm[:, None] + rng.uniform(-0.01, 0.01, (n, d))).astype(np.float32)
            det = abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"])
            eng.profile_reset()
            ids, votes = eng.associate(0, 1, det)
            kernels.append(set(eng.profile_read()))
            vis = eng.tap_visual()
            ref = O.associate(cfg, tracks, 1, det)
            both = ~np.isnan(vis) & ~np.isnan(ref["visual"])
            assert both.all()
            assert (np.abs(vis - ref["visual"]) <= 1e-5 * np.abs(ref["visual"])).all(), f"frame {f}"
            np.testing.assert_array_equal(ids, ref["track_id"])
            np.testing.assert_array_equal(ids, sc["truth"])
        assert "k_frame_visual" in kernels[0], kernels          # the first frames: contraction tiles inside the heterogeneous launch
        assert "k_visual_cost" in kernels[-1] and "k_frame_visual" not in kernels[-1], kernels  # after the report: the vector-pipe kernel
    finally:
        eng.close()
    # The back-off is per SCENE and bounded by sa_config.euclid_backoff_frames: with 2, the ill-conditioned scene runs matrix cores /
    # vector pipe / vector pipe / matrix cores ... while an ordinary scene of the same engine never leaves the matrix cores.
    if not (abi.EXTRA_FLAGS & (abi.SA_FLAG_EUCLID_VALU | abi.SA_FLAG_EUCLID_MFMA)):
        cfg3 = abi.make_config(positional="iou", visual="euclidean", visual_threshold=3.4e38, feature_len=d, max_observations=1,
                               visual_min_votes=1, positional_min_confidence=0.1, max_idle_epochs=5, flags=abi.SA_FLAG_PROFILE, euclid_backoff_frames=2)
        sc1 = synth.visual_scene(rng, t, n, d, 1, canvas=(3000.0, 3000.0))
        tr1 = abi.make_tracks(sc1["track_ids"], sc1["track_boxes"], sc1["track_epochs"], feats=sc1["track_feats"], feat_present=sc1["track_present"])
        det1 = abi.make_detections(sc1["det_boxes"], feats=sc1["det_feats"], feat_quality=sc1["det_quality"])
        ref1 = O.associate(cfg3, tr1, 1, det1)
        eng = Engine(cfg3)
        try:
            eng.upsert(0, tracks)
            eng.upsert(1, tr1)
            seq0, seq1 = [], []
            for f in range(7):
                eng.profile_reset()
                ids, _ = eng.associate(0, 1, det)
                seq0.append("M" if "k_frame_visual" in eng.profile_read() else "V")
                np.testing.assert_array_equal(ids, sc["truth"])
                eng.profile_reset()
                ids1, _ = eng.associate(1, 1, det1)
                seq1.append("M" if "k_frame_visual" in eng.profile_read() else "V")
                np.testing.assert_array_equal(ids1, ref1["track_id"])
            assert "".join(seq0) == "MVVMVVM", seq0
            assert "".join(seq1) == "MMMMMMM", seq1
        finally:
            eng.close()
    sc2 = synth.visual_scene(rng, t, n, d, 1, canvas=(3000.0, 3000.0))
    cfg2 = abi.make_config(positional="iou", visual="euclidean", visual_threshold=0.6, feature_len=d, max_observations=1,
                           visual_min_votes=1, positional_min_confidence=0.1, max_idle_epochs=5, flags=abi.SA_FLAG_PROFILE)
    eng = Engine(cfg2)
    try:
        eng.upsert(0, abi.make_tracks(sc2["track_ids"], sc2["track_boxes"], sc2["track_epochs"], feats=sc2["track_feats"], feat_present=sc2["track_present"]))
        det = abi.make_detections(sc2["det_boxes"], feats=sc2["det_feats"], feat_quality=sc2["det_quality"])
        for _ in range(4):
            eng.profile_reset()
            eng.associate(0, 1, det)
            assert "k_frame_visual" in eng.profile_read()
    finally:
        eng.close()


def test_visual_maha_with_constraints_and_own_area():
    rng = np.random.default_rng(79)
    sc = synth.visual_scene(rng, 100, 110, 64, 2, canvas=(1200.0, 800.0), new_fraction=0.1)
    kf = kf_states(rng, sc["track_boxes"])
    own = rng.uniform(0.2, 1.0, 110).astype(np.float32)
    own[::7] = np.nan  # None
    dpres = (rng.uniform(size=110) > 0.1).astype(np.uint8)
    cfg = abi.make_config(positional="maha", visual="cosine", visual_threshold=0.3, feature_len=64, max_observations=2,
                          visual_min_votes=1, visual_minimal_own_area_percentage_use=0.5, constraints=[(1, 1.0)],
                          max_idle_epochs=3, positional_min_confidence=0.1)
    check_visual(cfg, sc, kf=kf, own_area=own, det_present=dpres)


@pytest.mark.paths("bestfit_tile", "separate_resolve")
def test_zero_feature_vectors_are_absent():
    rng = np.random.default_rng(80)
    sc = synth.visual_scene(rng, 20, 20, 32, 1, canvas=(800.0, 600.0))
    sc["det_feats"][3] = 0.0  # cosine -> 0/0 = NaN -> fails is_ok -> absent
    sc["track_feats"][5] = 0.0
    cfg = abi.make_config(positional="iou", visual="cosine", visual_threshold=-1.0, feature_len=32, max_observations=1,
                          max_idle_epochs=5)
    ids, votes, pos, vis, ref = visual_run(cfg, sc)
    assert np.isnan(vis[3]).all() and np.isnan(vis[:, 5]).all()
    np.testing.assert_array_equal(np.isnan(vis), np.isnan(ref["visual"]))
    np.testing.assert_array_equal(ids, ref["track_id"])


def test_empty_and_degenerate_frames():
    cfg = abi.make_config(positional="iou", max_idle_epochs=5)
    rng = np.random.default_rng(81)
    eng = Engine(cfg)
    try:
        boxes = synth.dense_boxes(rng, 10)
        # no tracks at all: everything is a new track
        ids, votes = eng.associate(0, 1, abi.make_detections(boxes))
        assert (ids == 0).all() and (votes == 0).all()
        eng.upsert(0, abi.make_tracks(np.arange(1, 11), boxes, np.zeros(10)))
        # no detections
        ids, votes = eng.associate(0, 1, abi.make_detections(boxes[:0]))
        assert len(ids) == 0
        ids, _ = eng.associate(0, 1, abi.make_detections(boxes))
        np.testing.assert_array_equal(ids, np.arange(1, 11))
        # other scene is isolated (compatible(): scene_id equality, sort.rs:251)
        ids, _ = eng.associate(5, 1, abi.make_detections(boxes))
        assert (ids == 0).all()
        assert eng.count(0) == 10 and eng.count(5) == 0
    finally:
        eng.close()


def test_bad_arguments_are_errors_not_aborts():
    cfg = abi.make_config(positional="iou")
    eng = Engine(cfg)
    try:
        b = synth.dense_boxes(np.random.default_rng(0), 3)
        bad = b.copy(); bad["height"][1] = 0.0
        with pytest.raises(EngineError) as ei:
            eng.associate(0, 1, abi.make_detections(bad))
        assert ei.value.code == abi.SA_ERR_BAD_ARG
        bad = b.copy(); bad["confidence"][0] = 1.5
        with pytest.raises(EngineError):
            eng.associate(0, 1, abi.make_detections(bad))
        with pytest.raises(EngineError):
            eng.upsert(0, abi.make_tracks([0, 1, 2], b, [0, 0, 0]))  # id 0
        with pytest.raises(EngineError) as ei:
            eng.remove(0, [42])
        assert ei.value.code == abi.SA_ERR_NOT_FOUND
    finally:
        eng.close()
    cfg2 = abi.make_config(positional="iou", visual="cosine", visual_threshold=2.0, feature_len=8)
    with pytest.raises(EngineError):
        Engine(cfg2)


def test_upsert_replace_remove_keep_order():
    rng = np.random.default_rng(82)
    cfg = abi.make_config(positional="iou", visual="cosine", visual_threshold=0.2, feature_len=40, max_observations=2, max_idle_epochs=50)
    sc = synth.visual_scene(rng, 50, 50, 40, 2, canvas=(900.0, 700.0))
    eng = Engine(cfg)
    try:
        first = slice(0, 30)
        eng.upsert(0, abi.make_tracks(sc["track_ids"][first], sc["track_boxes"][first], sc["track_epochs"][first],
                                      feats=sc["track_feats"][first], feat_present=sc["track_present"][first]))
        rest = slice(30, 50)
        eng.upsert(0, abi.make_tracks(sc["track_ids"][rest], sc["track_boxes"][rest], sc["track_epochs"][rest],
                                      feats=sc["track_feats"][rest], feat_present=sc["track_present"][rest]))
        np.testing.assert_array_equal(eng.order(0), sc["track_ids"])
        # replace a few rows in place (merge of a candidate into a stored track)
        upd = np.array([4, 17, 44])
        nb = synth.jitter_boxes(rng, sc["track_boxes"][upd], 1.0)
        nf = synth.observe(rng, sc["track_feats"][upd].reshape(-1, 40)).reshape(3, 2, 40)
        sc["track_boxes"][upd] = nb
        sc["track_feats"][upd] = nf
        sc["track_epochs"][upd] = 1
        eng.upsert(0, abi.make_tracks(sc["track_ids"][upd], nb, sc["track_epochs"][upd], feats=nf, feat_present=sc["track_present"][upd]))
        np.testing.assert_array_equal(eng.order(0), sc["track_ids"])
        # remove some: stable compaction keeps ascending-id order
        gone = np.array([3, 4, 20, 50], np.uint64)
        eng.remove(0, gone)
        keep = ~np.isin(sc["track_ids"], gone)
        np.testing.assert_array_equal(eng.order(0), sc["track_ids"][keep])
        tracks = abi.make_tracks(sc["track_ids"][keep], sc["track_boxes"][keep], sc["track_epochs"][keep],
                                 feats=sc["track_feats"][keep], feat_present=sc["track_present"][keep])
        det = abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"])
        ref = O.associate(cfg, tracks, 2, det)
        ids, votes = eng.associate(0, 2, det)
        np.testing.assert_array_equal(ids, ref["track_id"])
        np.testing.assert_array_equal(votes, ref["voting_type"])
        assert not np.isin(ids, gone).any()
    finally:
        eng.close()


@pytest.mark.paths("general", "never_lean")
def test_batched_scenes_match_single_scene_runs():
    rng = np.random.default_rng(83)
    cfg = abi.make_config(positional="iou", max_idle_epochs=5)
    sizes = [(60, 50), (1, 7), (130, 200), (33, 0), (0, 12), (257, 255)]
    scenes = [synth.sort_scene(rng, t, n, canvas=(1000.0, 800.0)) for n, t in sizes]
    eng = Engine(cfg)
    try:
        for s, sc in enumerate(scenes):
            eng.upsert(10 + s, abi.make_tracks(sc["track_ids"] + 1000 * s, sc["track_boxes"], sc["track_epochs"]))
        eng.batch_begin()
        dets = [abi.make_detections(sc["det_boxes"]) for sc in scenes]
        slots = [eng.batch_add(10 + s, 1, d) for s, d in enumerate(dets)]
        eng.batch_run()
        eng.batch_sync()
        for s, sc in enumerate(scenes):
            ids, votes = eng.batch_fetch(slots[s], dets[s].n)
            tracks = abi.make_tracks(sc["track_ids"] + 1000 * s, sc["track_boxes"], sc["track_epochs"])
            ref = O.associate(cfg, tracks, 1, dets[s], want_matrices=False)
            np.testing.assert_array_equal(ids, ref["track_id"])
            np.testing.assert_array_equal(votes, ref["voting_type"])
        # the same scene twice in one batch is a state error (one entry per scene, trackers/batch.rs)
        eng.batch_begin()
        eng.batch_add(10, 2, dets[0])
        with pytest.raises(EngineError):
            eng.batch_add(10, 2, dets[0])
    finally:
        eng.close()


@pytest.mark.parametrize("k,d,flags", [(1, 64, 0), (1, 64, abi.SA_FLAG_SEPARATE_FRAME), (1, 40, 0), (3, 64, 0)],
                         ids=["partials_fused", "partials_separate", "partials_padded", "bank3"])
@pytest.mark.paths("never_lean", "separate_resolve")
def test_batched_visual_scenes_match_single_scene_runs(k, d, flags):
    """Scenes of different sizes in ONE set of launches (grid.z = scene): every scene has its own tile grid of BestFit partials,
    tiles past a small scene's edge do nothing, and the answers are those of the oracle scene by scene."""
    rng = np.random.default_rng(91 + k + d)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=d,
                          max_observations=k, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                          max_idle_epochs=5, flags=flags)
    sizes = [(150, 170), (5, 3), (257, 70), (64, 300), (1, 1)]
    scenes = [synth.visual_scene(rng, t, n, d, k, canvas=(1200.0, 800.0), new_fraction=0.1) for n, t in sizes]
    eng = Engine(cfg)
    try:
        tracks = []
        for s, sc in enumerate(scenes):
            tr = abi.make_tracks(sc["track_ids"] + 1000 * s, sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"],
                                 feat_present=sc["track_present"])
            eng.upsert(20 + s, tr)
            tracks.append(tr)
        eng.batch_begin()
        dets = [abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"]) for sc in scenes]
        slots = [eng.batch_add(20 + s, 1, dd) for s, dd in enumerate(dets)]
        eng.batch_run()
        eng.batch_sync()
        for s in range(len(scenes)):
            ids, votes = eng.batch_fetch(slots[s], dets[s].n)
            ref = O.associate(cfg, tracks[s], 1, dets[s], want_matrices=False)
            np.testing.assert_array_equal(ids, ref["track_id"], err_msg=f"scene {s}")
            np.testing.assert_array_equal(votes, ref["voting_type"], err_msg=f"scene {s}")
    finally:
        eng.close()


@pytest.mark.parametrize("kind", ["cosine", "euclidean"])
@pytest.mark.parametrize("n,t,d", [(100, 130, 512), (257, 129, 72), (64, 64, 33), (1, 1, 5)])
def test_distance_matrix_vs_numpy_f64(kind, n, t, d):
    rng = np.random.default_rng(n + t + d)
    a = rng.standard_normal((n, d)).astype(np.float32)
    b = rng.standard_normal((t, d)).astype(np.float32)
    b[: min(n, t)] = a[: min(n, t)] + rng.uniform(-0.01, 0.01, (min(n, t), d)).astype(np.float32)
    cfg = abi.make_config()
    eng = Engine(cfg)
    try:
        out, ms = eng.distance_matrix(kind, a, b)
    finally:
        eng.close()
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    if kind == "cosine":
        ref = (a64 @ b64.T) / np.sqrt((a64 * a64).sum(1)[:, None] * (b64 * b64).sum(1)[None, :])
        assert np.abs(out - ref).max() <= 1e-5
    else:
        ref = np.sqrt(((a64[:, None, :] - b64[None, :, :]) ** 2).sum(-1))
        assert (np.abs(out - ref) <= 1e-5 * ref + 1e-7).all()
    # asymmetric operands + non-square shape: a transposed C write cannot pass
    assert out.shape == (n, t)


@pytest.mark.paths("never_lean", "bestfit_tile", "separate_resolve")
@pytest.mark.parametrize("plan", [0, 1, 2, 4, 5, 6, 7, 8, 9, 15, 16, 18])
@pytest.mark.parametrize("n,t,d", [(300, 333, 512), (129, 70, 96)])
def test_every_tile_plan_of_the_contraction(plan, n, t, d):
    """All six tile plans (128x128, 64x128, 128x64, 64x64 with 1/2/4 k-groups) produce the same cosine matrix, both in the
    standalone entry point and in the fused VisualSORT kernel (tap), including ragged edge tiles."""
    rng = np.random.default_rng(plan + n)
    a = rng.standard_normal((n, d)).astype(np.float32)
    b = rng.standard_normal((t, d)).astype(np.float32)
    eng = Engine(abi.make_config(gemm_plan=plan))
    try:
        out, _ = eng.distance_matrix("cosine", a, b)
    finally:
        eng.close()
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    ref = (a64 @ b64.T) / np.sqrt((a64 * a64).sum(1)[:, None] * (b64 * b64).sum(1)[None, :])
    assert np.abs(out - ref).max() <= 1e-5
    sc = synth.visual_scene(np.random.default_rng(3 + plan), t, n, d, 2, canvas=(1500.0, 900.0), new_fraction=0.1)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=d,
                          max_observations=2, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                          max_idle_epochs=5, gemm_plan=plan)
    check_visual(cfg, sc)


@pytest.mark.parametrize("plan", [0, 5, 15, 16, 18])
@pytest.mark.parametrize("k", [1, 3])
def test_wide_euclidean_tiles_of_the_contraction(plan, k):
    """The euclidean metric on the WIDER tiles of the stand-alone contraction (the contraction as a launch of its own, the tile plan
    pinned: 128 x 128 and 64 x 128 on the staged, direct and k-split loops): a lane holds two columns there and 128-row tiles take two
    64-row passes, the flagged cells of each pass (every true match: near-identical vectors) registered behind its cell loop and
    recomputed directly.  One observation per track: the tile votes itself (vote words; the tapped matrix from the same tile without
    them); three: the weight matrix.  Ragged edges in both directions."""
    n, t, d = 300, 333, 128
    sc = synth.visual_scene(np.random.default_rng(40 + plan + k), t, n, d, k, canvas=(1500.0, 900.0), new_fraction=0.1)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="euclidean", visual_threshold=0.6, feature_len=d,
                          max_observations=k, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                          max_idle_epochs=5, gemm_plan=plan, flags=abi.SA_FLAG_SEPARATE_FRAME)
    ids, votes, ref = check_visual(cfg, sc, tol_abs=1e-6, tol_rel=1e-5)
    assert (votes == abi.SA_VOTE_VISUAL).sum() > 100


@pytest.mark.paths("never_lean", "bestfit_tile", "separate_resolve")
def test_full_size_properties_c2():
    """BASELINE config C2 (1000 x 1000 x 512 cosine): size-independent properties instead of the slow oracle."""
    rng = np.random.default_rng(2)
    n = t = 1000
    d = 512
    sc = synth.visual_scene(rng, t, n, d, 1)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=d,
                          max_observations=1, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                          max_idle_epochs=5)
    tracks = abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"], feat_present=sc["track_present"])
    eng = Engine(cfg)
    try:
        eng.upsert(0, tracks)
        det = abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"])
        ids, votes = eng.associate(0, 1, det)
        # every identity is re-found, each track used once
        np.testing.assert_array_equal(ids, sc["truth"])
        assert (votes == abi.SA_VOTE_VISUAL).all()
        # idempotence
        ids2, votes2 = eng.associate(0, 1, det)
        np.testing.assert_array_equal(ids, ids2)
        # permutation equivariance over candidates
        p = rng.permutation(n)
        det_p = abi.make_detections(sc["det_boxes"][p], feats=sc["det_feats"][p], feat_quality=sc["det_quality"][p])
        ids3, _ = eng.associate(0, 1, det_p)
        np.testing.assert_array_equal(ids3, ids[p])
        # the visual matrix agrees with an f64 numpy contraction
        vis = eng.tap_visual()[:, :, 0]
        a64, b64 = sc["det_feats"][p].astype(np.float64), sc["track_feats"][:, 0].astype(np.float64)
        ref = 1.0 - (a64 @ b64.T) / np.sqrt((a64 * a64).sum(1)[:, None] * (b64 * b64).sum(1)[None, :])
        m = ~np.isnan(vis)
        assert m.mean() > 0.5
        assert np.abs(vis[m] - ref[m]).max() <= 1e-5
    finally:
        eng.close()


@pytest.mark.paths("never_lean")
def test_full_size_sort_oriented_c4_properties():
    """C4-sized oriented SORT (2000 x 2000): every shuffled, jittered detection returns to its track."""
    rng = np.random.default_rng(4)
    sc = synth.sort_scene(rng, 2000, 2000, canvas=(8192.0, 8192.0), oriented=True, pos_sigma=1.0)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, max_idle_epochs=5)
    eng = Engine(cfg)
    try:
        eng.upsert(0, abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"]))
        ids, votes = eng.associate(0, 1, abi.make_detections(sc["det_boxes"]))
        assert (ids == sc["truth"]).mean() > 0.97
        used = ids[ids != 0]
        assert len(used) == len(set(used.tolist()))
        q = eng.tap_quantised()
        assert (q >= 0).all() and (q <= 1_000_000).all()
        assert ((q == 0) | (q >= 300_000)).all()
    finally:
        eng.close()


def test_full_size_batch_c3_against_the_oracle():
    """BASELINE config C3's per-GPU share (8 scenes x 500 x 500, axis-aligned IoU) as ONE batch: every scene's answers are the
    oracle's (500 x 500 is still affordable on the host), and the same as that scene's alone."""
    rng = np.random.default_rng(33)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, max_idle_epochs=5)
    scs = [synth.sort_scene(rng, 500, 500, canvas=(4096.0, 4096.0)) for _ in range(8)]
    eng = Engine(cfg)
    try:
        dets, tracks = [], []
        for s, sc in enumerate(scs):
            tr = abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"])
            eng.upsert(s, tr)
            tracks.append(tr)
            dets.append(abi.make_detections(sc["det_boxes"]))
        eng.batch_begin()
        slots = [eng.batch_add(s, 1, d) for s, d in enumerate(dets)]
        eng.batch_run()
        eng.batch_sync()
        got = [eng.batch_fetch(sl, 500) for sl in slots]
        for s, sc in enumerate(scs):
            ref = O.associate(cfg, tracks[s], 1, dets[s], want_matrices=False)
            np.testing.assert_array_equal(got[s][0], ref["track_id"], err_msg=f"scene {s}")
            np.testing.assert_array_equal(got[s][1], ref["voting_type"])
            assert (got[s][0] == sc["truth"]).mean() > 0.9
        alone, _ = eng.associate(3, 1, dets[3])
        np.testing.assert_array_equal(alone, got[3][0])
    finally:
        eng.close()


def test_full_size_maha_c3_against_the_oracle():
    """BASELINE config C3's Mahalanobis half at its full per-scene size (500 x 500, Kalman states from three oracle cycles): every
    cost cell and the quantised matrix bit-identical to the oracle, equal assignment total (cost-0 ties leave the ids free)."""
    rng = np.random.default_rng(35)
    sc = synth.sort_scene(rng, 500, 500, canvas=(4096.0, 4096.0))
    kf = kf_states(rng, sc["track_boxes"])
    sc["det_boxes"] = synth.jitter_boxes(rng, kf[0], 2.0)[rng.permutation(500)]
    cfg = abi.make_config(positional="maha", positional_min_confidence=0.05, max_idle_epochs=5)
    ids, ref = check_sort(cfg, sc, kf=kf, require_ids=False)
    assert (ids != 0).sum() > 400


def test_full_size_properties_c5():
    """BASELINE config C5 (5000 tracks x 2000 detections x 4096-d cosine): size-independent properties — identities re-found,
    idempotence, permutation equivariance, and the weights of a sample of candidates against an f64 numpy contraction."""
    rng = np.random.default_rng(5)
    t, n, d = 5000, 2000, 4096
    sc = synth.visual_scene(rng, t, n, d, 1, canvas=(7680.0, 4320.0))
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=d,
                          max_observations=1, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                          max_idle_epochs=5)
    eng = Engine(cfg)
    try:
        eng.upsert(0, abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"], feat_present=sc["track_present"]))
        det = abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"])
        ids, votes = eng.associate(0, 1, det)
        np.testing.assert_array_equal(ids, sc["truth"])
        assert (votes == abi.SA_VOTE_VISUAL).all()
        ids2, _ = eng.associate(0, 1, det)
        np.testing.assert_array_equal(ids, ids2)
        p = rng.permutation(n)
        det_p = abi.make_detections(sc["det_boxes"][p], feats=sc["det_feats"][p], feat_quality=sc["det_quality"][p])
        ids3, _ = eng.associate(0, 1, det_p)
        np.testing.assert_array_equal(ids3, ids[p])
        vis = eng.tap_visual()[:, :, 0]
        rows = np.arange(0, n, 16)  # 125 candidates of the permuted frame against all 5000 tracks
        a64, b64 = sc["det_feats"][p][rows].astype(np.float64), sc["track_feats"][:, 0].astype(np.float64)
        ref = 1.0 - (a64 @ b64.T) / np.sqrt((a64 * a64).sum(1)[:, None] * (b64 * b64).sum(1)[None, :])
        m = ~np.isnan(vis[rows])
        assert m.mean() > 0.2
        assert np.abs(vis[rows][m] - ref[m]).max() <= 1e-5
    finally:
        eng.close()


@pytest.mark.paths("never_lean", "bestfit_tile", "separate_resolve")
def test_full_size_properties_c2_euclidean():
    """The C2 frame with the euclidean metric (vector-pipe kernel, vote words): identities re-found, idempotence, permutation
    equivariance, distances against f64 numpy within 1e-5 relative."""
    rng = np.random.default_rng(6)
    n = t = 1000
    d = 512
    sc = synth.visual_scene(rng, t, n, d, 1)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="euclidean", visual_threshold=0.5, feature_len=d,
                          max_observations=1, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                          max_idle_epochs=5)
    eng = Engine(cfg)
    try:
        eng.upsert(0, abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"], feat_present=sc["track_present"]))
        det = abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"])
        ids, votes = eng.associate(0, 1, det)
        np.testing.assert_array_equal(ids, sc["truth"])
        assert (votes == abi.SA_VOTE_VISUAL).all()
        p = rng.permutation(n)
        det_p = abi.make_detections(sc["det_boxes"][p], feats=sc["det_feats"][p], feat_quality=sc["det_quality"][p])
        ids3, _ = eng.associate(0, 1, det_p)
        np.testing.assert_array_equal(ids3, ids[p])
        vis = eng.tap_visual()[:, :, 0]
        a64, b64 = sc["det_feats"][p].astype(np.float64), sc["track_feats"][:, 0].astype(np.float64)
        ref = np.sqrt(np.maximum(((a64 * a64).sum(1)[:, None] + (b64 * b64).sum(1)[None, :] - 2.0 * (a64 @ b64.T)), 0.0))
        m = ~np.isnan(vis)
        assert m.sum() >= n  # at least the true pairs are within the threshold
        assert (np.abs(vis[m] - ref[m]) <= 1e-5 * ref[m] + 1e-6).all()
    finally:
        eng.close()


# ---- the positional vote on graphs that do NOT fall apart into tiny components ---------------------------------------------
@pytest.mark.paths("general")
def test_one_giant_component_against_the_oracle():
    """640 boxes piled on each other under IoU(0.05): ONE connected component, ~100 k usable edges (they stay in the HBM lists: the
    LDS pool holds 3072), most greedy bids colliding.  kuhn_munkres does not care about density (sort/voting.rs:86); the
    group-cooperative solver must reach its optimum — equal total always, identical ids on this seeded (tie-free) frame."""
    for sigma, floor in ((2.0, 636), (10.0, 600), (25.0, 560)):  # 13 / 218 / 255 rows lose their greedy bid
        sc = synth.sort_scene(np.random.default_rng(64), 640, 640, canvas=(150.0, 150.0), pos_sigma=sigma)
        cfg = abi.make_config(positional="iou", positional_threshold=0.05, max_idle_epochs=5)
        ids, ref = check_sort(cfg, sc)
        assert (ids != 0).sum() > floor
        assert (~np.isnan(ref["positional"])).sum() > 50_000


@pytest.mark.paths("general")
@pytest.mark.parametrize("sigma", [2.0, 12.0])
@pytest.mark.parametrize("n,t,canvas", [(1000, 1000, (1920.0, 1080.0)), (1024, 1024, (700.0, 500.0)), (300, 900, (500.0, 400.0)),
                                        (900, 1800, (1920.0, 1080.0)), (1000, 2048, (900.0, 600.0)), (640, 1100, (400.0, 300.0)),
                                        (1000, 2500, (1920.0, 1080.0)), (700, 4096, (1200.0, 800.0))])
def test_crowds_against_the_oracle(n, t, canvas, sigma):
    """Plain SORT on crowded frames (the C2 canvas without features, and denser): components of tens to hundreds of rows, pool and
    HBM-list edge storage; with 12 px of jitter dozens to hundreds of rows lose their greedy bid and need real augmenting paths.
    The shapes beyond 1024 tracks run the one-workgroup tail with two columns per thread (no LDS pool: every search walks the HBM
    lists; the dense solver on 512 threads)."""
    sc = synth.sort_scene(np.random.default_rng(n + t), t, n, canvas=canvas, pos_sigma=sigma)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3 if canvas[0] > 1000 else 0.15, max_idle_epochs=5)
    ids, ref = check_sort(cfg, sc)
    assert (ids != 0).sum() > 0.4 * min(n, t)


@pytest.mark.parametrize("oriented", [False, True])
@pytest.mark.parametrize("n,t,canvas,sigma", [(1000, 2500, (1920.0, 1080.0), 2.0), (1500, 1300, (1920.0, 1080.0), 8.0), (1100, 1100, (1300.0, 900.0), 5.0)])
def test_general_tail_mid_sized_components_against_the_oracle(n, t, canvas, sigma, oriented):
    """A tracker loop's crowd frames beyond the one-workgroup tail: hundreds of components, dozens of them with 9..32 rows — the
    general tail's middle tier (one wavefront per component on a [rows][64] matrix in LDS, columns renumbered through a hash
    table), next to one-row components, pooled small ones and, on the denser frames, components that overflow 32 rows or 64
    columns and go to the scene's queue."""
    sc = synth.sort_scene(np.random.default_rng(n + 7 * t + int(oriented)), t, n, canvas=canvas, oriented=oriented, pos_sigma=sigma)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3 if canvas[0] > 1500 else 0.15, max_idle_epochs=5)
    ids, ref = check_sort(cfg, sc)
    assert (ids != 0).sum() > 0.4 * min(n, t)


def test_middle_tier_refusals_go_to_the_queue():
    """Components the middle tier has to refuse: 40 large detections over a carpet of ~250 small tracks (IoU ~0.09 against a
    threshold of 0.05) — more than 32 rows AND more than 128 distinct columns: no [rows][columns] matrix of 8192 cells holds it.
    The wavefront that took such a component records the refusal and its workgroup finishes it with the workgroup-cooperative dense
    solver; 1100 isolated pairs around them keep the frame in the general tail.  (A refusal used to be pushed by lane 0 inside the
    wave's loop: the compiler kept the other 63 lanes apart from then on and they re-solved the first entry for ever.)"""
    rng = np.random.default_rng(77)
    singles = 1100
    tb = synth.dense_boxes(rng, singles, (1.0, 1.0))
    tb["xc"] = 40000.0 + 300.0 * (np.arange(singles) % 40)
    tb["yc"] = 40000.0 + 300.0 * (np.arange(singles) // 40)
    db = synth.jitter_boxes(rng, tb, 1.0)
    tracks, dets = [tb], [db]
    for c in range(6):
        ox, oy = 3000.0 * c, 800.0 * c
        gx, gy = np.meshgrid(np.arange(19), np.arange(13))
        small = synth.dense_boxes(rng, gx.size, (1.0, 1.0))
        small["xc"] = ox + 15.0 + 30.0 * gx.ravel() + rng.uniform(-0.5, 0.5, gx.size)
        small["yc"] = oy + 15.0 + 30.0 * gy.ravel() + rng.uniform(-0.5, 0.5, gx.size)
        small["height"] = rng.uniform(24.0, 29.0, gx.size)
        small["aspect"] = rng.uniform(0.9, 1.1, gx.size)
        dx, dy = np.meshgrid(np.arange(8), np.arange(5))
        large = synth.dense_boxes(rng, dx.size, (1.0, 1.0))
        large["xc"] = ox + 45.0 + 60.0 * dx.ravel() + rng.uniform(-1.0, 1.0, dx.size)
        large["yc"] = oy + 45.0 + 60.0 * dy.ravel() + rng.uniform(-1.0, 1.0, dx.size)
        large["height"] = 90.0
        large["aspect"] = 1.0
        tracks.append(small)
        dets.append(large)
    tb, db = np.concatenate(tracks), np.concatenate(dets)
    db["confidence"] = 1.0
    perm = rng.permutation(len(db))
    sc = dict(track_ids=np.arange(1, len(tb) + 1, dtype=np.uint64), track_boxes=tb, track_epochs=np.zeros(len(tb), np.uint64), det_boxes=db[perm])
    cfg = abi.make_config(positional="iou", positional_threshold=0.05, max_idle_epochs=5)
    ids, ref = check_sort(cfg, sc, require_ids=False)  # (a carpet of near-equal overlaps: equal totals, ids not unique)
    present = ~np.isnan(ref["positional"])
    big_rows = present.sum(1) >= 6
    assert big_rows.sum() == 240 and (ids[big_rows] != 0).all()


@pytest.mark.parametrize("n,t", [(700, 700), (1300, 1200), (700, 1500), (600, 2600)])
def test_mahalanobis_crowd_takes_the_64_bit_dense_solver(n, t):
    """Mahalanobis gains are 1e8-scale (cost <= 100 / confidence, x 1e6): beyond the 32-bit variant of the dense solver.  A crowd with
    genuine Kalman states on a small canvas — every detection inside the chi-square gate of dozens of tracks: components of hundreds
    of rows — goes through the 64-bit keys and arithmetic (two-pass wave minima) of sa_assign_component_dense, in the one-workgroup
    tail (700 x 700) and in the general one (1300 x 1200).  Cells and edges bit for bit, equal total gain (cells beyond the gate tie
    at cost 0, so ids are not unique)."""
    rng = np.random.default_rng(n + 3 * t)
    sc = synth.sort_scene(rng, t, n, canvas=(700.0, 500.0))
    kf = kf_states(rng, sc["track_boxes"])
    m = min(n, t)
    dets = synth.jitter_boxes(rng, kf[0][:m], 6.0)[rng.permutation(m)]
    if n > m:
        dets = np.concatenate([dets, synth.dense_boxes(rng, n - m, (700.0, 500.0))])
    sc["det_boxes"] = dets
    cfg = abi.make_config(positional="maha", positional_min_confidence=0.05, max_idle_epochs=5)
    ids, ref = check_sort(cfg, sc, kf=kf, require_ids=False)
    assert (ids != 0).sum() > 0.5 * m
    present = ~np.isnan(ref["positional"])
    assert present.sum() > 20 * n, "the frame lost its density"


@pytest.mark.paths("general", "euclid_valu", "euclid_mfma")
@pytest.mark.parametrize("visual", ["cosine", "euclidean"])
def test_dense_positional_stage_behind_a_visual_vote(visual):
    _dense_positional_stage_behind_a_visual_vote(visual, "eager" if visual == "cosine" else None)


@pytest.mark.paths("general")
def test_dense_positional_stage_behind_a_visual_vote_lazy():
    _dense_positional_stage_behind_a_visual_vote("cosine", "lazy")


def _dense_positional_stage_behind_a_visual_vote(visual, pos_mode):
    """VisualSORT on a pile: 35 % of the detections are new or below the quality gate, so the positional stage inherits hundreds of
    rows whose edges (IoU threshold 0.05, everything overlaps) overflow the LDS pool and run to columns the visual vote has
    excluded — the HBM-list variant of the cooperative solver with the exclusion table."""
    rng = np.random.default_rng(66)
    n = t = 600
    d = 64
    sc = synth.visual_scene(rng, t, n, d, 1, canvas=(300.0, 250.0), new_fraction=0.25)
    sc["det_quality"][rng.uniform(size=n) < 0.15] = 0.05
    cfg = abi.make_config(positional="iou", positional_threshold=0.05, visual=visual, visual_threshold=0.2 if visual == "cosine" else 0.5,
                          feature_len=d, max_observations=1, visual_min_votes=1, visual_minimal_track_length=1, visual_minimal_quality_use=0.3,
                          positional_min_confidence=0.1, max_idle_epochs=5)
    ids, votes, ref = check_visual(cfg, sc, tol_abs=1e-5 if visual == "cosine" else 0.0, tol_rel=0.0 if visual == "cosine" else 1e-5,
                                   pos_mode=pos_mode)
    assert (votes == abi.SA_VOTE_POSITIONAL).sum() > 50 and (votes == abi.SA_VOTE_VISUAL).sum() > 200


@pytest.mark.parametrize("case", ["crowd", "pile", "rect"])
def test_big_frames_with_big_components_against_the_oracle(case):
    """More than 1024 detections or tracks AND components of tens to a thousand rows: the general tail's wave-cooperative solver
    (state in HBM).  A crowd of 1500 x 1500 with 12 px of jitter, ONE pile of 1200 boxes under IoU(0.05) with most bids colliding,
    and 700 detections against 1800 tracks."""
    n, t, canvas, thr, sigma = {"crowd": (1500, 1500, (1000.0, 800.0), 0.15, 12.0), "pile": (1200, 1200, (200.0, 200.0), 0.05, 10.0),
                                "rect": (700, 1800, (600.0, 500.0), 0.1, 8.0)}[case]
    sc = synth.sort_scene(np.random.default_rng(n + t), t, n, canvas=canvas, pos_sigma=sigma)
    cfg = abi.make_config(positional="iou", positional_threshold=thr, max_idle_epochs=5)
    ids, ref = check_sort(cfg, sc)
    assert (ids != 0).sum() > 0.4 * min(n, t)


def test_big_visual_frame_with_a_dense_positional_stage():
    """1300 x 1300 VisualSORT on a small canvas, a third of the detections new or featureless: partials + resolve (no vote words
    beyond 1024), exclusions, and a positional stage whose components are hundreds of rows — the general tail end to end."""
    rng = np.random.default_rng(67)
    n = t = 1300
    d = 64
    sc = synth.visual_scene(rng, t, n, d, 1, canvas=(400.0, 300.0), new_fraction=0.2)
    sc["det_quality"][rng.uniform(size=n) < 0.15] = 0.05
    cfg = abi.make_config(positional="iou", positional_threshold=0.05, visual="cosine", visual_threshold=0.2, feature_len=d, max_observations=1,
                          visual_min_votes=1, visual_minimal_track_length=1, visual_minimal_quality_use=0.3, positional_min_confidence=0.1,
                          max_idle_epochs=5)
    ids, votes, ref = check_visual(cfg, sc)
    assert (votes == abi.SA_VOTE_POSITIONAL).sum() > 100 and (votes == abi.SA_VOTE_VISUAL).sum() > 500


@pytest.mark.paths("general", "separate_resolve")   # (default: k_assign_small2 with vote words at K = 1; separate_resolve: its verdict-array form; general: the other tail)
@pytest.mark.parametrize("visual,k", [("cosine", 1), ("euclidean", 2)])
def test_visual_frame_whose_positional_stage_is_pairs_and_knots(visual, k):
    """1200 detections x 1500 tracks VisualSORT on the C2 canvas, 40 % of the detections new or below the quality gate: the
    positional stage inherits several hundred rows in components of one, two (the register path of the general tail) and a dozen rows
    (its one-wavefront middle tier), whose records also name columns the visual vote has taken (excluded_tracks: skipped when the
    bids are formed, when the hash table is filled and when the pair's runner-ups are chosen)."""
    rng = np.random.default_rng(91 + k)
    n, t, d = 1200, 1500, 48
    sc = synth.visual_scene(rng, t, n, d, k, canvas=(1920.0, 1080.0), new_fraction=0.25)
    sc["det_quality"][rng.uniform(size=n) < 0.2] = 0.05
    cfg = abi.make_config(positional="iou", positional_threshold=0.15, visual=visual, visual_threshold=0.2 if visual == "cosine" else 0.5,
                          feature_len=d, max_observations=k, visual_min_votes=1, visual_minimal_track_length=1, visual_minimal_quality_use=0.3,
                          positional_min_confidence=0.1, max_idle_epochs=5)
    ids, votes, ref = check_visual(cfg, sc, tol_abs=1e-5 if visual == "cosine" else 0.0, tol_rel=0.0 if visual == "cosine" else 1e-5)
    assert (votes == abi.SA_VOTE_POSITIONAL).sum() > 100 and (votes == abi.SA_VOTE_VISUAL).sum() > 400


# ---- the headline configurations at FULL size against the oracle -------------------------------------------------------
# The oracle's distance stage runs on host threads partitioned like the reference's TrackStore (or_associate_sharded: track id %
# shards, one vote after the shards) — cell for cell the single-thread oracle, in a fraction of its time.
def _full_size_visual(cfg, sc, shards=32, pos_mode=None):
    tracks = abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"], feat_present=sc["track_present"])
    det = abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"])
    ref = O.associate(cfg, tracks, 1, det, shards=shards)
    ref["_track_ids"] = sc["track_ids"]
    cfg.flags |= abi.SA_FLAG_TAP | POS_MODE_FLAGS.get(pos_mode, 0)
    eng = Engine(cfg)
    try:
        eng.upsert(0, tracks)
        ids, votes = eng.associate(0, 1, det)
        # the frame's own launches (the fused raw-row first phase + the tail at C2): edge records bit for bit, vote weights within
        # the distance tolerance — before the matrix taps re-launch anything
        n_edges = check_edges(eng, ref["quantised"], thr_q_of(cfg), mode=mode_of(cfg, det.n, tracks.n), prove=pos_mode is not None,
                              pos_ref=ref["positional"])
        euclid = cfg.visual_kind == abi.SA_VIS_EUCLIDEAN
        check_votes(cfg, eng, ref["visual"], tol_abs=0.0 if euclid else 1e-5, tol_rel=1e-5 if euclid else 0.0)
        assert n_edges > 0 or pos_mode == "lazy"   # (lazy: a frame whose every row finds a visual group has no edge at all)
        pos, vis, q = eng.tap_positional(), eng.tap_visual(), eng.tap_quantised()
    finally:
        eng.close()
    np.testing.assert_array_equal(q, ref["quantised"])  # IoU: the i64 matrix of SortVoting bit for bit
    return ids, votes, pos, vis, ref


@pytest.mark.paths("row_tiles", "staged_loop", "no_yield")
def test_full_size_c2_against_the_oracle():
    _full_size_c2("eager")


@pytest.mark.paths("row_tiles", "staged_loop", "no_yield")
def test_full_size_c2_against_the_oracle_lazy():
    """C2 forced lazy: every row finds a visual group, so the lazy phase emits no edge where eager emits ~1500."""
    _full_size_c2("lazy")


def _full_size_c2(pos_mode):
    """BASELINE C2 (1000 x 1000 x 512-d cosine + IoU): IoU cells and the quantised matrix bit for bit, every cosine weight within
    1e-5, ids and vote types identical."""
    sc = synth.visual_scene(np.random.default_rng(2), 1000, 1000, 512, 1)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=512,
                          max_observations=1, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                          max_idle_epochs=5)
    ids, votes, pos, vis, ref = _full_size_visual(cfg, sc, pos_mode=pos_mode)
    compare_visual(cfg, ids, votes, pos, vis, ref)
    assert (~np.isnan(pos)).sum() > 1000 and (~np.isnan(vis)).mean() > 0.5


def test_full_size_c2_with_new_and_featureless_detections_against_the_oracle():
    _full_size_c2_with_new_and_featureless("eager")


def test_full_size_c2_with_new_and_featureless_detections_against_the_oracle_lazy():
    _full_size_c2_with_new_and_featureless("lazy")


def _full_size_c2_with_new_and_featureless(pos_mode):
    """The C2 frame with 15 % new objects and 10 % of the detections without a usable feature: the positional (Hungarian) stage has
    real work after the visual vote.  Same gates."""
    rng = np.random.default_rng(12)
    sc = synth.visual_scene(rng, 1000, 1000, 512, 1, new_fraction=0.15)
    sc["det_quality"][rng.uniform(size=1000) < 0.10] = 0.05
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=512,
                          max_observations=1, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                          visual_minimal_quality_use=0.3, max_idle_epochs=5)
    ids, votes, pos, vis, ref = _full_size_visual(cfg, sc, pos_mode=pos_mode)
    compare_visual(cfg, ids, votes, pos, vis, ref)
    assert (votes == abi.SA_VOTE_POSITIONAL).sum() > 20 and (votes == abi.SA_VOTE_VISUAL).sum() > 600


def test_full_size_c2_three_observations_against_the_oracle():
    """C2 with the bank three observations deep (weight matrix + BestFit tile + resolve path)."""
    sc = synth.visual_scene(np.random.default_rng(13), 1000, 1000, 512, 3)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=512,
                          max_observations=3, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                          max_idle_epochs=5)
    ids, votes, pos, vis, ref = _full_size_visual(cfg, sc)
    compare_visual(cfg, ids, votes, pos, vis, ref)


@pytest.mark.paths("separate_resolve", "never_lean")
@pytest.mark.parametrize("k", [1, 3])
def test_full_size_more_tracks_than_the_small_tail_holds_against_the_oracle(k):
    """1000 detections x 1500 tracks x 512-d (a tracker loop's table once idle tracks linger: T > 1024 is its NORMAL state): the fused
    first phase with vote words (class words at K = 3) feeding the many-workgroup tail — k_assign_label<WORDS> turns the words into
    verdicts, the solver re-arms them — three launches.  Same gates as C2: IoU cells and the quantised matrix bit for bit, every
    cosine weight within 1e-5, the timed launches' own edges and votes, ids and vote types identical."""
    rng = np.random.default_rng(1500 + k)
    sc = synth.visual_scene(rng, 1500, 1000, 512, k, new_fraction=0.1)
    sc["det_quality"][rng.uniform(size=1000) < 0.05] = 0.05
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=512,
                          max_observations=k, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                          visual_minimal_quality_use=0.3, max_idle_epochs=5)
    ids, votes, pos, vis, ref = _full_size_visual(cfg, sc)
    compare_visual(cfg, ids, votes, pos, vis, ref)
    assert (votes == abi.SA_VOTE_POSITIONAL).sum() > 10 and (votes == abi.SA_VOTE_VISUAL).sum() > 700


def test_c4_shaped_sort_frame_takes_two_launches():
    """2000 x 2000 oriented SORT (BASELINE C4's shape): positional tiles + the one-workgroup tail with two rows and two columns per thread
    (k_assign_small2) — two launches, not three; ids against the oracle."""
    rng = np.random.default_rng(2000)
    sc = synth.sort_scene(rng, 2000, 2000, canvas=(7000.0, 5000.0), oriented=True)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, max_idle_epochs=5, flags=abi.SA_FLAG_PROFILE)
    if abi.EXTRA_FLAGS:
        pytest.skip("default path only")
    tracks = abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"])
    det = abi.make_detections(sc["det_boxes"])
    eng = Engine(cfg)
    try:
        eng.upsert(0, tracks)
        eng.associate(0, 1, det)
        eng.profile_reset()
        ids, votes = eng.associate(0, 1, det)
        prof = eng.profile_read()
    finally:
        eng.close()
    launched = {k for k, (n, _) in prof.items() if n and k != "d2h_results"}
    assert launched == {"k_frame", "k_assign_small"}, prof
    ref = O.associate(cfg, tracks, 1, det, want_matrices=False)
    np.testing.assert_array_equal(ids, ref["track_id"])
    np.testing.assert_array_equal(votes, ref["voting_type"])
    assert (ids != 0).sum() > 1500


@pytest.mark.parametrize("t,k,expect", [(1500, 1, {"k_frame_visual", "k_assign_small"}), (2048, 1, {"k_frame_visual", "k_assign_small"}),
                                        (1500, 3, {"k_frame_visual", "k_assign_small"}),
                                        (2100, 1, {"k_frame_visual", "k_assign_small"}), (3000, 1, {"k_frame_visual", "k_assign_small"}),
                                        (4096, 1, {"k_frame", "k_visual_cost", "k_assign_small"}),   # (1024 tiles of 64 x 64: the contraction takes 128 x 128 tiles, a launch of its own)
                                        (2100, 3, {"k_frame_visual", "k_assign_small"}),   # (class words read twice: k_assign_small2<.., 1, 4>)
                                        (4200, 1, {"k_frame_visual", "k_assign_label", "k_assign_solve"})])
def test_launches_of_frames_beyond_1024_tracks(t, k, expect):
    """1000 detections against 1025 .. 2048 tracks (a tracker loop's table once idle tracks linger): first phase + the ONE-workgroup tail,
    two columns per thread — two launches, with vote words (one observation per track) and with class words (three); up to 4096 tracks
    four columns per thread (k_assign_small2<.., 1, 4>); beyond: first phase, label, solve.
    No stand-alone contraction, no resolve kernel."""
    rng = np.random.default_rng(1503 + t + k)
    sc = synth.visual_scene(rng, t, 1000, 128, k)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=128,
                          max_observations=k, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                          max_idle_epochs=5, flags=abi.SA_FLAG_PROFILE)
    if abi.EXTRA_FLAGS:
        pytest.skip("default path only")
    tracks = abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"], feat_present=sc["track_present"])
    det = abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"])
    eng = Engine(cfg)
    try:
        eng.upsert(0, tracks)
        eng.associate(0, 1, det)
        eng.profile_reset()
        ids, votes = eng.associate(0, 1, det)
        prof = eng.profile_read()
    finally:
        eng.close()
    launched = {k for k, (n, _) in prof.items() if n and k != "d2h_results"}
    assert launched == expect, prof
    np.testing.assert_array_equal(ids, sc["truth"])


@pytest.mark.paths("never_lean")
@pytest.mark.parametrize("k", [1, 3])
def test_full_size_batched_c2_against_the_oracle(k):
    _full_size_batched_c2(k, "eager" if k == 1 else None)


@pytest.mark.paths("never_lean")
def test_full_size_batched_c2_against_the_oracle_lazy():
    _full_size_batched_c2(1, "lazy")


def _full_size_batched_c2(k, pos_mode):
    """BatchVisualSORT at configuration scale (visual_sort/batch_api.rs:213-317): 8 scenes x (1000 x 1000 x 512-d cosine + IoU) in ONE
    request set — grid.z = scene through the first phase and the tail — with SA_FLAG_TAP: every scene's edge records bit for bit, its
    vote words (class words at K = 3) within the distance tolerance, its ids and vote types against the oracle's (distance stage
    sharded over the host's cores)."""
    S = 8
    rng = np.random.default_rng(800 + k)
    scs = [synth.visual_scene(rng, 1000, 1000, 512, k, new_fraction=0.05 * (s % 3)) for s in range(S)]
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=512,
                          max_observations=k, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                          max_idle_epochs=5, flags=abi.SA_FLAG_TAP | POS_MODE_FLAGS.get(pos_mode, 0))
    trs = [abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"], feat_present=sc["track_present"]) for sc in scs]
    dets = [abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"]) for sc in scs]
    eng = Engine(cfg)
    try:
        for s in range(S):
            eng.upsert(100 + s, trs[s])
        eng.batch_begin()
        slots = [eng.batch_add(100 + s, 1, dets[s]) for s in range(S)]
        eng.batch_run()
        eng.batch_sync()
        first = {}
        for s in range(S):
            ref = O.associate(cfg, trs[s], 1, dets[s], shards=32)
            ids, votes = eng.batch_fetch(slots[s], 1000)
            first[s] = ids
            n_edges = check_edges(eng, ref["quantised"], thr_q_of(cfg), slot=slots[s], mode=mode_of(cfg, 1000, 1000),
                                  prove=pos_mode is not None, pos_ref=ref["positional"])
            assert n_edges > 0 or pos_mode == "lazy"
            check_votes(cfg, eng, ref["visual"], tol_abs=1e-5, slot=slots[s])
            np.testing.assert_array_equal(ids, ref["track_id"], err_msg=f"scene {s}")
            np.testing.assert_array_equal(votes, ref["voting_type"], err_msg=f"scene {s}")
            assert (ids == scs[s]["truth"]).mean() > 0.99
        # the same request set again (the replay the bench times): state left clean by the first run
        eng.batch_run()
        eng.batch_sync()
        for s in (0, S - 1):
            ids2, _ = eng.batch_fetch(slots[s], 1000)
            np.testing.assert_array_equal(ids2, first[s])
    finally:
        eng.close()


@pytest.mark.paths("euclid_valu", "euclid_mfma", "staged_loop")
def test_full_size_c2_euclidean_against_the_oracle():
    """The C2 frame under the reference's DEFAULT visual metric: every euclidean distance within 1e-5 relative."""
    sc = synth.visual_scene(np.random.default_rng(6), 1000, 1000, 512, 1)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="euclidean", visual_threshold=0.5, feature_len=512,
                          max_observations=1, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                          max_idle_epochs=5)
    ids, votes, pos, vis, ref = _full_size_visual(cfg, sc)
    compare_visual(cfg, ids, votes, pos, vis, ref, tol_abs=0.0, tol_rel=1e-5)
    assert (~np.isnan(vis)).sum() >= 1000


def hard_margin_scene(rng, metric, pairs=500, d=512, gap=(3e-5, 1e-4)):
    """A C2-sized frame built so that the BestFit vote is SENSITIVE to the 1e-5 distance tolerance: every one of `pairs` tracks is seen
    by TWO detections whose distances to it differ by only `gap` (uniform; absolute for the cosine, relative for the euclidean
    distance) — a kernel whose distances were off by a few 1e-5 would hand columns to the wrong candidate, where the plain synthetic
    frame (winner at cos ~1.0, runner-up at ~0.6) would not notice an error of 1e-3.  The other tracks see nothing."""
    t = n = 2 * pairs
    ident = synth.reid_identities(rng, t, d).astype(np.float64)
    bank = ident + rng.uniform(-0.01, 0.01, ident.shape)
    det = np.empty((n, d), np.float64)
    for i in range(pairs):
        f = bank[i]
        a = ident[i] + rng.uniform(-0.01, 0.01, d)
        g = rng.uniform(*gap)
        if metric == "euclidean":
            b = f + (a - f) * (1.0 + g)   # |b - f| = (1 + g) |a - f| exactly
        else:
            # a + s r with r orthogonal to f lowers the cosine monotonically in s: bisection for a drop of g
            ca = a @ f / np.sqrt((a @ a) * (f @ f))
            r = rng.standard_normal(d)
            r -= (r @ f) / (f @ f) * f
            r *= np.linalg.norm(a) / np.linalg.norm(r)
            lo, hi = 0.0, 1.0
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                b = a + mid * r
                cb = b @ f / np.sqrt((b @ b) * (f @ f))
                lo, hi = (mid, hi) if cb > ca - g else (lo, mid)
            b = a + 0.5 * (lo + hi) * r
        det[2 * i], det[2 * i + 1] = a, b
    perm = rng.permutation(n)
    tboxes = synth.dense_boxes(rng, t, (6000.0, 4000.0))
    dboxes = synth.dense_boxes(rng, n, (6000.0, 4000.0))   # positions unrelated to the tracks: the visual vote alone decides
    return dict(track_ids=np.arange(1, t + 1, dtype=np.uint64), track_boxes=tboxes, track_epochs=np.zeros(t, np.uint64),
                track_feats=bank.astype(np.float32)[:, None, :].copy(), track_present=np.ones((t, 1), np.uint8),
                det_boxes=dboxes, det_feats=det.astype(np.float32)[perm].copy(), det_quality=np.full(n, 0.9, np.float32))


@pytest.mark.parametrize("visual", ["cosine", "euclidean"])
def test_full_size_c2_hard_margins_against_the_oracle(visual):
    _full_size_c2_hard_margins(visual, "eager" if visual == "cosine" else None)


def test_full_size_c2_hard_margins_against_the_oracle_lazy():
    _full_size_c2_hard_margins("cosine", "lazy")


def _full_size_c2_hard_margins(visual, pos_mode):
    """C2 size with runner-ups within 1e-4 of the winners (hard_margin_scene): ids and vote types of the DEFAULT path (lean fused
    raw-row first phase, vote words) must equal the oracle's on every row whose decision the oracle makes with a margin above
    2.5 times the tolerance — i.e. on nearly all of them — and the vote words themselves pass check_votes."""
    sc = hard_margin_scene(np.random.default_rng(77), visual)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual=visual, visual_threshold=0.2 if visual == "cosine" else 0.5,
                          feature_len=512, max_observations=1, visual_min_votes=1, visual_minimal_track_length=1,
                          positional_min_confidence=0.1, max_idle_epochs=5)
    ids, votes, pos, vis, ref = _full_size_visual(cfg, sc, pos_mode=pos_mode)
    rv = ref["visual"][:, :, 0].astype(np.float64)
    w = np.where(np.isnan(rv), np.inf, rv)
    # margin of every column's decision in the ORACLE's matrix: lightest against second lightest weight of the column, in units of
    # the metric's tolerance (absolute for the cosine, relative for the euclidean distance)
    part = np.partition(w, 1, axis=0)
    scale = np.ones(w.shape[1]) if visual == "cosine" else np.where(np.isfinite(part[0]), np.abs(part[0]), 1.0)
    with np.errstate(invalid="ignore"):
        margin = (part[1] - part[0]) / scale
    has = np.isfinite(w.min(axis=1))
    best_col = np.argmin(w, axis=1)
    used = np.unique(best_col[has])                      # the columns somebody competes for: the 500 tracks with two detections each
    assert len(used) >= 450 and np.isfinite(margin[used]).all()
    assert np.median(margin[used]) < 1.5e-4 and margin[used].max() < 1e-3, "the scene lost its hard margins"
    safe_cols = ~np.isfinite(margin) | (margin > 2.5e-5)
    assert safe_cols[used].mean() > 0.97
    # a row is checked unless it competes for an unsafe column (its own best column)
    checked = ~has | safe_cols[best_col]
    np.testing.assert_array_equal(ids[checked], ref["track_id"][checked])
    np.testing.assert_array_equal(votes[checked], ref["voting_type"][checked])
    assert (votes[checked] == abi.SA_VOTE_VISUAL).sum() >= 450


def hard_margin_scene_bank(rng, metric, pairs=500, d=512, k=3, gap=(1e-4, 4e-4)):
    """hard_margin_scene for banks of k observations: every one of `pairs` tracks (k noisy views of its identity) is seen by TWO
    detections whose GROUP weights — the sums over the track's k observations that BestFitVoting compares (voting/best.rs:93-95) — differ
    by only `gap` (absolute for the cosine weights 1 - cos, relative for the euclidean distances): the class words of the default path
    (one 64-bit word per candidate / track and count class, the key of the f32 sum of a group's weights) must rank them as the
    reference's f64 sum of f32 differences does."""
    t = n = 2 * pairs
    ident = synth.reid_identities(rng, t, d).astype(np.float64)
    bank = ident[:, None, :] + rng.uniform(-0.01, 0.01, (t, k, d))

    def group(x, fs):
        if metric == "euclidean":
            return float(np.sqrt(((x[None, :] - fs) ** 2).sum(1)).sum())
        return float((1.0 - (fs @ x) / np.sqrt((x @ x) * (fs * fs).sum(1))).sum())

    det = np.empty((n, d), np.float64)
    for i in range(pairs):
        fs = bank[i]
        a = ident[i] + rng.uniform(-0.01, 0.01, d)
        g = rng.uniform(*gap)
        target = group(a, fs) * (1.0 + g) if metric == "euclidean" else group(a, fs) + g
        r = rng.standard_normal(d)
        fm = fs.mean(0)
        r -= (r @ fm) / (fm @ fm) * fm
        r *= np.linalg.norm(a) / np.linalg.norm(r)
        lo, hi = 0.0, 1.0
        for _ in range(70):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if group(a + mid * r, fs) < target else (lo, mid)
        det[2 * i], det[2 * i + 1] = a, a + 0.5 * (lo + hi) * r
    perm = rng.permutation(n)
    tboxes = synth.dense_boxes(rng, t, (6000.0, 4000.0))
    dboxes = synth.dense_boxes(rng, n, (6000.0, 4000.0))   # positions unrelated to the tracks: the visual vote alone decides
    return dict(track_ids=np.arange(1, t + 1, dtype=np.uint64), track_boxes=tboxes, track_epochs=np.zeros(t, np.uint64),
                track_feats=bank.astype(np.float32).copy(), track_present=np.ones((t, k), np.uint8),
                det_boxes=dboxes, det_feats=det.astype(np.float32)[perm].copy(), det_quality=np.full(n, 0.9, np.float32))


@pytest.mark.paths("bestfit_tile", "staged_loop")
@pytest.mark.parametrize("visual", ["cosine", "euclidean"])
def test_full_size_c2_bank_of_three_hard_margins_against_the_oracle(visual):
    """C2 size, three observations per track, runner-up GROUPS within 4e-4 of the winners (hard_margin_scene_bank): ids and vote types of
    the default path (whole-track tiles, class words) — and of the weight-matrix path (SA_FLAG_BESTFIT_TILE: the reference's formula on
    the engine's own distances) — equal the oracle's on every row whose decision the oracle makes with a margin above 2.5 times the
    tolerance of a three-term sum."""
    k = 3
    sc = hard_margin_scene_bank(np.random.default_rng(79), visual, k=k)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual=visual, visual_threshold=0.2 if visual == "cosine" else 0.5,
                          feature_len=512, max_observations=k, visual_min_votes=1, visual_minimal_track_length=1,
                          positional_min_confidence=0.1, max_idle_epochs=5)
    ids, votes, pos, vis, ref = _full_size_visual(cfg, sc)
    rv = ref["visual"].astype(np.float64)                       # [N][T][K] weights, NaN = absent
    full = ~np.isnan(rv).any(axis=2)
    w = np.where(full, np.nansum(rv, axis=2), np.inf)            # group sums where all three observations vote (the scene's pairs)
    part = np.partition(w, 1, axis=0)
    scale = np.ones(w.shape[1]) if visual == "cosine" else np.where(np.isfinite(part[0]), np.abs(part[0]), 1.0)
    with np.errstate(invalid="ignore"):
        margin = (part[1] - part[0]) / scale
    has = np.isfinite(w.min(axis=1))
    best_col = np.argmin(w, axis=1)
    used = np.unique(best_col[has])
    assert len(used) >= 450 and np.isfinite(margin[used]).all()
    assert np.median(margin[used]) < 6e-4 and margin[used].max() < 4e-3, "the scene lost its hard margins"
    tol = (1e-5 if visual == "cosine" else 1e-5 / k) * k          # a sum of k weights each within 1e-5 (euclidean: relative to the sum)
    safe_cols = ~np.isfinite(margin) | (margin > 2.5 * tol)
    assert safe_cols[used].mean() > 0.9
    checked = ~has | safe_cols[best_col]
    np.testing.assert_array_equal(ids[checked], ref["track_id"][checked])
    np.testing.assert_array_equal(votes[checked], ref["voting_type"][checked])
    assert (votes[checked] == abi.SA_VOTE_VISUAL).sum() >= 400


def test_full_size_c4_against_the_oracle():
    """BASELINE C4 (oriented SORT 2000 x 2000): all 4 M cells — present/absent mask, f32 IoU bit patterns, quantised i64 matrix —
    and the assignment against the oracle."""
    sc = synth.sort_scene(np.random.default_rng(4), 2000, 2000, canvas=(8192.0, 8192.0), oriented=True, pos_sigma=1.0)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, max_idle_epochs=5)
    ids, ref = check_sort(cfg, sc)
    assert (ids == sc["truth"]).mean() > 0.97


def test_full_size_c5_against_the_oracle():
    """BASELINE C5 (5000 tracks x 2000 detections x 4096-d cosine): all 10 M cosine weights within 1e-5, all IoU cells bit for
    bit, ids and vote types identical.  (The oracle's distance stage takes ~100 s on one host thread: sharded over 32.)"""
    sc = synth.visual_scene(np.random.default_rng(5), 5000, 2000, 4096, 1, canvas=(7680.0, 4320.0))
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.2, feature_len=4096,
                          max_observations=1, visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1,
                          max_idle_epochs=5)
    ids, votes, pos, vis, ref = _full_size_visual(cfg, sc, shards=48)
    compare_visual(cfg, ids, votes, pos, vis, ref)
    np.testing.assert_array_equal(ids, sc["truth"])


# ---- randomized sweep over the configuration space --------------------------------------------------------------------
def _fuzz_case(seed):
    """One random (config, scene): sizes around the tile edges (16, 64, 128, 256), every metric pair, ragged banks, missing
    features, qualities, own areas, idle epochs and spatio-temporal constraints."""
    rng = np.random.default_rng(90000 + seed)
    n = int(rng.choice([0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 129, 200, 257]))
    t = int(rng.choice([0, 1, 3, 16, 63, 64, 65, 128, 130, 255, 256, 260, 300]))
    oriented = bool(rng.integers(2))
    canvas = (float(rng.uniform(300, 2500)), float(rng.uniform(300, 1500)))
    visual = [None, "cosine", "euclidean"][int(rng.integers(3))]
    positional = ["iou", "maha"][int(rng.integers(2))]
    cons = ()
    if rng.uniform() < 0.5:
        cons = tuple(sorted((int(e), float(rng.uniform(0.3, 3.0))) for e in rng.choice(np.arange(1, 6), size=int(rng.integers(1, 3)), replace=False)))
    common = dict(positional=positional, positional_threshold=float(rng.choice([0.1, 0.3, 0.5])), max_idle_epochs=int(rng.integers(1, 6)),
                  positional_min_confidence=float(rng.choice([0.05, 0.1, 0.4])), constraints=cons, flags=int(rng.choice([0, abi.SA_FLAG_SEPARATE_FRAME])))
    if visual is None:
        sc = synth.sort_scene(rng, t, n, canvas=canvas, oriented=oriented)
        cfg = abi.make_config(**common)
    else:
        # (d = 1 is left out: every cosine is exactly +-1 there, the BestFit vote is one big tie and the 1e-5 freedom of the
        # feature distances decides the winners)
        d = int(rng.choice([5, 7, 8, 31, 32, 33, 64, 100, 128, 200]))
        k = int(rng.integers(1, 5))
        sc = synth.visual_scene(rng, max(t, 1), max(n, 1), d, k, canvas=canvas, oriented=oriented, new_fraction=float(rng.uniform(0, 0.3)))
        for key in ("track_ids", "track_boxes", "track_epochs", "track_feats", "track_present"):
            sc[key] = sc[key][:t]
        for key in ("det_boxes", "det_feats", "det_quality", "truth"):
            sc[key] = sc[key][:n]
        pres = sc["track_present"]
        pres[rng.uniform(size=pres.shape) < 0.2] = 0
        cfg = abi.make_config(visual=visual, visual_threshold=float(rng.choice([0.2, 0.5])) if visual == "cosine" else float(rng.choice([0.3, 0.8, 3.0e38])),
                              feature_len=d, max_observations=k, visual_min_votes=int(rng.integers(1, k + 1)),
                              visual_minimal_track_length=int(rng.integers(1, k + 1)), visual_minimal_area=float(rng.choice([0.0, 3000.0])),
                              visual_minimal_quality_use=float(rng.choice([0.0, 0.5])),
                              visual_minimal_own_area_percentage_use=float(rng.choice([0.0, 0.4])), **common)
    # epochs spread around the current one so that max_idle_epochs and the constraints' epoch deltas bite
    epoch = 7
    if t:
        sc["track_epochs"] = rng.integers(1, 8, size=t).astype(np.uint64)
    return rng, cfg, sc, epoch, positional, visual


@pytest.mark.paths("general", "euclid_valu", "euclid_mfma")
@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("SA_FUZZ_N", "40"))))
def test_random_configurations(seed):
    rng, cfg, sc, epoch, positional, visual = _fuzz_case(seed)
    n, t = len(sc["det_boxes"]), len(sc["track_boxes"])
    kf = kf_states(rng, sc["track_boxes"]) if (positional == "maha" and t) else None
    if positional == "maha" and not t:
        kf = (sc["track_boxes"], np.zeros((0, 5), np.float32), np.zeros((0, 25), np.float32))
    if visual is None:
        # Mahalanobis cells are often exactly tied at cost 0 (d2 above the chi-square bound): ids only on IoU
        check_sort(cfg, sc, epoch=epoch, kf=kf, require_ids=positional == "iou")
    else:
        own = rng.uniform(0, 1, n).astype(np.float32) if rng.uniform() < 0.5 else None
        if own is not None:
            own[rng.uniform(size=n) < 0.2] = np.nan
        dp = (rng.uniform(size=n) > 0.15).astype(np.uint8) if rng.uniform() < 0.5 else None
        tol_rel = 1e-5 if visual == "euclidean" else 0.0
        if positional == "maha":
            ids, votes, pos, vis, ref = visual_run(cfg, sc, epoch=epoch, kf=kf, own_area=own, det_present=dp)
            np.testing.assert_array_equal(np.isnan(pos), np.isnan(ref["positional"]))
            np.testing.assert_array_equal(pos.view(np.uint32)[~np.isnan(pos)], ref["positional"].view(np.uint32)[~np.isnan(pos)])
            both = ~np.isnan(vis) & ~np.isnan(ref["visual"])
            assert (np.abs(vis[both] - ref["visual"][both]) <= 1e-5 + tol_rel * np.abs(ref["visual"][both])).all()
            np.testing.assert_array_equal(votes == abi.SA_VOTE_VISUAL, ref["voting_type"] == abi.SA_VOTE_VISUAL)
        else:
            check_visual(cfg, sc, tol_abs=1e-5 if visual == "cosine" else 0.0, tol_rel=tol_rel, epoch=epoch, kf=kf, own_area=own, det_present=dp)


def test_unique_optima_were_compared_by_id():
    """Runs after the sweep: among the frames whose assignment is compared by total gain (Mahalanobis SORT, carpets of equal overlaps) a
    fair share has a unique optimum — and those were compared id by id."""
    print("unique-optimum bookkeeping:", UNIQUE_CHECKS)
    if UNIQUE_CHECKS["frames"] == 0:
        pytest.skip("no frame went through the uniqueness check in this session")
    assert UNIQUE_CHECKS["unique"] >= 1, UNIQUE_CHECKS


def test_borderline_cells_stay_rare():
    """Runs last in this module: over every frame compare_visual saw, cells that sat on the is_ok threshold (present on one side
    only) and the rows whose id comparison they excused must be a vanishing share — otherwise the id gate is not a gate."""
    b = BORDERLINE
    print("borderline bookkeeping:", b)
    if b["frames"] == 0:
        pytest.skip("no visual frame was compared in this session")
    assert b["frames_with_borderline"] <= max(2, 0.05 * b["frames"]), b
    assert b["rows_excused"] <= 0.002 * max(1, b["rows_checked"]) + 4, b
