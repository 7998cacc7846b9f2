"""Device-side feature-bank upkeep (similari_amd/csrc/sa_upkeep.hip: bank_block<KMAX>) against the numpy model of the policy
(tests/bank_ref.py), in every bank-depth class and at row widths on both sides of the row loop's first turn.

A raw engine runs a short scripted sequence with device upkeep.  After every frame every track's bank is read back
(sa_tracks_get_state: quality, present, K x D rows) and compared BIT FOR BIT, in slot order, with the model fed the same events — the
engine's own winners are the model's input, so the upkeep is checked and not the vote.  What get_state does not return — the rows'
squared norms and the bank's fragment-order twin — is checked through the next frame: a twin engine is given the model's banks fresh
through sa_tracks_upsert, and the two engines' visual cells (sa_tap_visual), the vote words of their own first phases (sa_tap_votes) and
their winners must be the same bits; the cells are also held against f64 distances over the model's rows within the bound
tests/test_gpu_parity.py applies to sa_tap_visual (cosine 1e-5 absolute, euclidean 1e-5 relative + 1e-6).

  K  1, 3, 4   k_apply_visual<4>  / k_apply_bank_set<4>
  K  5, 8      k_apply_visual<8>  / k_apply_bank_set<8>       (4 | 5 and 8 | 9: both sides of each class edge)
  K  9, 16     k_apply_visual<16> / k_apply_bank_set<16>
  D  32        rows need no padding (D == Dp); 48: padded rows, norms from the frame's preparation; 260: Dp = 288, the row loop's second
               turn with 32 of 256 threads live; 512: two full turns.
test_bank_upkeep_single_scene runs sa_tracks_apply (k_apply_visual<KMAX>, Kalman and bank blocks in one launch);
test_bank_upkeep_entry_points adds sa_tracks_apply_begin / _end (part 1, then part 2: k_apply_visual<KMAX> with the bank blocks alone, at
K = 4, 5, 8, 9 and 16) and sa_batch_run_apply + sa_tracks_apply_collect (k_apply_bank_set<KMAX> over a request set of three scenes of
different sizes, one of them a single detection, one sitting a frame out) and requires the three to leave the same bits."""
import ctypes as C

import numpy as np
import pytest

import bank_ref as BR
from similari_amd import abi
from similari_amd.engine import Engine

pytestmark = pytest.mark.gpu

MIN_AREA, Q_USE, Q_COLLECT, OWN_USE, OWN_COLLECT = 500.0, 0.2, 0.5, 0.1, 0.5
GATES = dict(minimal_area=MIN_AREA, q_collect=Q_COLLECT, own_collect=OWN_COLLECT)
THR = {"cosine": 0.5, "euclidean": 0.7}
N_IDENT = 30
MAXDEV = {"cosine": 0.0, "euclidean": 0.0}    # largest deviation of a cell from f64 over the whole module (printed per test)
U64P, BOXP, FP, U8P = C.POINTER(C.c_uint64), C.POINTER(abi.sa_box), C.POINTER(C.c_float), C.POINTER(C.c_uint8)


def padded(D):
    """The engine's row length: the next multiple of 32 floats (the engine has no call that reports it; sa_engine_create sets it)."""
    return (D + 31) // 32 * 32


def config(metric, K, D):
    return abi.make_config(positional="iou", positional_threshold=0.3, positional_min_confidence=0.1, visual=metric, visual_threshold=THR[metric],
                           feature_len=D, max_observations=K, visual_min_votes=1, visual_minimal_track_length=1, visual_minimal_area=MIN_AREA,
                           visual_minimal_quality_use=Q_USE, visual_minimal_own_area_percentage_use=OWN_USE,
                           visual_minimal_quality_collect=Q_COLLECT, visual_minimal_own_area_percentage_collect=OWN_COLLECT,
                           max_idle_epochs=5, flags=abi.SA_FLAG_TAP)


def role(i, f):
    """What identity i brings to frame f: (has a feature, quality, small box, own-area share | None), or None when it is not in the frame.
    Qualities come from four levels, two of them equal, so banks hold ties."""
    has, q, small, own = True, (0.6, 0.8, 0.8, 0.9)[(i + f) % 4], False, None
    if i in (12, 13) and f % 3 == 1:
        q = 0.3                     # usable for the vote, below the collect gate
    elif i == 14 and f % 2 == 1:
        q = 0.1                     # not even usable: the positional vote finds its track
    elif i == 15:
        small = True                # a box under visual_minimal_area, always
    elif i in (16, 17) and f % 3 == 2:
        has = False                 # a merge without a feature
    elif i == 18 and f == 0:
        q = 0.1                     # a track that starts with a poor observation keeps it
    elif i == 19 and f == 0:
        has = False                 # a track that starts without a feature
    elif i == 20:
        has = False                 # never a feature
    elif i in (21, 22) and f % 4 == 2:
        return None                 # sits the frame out
    elif i == 23:
        own = 0.3 if f % 2 == 0 else 0.9   # every other frame its own-area share is under the collect gate
    elif 24 <= i <= 27:             # late arrivals
        if f < i - 22:
            return None
        if f == i - 22 and i == 25:
            q = 0.3
        if f == i - 22 and i == 26:
            has = False
    elif i >= 28:
        return None
    return has, q, small, own


def scenario(seed, K, D, metric, idents, skip=()):
    """K + 3 frames (a bank fills, drops its lowest row and rotates) of the identities `idents`, each frame in a fresh random order.
    Identities are orthonormal directions, an observation is its identity plus noise of length ~0.1 — its own track's rows lie at
    cosine ~0.995 / distance ~0.14, every other track's at ~0 / ~1.4: no cell anywhere near the threshold.  Cosine observations are
    scaled by 0.5 .. 2, so every row has a norm of its own.  Returns one dict per frame (None for a frame in `skip`)."""
    rng = np.random.default_rng(seed)
    basis = np.linalg.qr(rng.standard_normal((D, N_IDENT)))[0].T
    frames = []
    for f in range(K + 3):
        here = [(i, role(i, f)) for i in idents if role(i, f) is not None]
        here = [here[j] for j in rng.permutation(len(here))]
        n = len(here)
        xc = np.array([(i % 6) * 220.0 + 100.0 for i, _ in here]) + rng.uniform(-0.5, 0.5, n)
        yc = np.array([(i // 6) * 220.0 + 100.0 for i, _ in here]) + rng.uniform(-0.5, 0.5, n)
        small = np.array([r[2] for _, r in here])
        boxes = abi.make_boxes(xc, yc, np.full(n, 0.5), np.where(small, 24.0, 80.0))       # areas 288 and 3200
        feats = basis[[i for i, _ in here]] + rng.standard_normal((n, D)) * (0.1 / np.sqrt(D))
        if metric == "cosine":
            feats *= rng.uniform(0.5, 2.0, (n, 1))
        has = np.array([r[0] for _, r in here], np.uint8)
        feats = (feats * has[:, None]).astype(np.float32)
        fr = dict(ident=[i for i, _ in here], boxes=boxes, feats=feats, has=has, quality=np.array([r[1] for _, r in here], np.float32),
                  own=np.array([np.nan if r[3] is None else r[3] for _, r in here], np.float32))
        fr["det"] = abi.make_detections(boxes, feats=feats, feat_present=has, feat_quality=fr["quality"], own_area=fr["own"])
        frames.append(None if f in skip else fr)
    return frames


class Table:
    """The model of one scene's track table: ids in table order (new tracks are appended in candidate order), every track's bank
    (bank_ref), predicted box and epoch, and the events the sequence has met."""

    def __init__(self, K, D):
        self.K, self.D, self.order, self.bank, self.box, self.epoch, self.events = K, D, [], {}, {}, {}, set()

    def apply(self, fr, epoch, tids, pred):
        ev = self.events
        if set(self.order) - {int(t) for t in tids}:
            ev.add("a track sits the frame out")
        for i, tid in enumerate(int(t) for t in tids):
            merged = tid in self.bank
            old = self.bank[tid] if merged else BR.Bank(self.K, self.D)
            has, q = bool(fr["has"][i]), fr["quality"][i]
            own = None if np.isnan(fr["own"][i]) else fr["own"][i]
            asp, hgt = fr["boxes"]["aspect"][i], fr["boxes"]["height"][i]
            new = BR.step(old, merged, fr["feats"][i] if has else None, q, asp, hgt, own, **GATES)
            big = np.float32(asp * hgt) * hgt >= MIN_AREA
            if merged:
                ev.add("merge, collected" if new.present[0] else "merge, no feature" if not has else "merge, small box" if not big
                       else "merge, below the quality gate" if q < Q_COLLECT else "merge, below the own-area gate")
                if old.count == self.K:
                    lost = set(range(self.K)) - {s for s in new.src if s != BR.NEW}
                    assert new.src[0] == BR.NEW and len(lost) == 1 and old.quality[lost.pop()] == old.quality.min()
                    ev.add("merge into a full bank")
            else:
                self.order.append(tid)
                ev.add("new, no feature" if not has else "new, low quality kept" if q < Q_COLLECT else "new")
            pq = new.quality[new.present != 0]
            if len(set(pq.tolist())) < len(pq):
                ev.add("ties in a bank")
            self.bank[tid], self.box[tid], self.epoch[tid] = new, pred[i], epoch

    def tracks(self):
        ids = np.array(self.order, np.uint64)
        return abi.make_tracks(ids, np.array([self.box[t] for t in self.order], abi.BOX_DTYPE), [self.epoch[t] for t in self.order],
                               feats=np.stack([self.bank[t].rows for t in self.order]), feat_present=np.stack([self.bank[t].present for t in self.order]))


EVENTS = {"merge, collected", "merge, no feature", "merge, small box", "merge, below the quality gate", "merge, below the own-area gate",
          "merge into a full bank", "new", "new, no feature", "new, low quality kept", "a track sits the frame out", "ties in a bank"}


def expected_cells(metric, fr, tab):
    """[n, T, K] f64 weights (cosine: 1 - cos, euclidean: the distance) of the frame's candidates against the model's banks, NaN where the
    reference has no visual cell: the candidate's feature may not be USED, a slot holds no feature, the distance fails the threshold."""
    n, T, K = len(fr["ident"]), len(tab.order), tab.K
    out = np.full((n, T, K), np.nan)
    use = np.array([bool(fr["has"][i]) and BR.feature_can_be_used(MIN_AREA, fr["boxes"]["aspect"][i], fr["boxes"]["height"][i], fr["quality"][i], Q_USE,
                                                                 None if np.isnan(fr["own"][i]) else fr["own"][i], OWN_USE) for i in range(n)])
    a = fr["feats"].astype(np.float64)
    for j, tid in enumerate(tab.order):
        bk = tab.bank[tid]
        for k in np.nonzero(bk.present)[0]:
            b = bk.rows[k].astype(np.float64)
            if metric == "cosine":
                cos = (a[use] @ b) / np.sqrt((a[use] * a[use]).sum(1) * (b @ b))
                assert (np.abs(cos - THR[metric]) > 0.05).all()                 # nothing near the threshold: the NaN pattern is decided
                out[use, j, k] = np.where(cos >= THR[metric], 1.0 - cos, np.nan)
            else:
                dist = np.sqrt(((a[use] - b) ** 2).sum(1))
                assert (np.abs(dist - THR[metric]) > 0.1).all()
                out[use, j, k] = np.where(dist <= THR[metric], dist, np.nan)
    return out


def check_cells(metric, eng, twin, scene, epoch, fr, tab):
    """The frame's association on the engine under test and on a twin whose table is the model's, given fresh by sa_tracks_upsert: same
    winners, same vote words, same visual cells bit for bit — rows, norms and the fragment-order twin of the device-kept bank are what a
    fresh upload makes of the model's rows — and the cells within the parity bound of f64."""
    ids, votes = eng.associate(scene, epoch, fr["det"])
    if not tab.order:
        return ids, votes
    vis, vt = eng.tap_visual(), eng.tap_votes()
    np.testing.assert_array_equal(eng.order(scene), np.array(tab.order, np.uint64))
    twin.upsert(scene, tab.tracks())
    ids2, votes2 = twin.associate(scene, epoch, fr["det"])
    vis2, vt2 = twin.tap_visual(), twin.tap_votes()
    np.testing.assert_array_equal(np.isnan(vis), np.isnan(vis2), err_msg=f"epoch {epoch}: NaN pattern of the cells")
    m = ~np.isnan(vis)
    np.testing.assert_array_equal(vis[m].view(np.uint32), vis2[m].view(np.uint32), err_msg=f"epoch {epoch}: cells against the twin engine")
    for x, y in zip(vt, vt2):
        np.testing.assert_array_equal(x, y, err_msg=f"epoch {epoch}: vote words against the twin engine")
    np.testing.assert_array_equal(ids, ids2)
    np.testing.assert_array_equal(votes, votes2)
    ref = expected_cells(metric, fr, tab)
    np.testing.assert_array_equal(m, ~np.isnan(ref), err_msg=f"epoch {epoch}: NaN pattern against the model")
    assert m.any()
    dev = np.abs(vis[m] - ref[m])
    MAXDEV[metric] = max(MAXDEV[metric], float(dev.max()))
    if metric == "cosine":
        assert (dev <= 1e-5).all(), dev.max()
    else:
        assert (dev <= 1e-5 * ref[m] + 1e-6).all(), (dev / ref[m]).max()
    return ids, votes


def read_banks(eng, scene, tab):
    out = {}
    for tid in tab.order:
        q, p, ft = np.zeros(tab.K, np.float32), np.zeros(tab.K, np.uint8), np.zeros((tab.K, tab.D), np.float32)
        eng._chk(eng.lib.sa_tracks_get_state(eng.h, scene, tid, None, None, q.ctypes.data_as(FP), p.ctypes.data_as(U8P), ft.ctypes.data_as(FP)))
        out[tid] = (q, p, ft)
    return out


def check_banks(got, tab, what):
    """rows, presence flags and qualities bit for bit in slot order; a slot the model leaves empty reads present 0, quality 0, a zero row
    (the model's own arrays are zero there)"""
    for tid in tab.order:
        (q, p, ft), bk = got[tid], tab.bank[tid]
        np.testing.assert_array_equal(p, bk.present, err_msg=f"{what} track {tid}: present (sources {bk.src})")
        np.testing.assert_array_equal(q.view(np.uint32), bk.quality.view(np.uint32), err_msg=f"{what} track {tid}: qualities (sources {bk.src})")
        np.testing.assert_array_equal(ft.view(np.uint32), bk.rows.view(np.uint32), err_msg=f"{what} track {tid}: rows (sources {bk.src})")
        for k, s in enumerate(bk.src):
            if s is BR.EMPTY:
                assert p[k] == 0 and q[k].view(np.uint32) == 0 and not ft[k].view(np.uint32).any()


def snapshot(got, tab):
    return b"".join(got[t][0].tobytes() + got[t][1].tobytes() + got[t][2].tobytes() for t in tab.order)


def run(entry, metric, K, D, seed):
    """One sequence through one entry point: "apply" (sa_tracks_apply), "halves" (sa_tracks_apply_begin / _end), "set" (sa_batch_run_apply +
    sa_tracks_apply_collect over three scenes).  Every candidate i of frame f that starts a track gets the id 100 f + 1 + i — the rule
    sa_batch_run_apply draws ids by (one per candidate), so the three entry points build the same tables.  Returns scene 0's banks after
    every frame, as bytes, and its winners."""
    assert padded(D) == {32: 32, 48: 64, 260: 288, 512: 512}[D] and (padded(D) > 256) == (D > 256)
    cfg = config(metric, K, D)
    scenes = {0: scenario(seed, K, D, metric, range(N_IDENT))}
    if entry == "set":
        scenes[1] = scenario(seed + 1, K, D, metric, range(7), skip=(2,))   # a smaller scene, which sits frame 2 out
        scenes[2] = scenario(seed + 2, K, D, metric, [0])                   # a single detection: every other block of its row leaves at once
    tabs = {sc: Table(K, D) for sc in scenes}
    eng, twin = Engine(cfg), Engine(cfg)
    shots, winners = [], []
    try:
        for f in range(K + 3):
            epoch = f + 1
            live = [sc for sc in scenes if scenes[sc][f] is not None]
            probe = {sc: check_cells(metric, eng, twin, sc, epoch, scenes[sc][f], tabs[sc]) for sc in live}
            res = {}
            if entry == "set":
                eng.batch_begin()
                slots = {sc: eng.batch_add(sc, epoch, scenes[sc][f]["det"]) for sc in live}
                base = np.full(len(live), 100 * f, np.uint64)
                eng._chk(eng.lib.sa_batch_run_apply(eng.h, base.ctypes.data_as(U64P), 1))
                eng.batch_sync()
                for sc in live:
                    n = scenes[sc][f]["det"].n
                    ids, votes = eng.batch_fetch(slots[sc], n)
                    nid, pred = np.zeros(n, np.uint64), np.zeros(n, abi.BOX_DTYPE)
                    eng._chk(eng.lib.sa_tracks_apply_collect(eng.h, slots[sc], nid.ctypes.data_as(U64P), C.cast(pred.ctypes.data, BOXP)))
                    np.testing.assert_array_equal(nid, np.where(ids == 0, 100 * f + 1 + np.arange(n), 0).astype(np.uint64))
                    res[sc] = (ids, votes, nid, pred)
            else:
                fr = scenes[0][f]
                n = fr["det"].n
                ids, votes = eng.associate(0, epoch, fr["det"])     # (staged afresh: the probe's taps prepared the slot, this frame is as the plan runs it)
                nid, pred = np.where(ids == 0, 100 * f + 1 + np.arange(n), 0).astype(np.uint64), np.zeros(n, abi.BOX_DTYPE)
                if entry == "apply":
                    eng._chk(eng.lib.sa_tracks_apply(eng.h, 0, nid.ctypes.data_as(U64P), C.cast(pred.ctypes.data, BOXP)))
                else:
                    eng._chk(eng.lib.sa_tracks_apply_begin(eng.h, 0, nid.ctypes.data_as(U64P)))
                    eng._chk(eng.lib.sa_tracks_apply_end(eng.h, 0, C.cast(pred.ctypes.data, BOXP)))
                res[0] = (ids, votes, nid, pred)
            for sc in live:
                ids, votes, nid, pred = res[sc]
                np.testing.assert_array_equal(ids, probe[sc][0])
                np.testing.assert_array_equal(votes, probe[sc][1])
                tabs[sc].apply(scenes[sc][f], epoch, np.where(ids == 0, nid, ids), pred)
                got = read_banks(eng, sc, tabs[sc])
                check_banks(got, tabs[sc], f"{entry}, scene {sc}, frame {f},")
                if sc == 0:
                    shots.append(snapshot(got, tabs[sc]))
                    winners.append(ids)
        assert tabs[0].events >= (EVENTS if K > 1 else EVENTS - {"ties in a bank"}), EVENTS - tabs[0].events
        full = [t for t in tabs[0].order if tabs[0].bank[t].count == K]
        assert len(full) >= 8, "banks must have filled"
    finally:
        eng.close()
        twin.close()
    print(f"\n{entry} {metric} K={K} D={D} (Dp={padded(D)}): largest |cell - f64| so far: cosine {MAXDEV['cosine']:.3g}, euclidean {MAXDEV['euclidean']:.3g}")
    return shots, winners


SINGLE = [(1, 32, "cosine"), (1, 512, "euclidean"), (3, 48, "euclidean"), (3, 260, "cosine"), (4, 260, "euclidean"), (5, 32, "euclidean"),
          (5, 260, "cosine"), (8, 512, "cosine"), (9, 32, "cosine"), (16, 48, "cosine"), (16, 260, "euclidean")]
ENTRIES = [(4, 48, "cosine"), (5, 512, "cosine"), (8, 48, "euclidean"), (9, 260, "euclidean"), (16, 512, "cosine")]


@pytest.mark.parametrize("K,D,metric", SINGLE)
def test_bank_upkeep_single_scene(K, D, metric):
    """sa_tracks_apply: k_apply_visual<4> at K = 1, 3, 4, k_apply_visual<8> at K = 5, 8, k_apply_visual<16> at K = 9, 16; every class at
    a narrow row (one turn of the row loop) and a wide one (D = 260: the second turn with 32 threads live; D = 512: two full turns)."""
    run("apply", metric, K, D, seed=1000 * K + D)


@pytest.mark.parametrize("K,D,metric", ENTRIES)
def test_bank_upkeep_entry_points(K, D, metric):
    """The same sequence through sa_tracks_apply (k_apply_visual<KMAX>), sa_tracks_apply_begin / _end (the part == 2 launch: the bank blocks
    of k_apply_visual<KMAX> alone — <8> at K = 5 and 8, <16> at K = 9 and 16) and sa_batch_run_apply + sa_tracks_apply_collect
    (k_apply_bank_set<4> at K = 4, <8> at K = 5 and 8, <16> at K = 9 and 16; three scenes of 20-odd, seven and one detection, the second
    sitting a frame out).  Each is held against the model frame by frame inside run(); here the three must agree among themselves."""
    seed = 1000 * K + D
    a, wa = run("apply", metric, K, D, seed)
    for entry in ("halves", "set"):
        b, wb = run(entry, metric, K, D, seed)
        assert len(a) == len(b) == K + 3
        for f, (x, y) in enumerate(zip(wa, wb)):
            np.testing.assert_array_equal(x, y, err_msg=f"{entry}: winners of frame {f}")
        assert [x == y for x, y in zip(a, b)] == [True] * (K + 3), f"{entry}: banks differ from sa_tracks_apply's"
