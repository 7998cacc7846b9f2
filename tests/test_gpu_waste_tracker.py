"""sa_tracker_waste_into on the MI355X (include/similari_waste.h): while a store is attached to a VisualSORT tracker, the feature bank
of every track that leaves the engine's table enters it, and nothing the tracker returns changes.

Two trackers run the same scripted frames, one with a store attached and one without.  Objects stand still and far apart and every
object has a direction of its own in feature space, so identities are trivial; features and qualities are known per frame, and
tests/bank_ref.py (the model the bank upkeep is held against) predicts every track's bank from its observation sequence.  After each
wasted() every reported id's bank in the store must be that bank with its present slots compacted in slot order — the rows bit for
bit, an f32 store keeps them as they are — and its attributes (scene, first epoch, last epoch); no track that can still match is in
the store.  Scenario (a): 6 objects in 2 scenes, seen for 1 to 5 frames, some frames without a feature, retired by the periodic
waste.  Scenario (b): 70 objects that vanish at once, retired by the eviction of expired rows inside predict()."""
import numpy as np
import pytest

import bank_ref as BR
from similari_amd import abi, trackers as T, waste as W
from similari_amd.engine import Engine
from similari_amd.retain import RetainStore

pytestmark = pytest.mark.gpu
u32, u64, f32 = np.uint32, np.uint64, np.float32
K, MAX_IDLE, PERIOD = 3, 2, 5


def tracker(D, device_upkeep, batch=False, devices=None):
    opts = (T.VisualSortOptions().max_idle_epochs(MAX_IDLE).kept_history_length(3).visual_metric(T.VisualSortMetricType.cosine(0.5))
            .positional_metric(T.PositionalMetricType.iou(0.3)).visual_minimal_track_length(1).visual_max_observations(K).visual_min_votes(1))
    o, keep = T.visual_options(opts, D, batch, 0, device_upkeep, 0, devices)
    o.auto_waste_periodicity = PERIOD
    return T._Tracker(o, keep)


def store_on(trk, D, depth=K):
    eng = Engine.borrowed(trk.lib, trk.lib.sa_tracker_engine(trk.h))
    return RetainStore(eng, "cosine", D, depth)


def box(obj):
    return T.Universal2DBox(100.0 + 300.0 * (obj % 10), 100.0 + 300.0 * (obj // 10), None, 0.5, 80.0, 1.0)


class Script:
    """What object `obj` shows in frame f (1-based): None when it is not there, else (feature or None, quality)."""

    def __init__(self, D, n_obj, seed):
        rng = np.random.default_rng(seed)
        self.D, self.rng = D, rng
        self.basis = np.linalg.qr(rng.standard_normal((max(D, n_obj), max(D, n_obj))))[0][:n_obj, :D] if n_obj <= D else None
        self.dirs = self.basis if self.basis is not None else rng.standard_normal((n_obj, D))
        self.seen = {}

    def obs(self, obj, f, featureless=False):
        if (obj, f) not in self.seen:
            feat = (self.dirs[obj] * 2.0 + self.rng.standard_normal(self.D) * 0.02).astype(f32)
            self.seen[(obj, f)] = (None if featureless else feat, float(f32(0.3 + 0.1 * ((obj * 7 + f * 3) % 6))))
        return self.seen[(obj, f)]


def expected_bank(D, sequence):
    """bank_ref over a track's observations [(feature or None, quality)], then the compaction of include/similari_waste.h."""
    bank = BR.Bank(K, D)
    for j, (feat, q) in enumerate(sequence):
        bank = BR.step(bank, j > 0, feat, q, 0.5, 80.0, None, 0.0, 0.0, 0.0)
    keep = bank.present != 0
    return bank.rows[keep], bank.quality[keep]


def same_tracks(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x == y, (x, y)


def check_wasted(store, D, wasted, history, epochs, seen_ids):
    """Every reported id's bank and attributes in the store."""
    if not wasted:
        return
    ids = np.array([t.id for t in wasted], u64)
    n_obs, feats, qual = store.fetch_raw(ids)
    attrs, known = store.get_attrs_raw(ids)
    assert known.all()
    for i, t in enumerate(wasted):
        rows, q = expected_bank(D, history[t.id])
        assert n_obs[i] == len(rows), (t.id, n_obs[i], len(rows))
        assert np.array_equal(feats[i, : n_obs[i]].view(u32), rows.view(u32)), t.id
        assert np.array_equal(qual[i, : n_obs[i]].view(u32), q.view(u32)), t.id
        first, last = epochs[t.id]
        assert (int(attrs[i]["key"]), int(attrs[i]["start"]), int(attrs[i]["end"])) == (t.scene_id, first, last) and last == t.epoch
        seen_ids.add(t.id)


def run(trk, ref, store, D, frames, scenes, script, schedule, batch=False, before_wasted=None):
    """frames x scenes of predict() on both trackers; schedule(scene, f) -> [(obj, featureless)].  -> ids wasted so far."""
    history, epochs, id_of, in_store = {}, {}, {}, set()
    for f in range(1, frames + 1):
        items = {s: [(obj, script.obs(obj, f, fl)) for obj, fl in schedule(s, f)] for s in scenes}
        outs = []
        for t in (trk, ref):
            if batch:
                req = T.PredictionBatchRequest()
                for s in scenes:
                    req.scenes.setdefault(s, [])   # (a scene without an object still moves its epoch on)
                    for obj, (feat, q) in items[s]:
                        req.add(s, T.VisualSortObservation(feat, q, box(obj)))
                got = {}
                if req.scenes:
                    res = t.predict_batch_async(req)
                    for _ in range(res.batch_size()):
                        sid, tracks = res.get()
                        got[sid] = tracks
                    res.close()
                outs.append({s: got.get(s, []) for s in scenes})
            else:
                outs.append({s: t.predict_with_scene(s, [T.VisualSortObservation(feat, q, box(obj)) for obj, (feat, q) in items[s]]) for s in scenes})
        for s in scenes:
            same_tracks(outs[0][s], outs[1][s])
            for (obj, ob), t in zip(items[s], outs[0][s]):
                assert id_of.setdefault((s, obj), t.id) == t.id and t.scene_id == s   # identities are trivial
                history.setdefault(t.id, []).append(ob)
                epochs[t.id] = (epochs.get(t.id, (t.epoch,))[0], t.epoch)
        if before_wasted:
            before_wasted(f)
        for s in scenes:
            same_tracks(trk.idle_tracks_with_scene(s), ref.idle_tracks_with_scene(s))
        wa, wb = trk.wasted(), ref.wasted()
        same_tracks(wa, wb)
        check_wasted(store, D, wa, history, epochs, in_store)
        # no track that can still match is in the store
        now = {s: trk.current_epoch_with_scene(s) for s in scenes}
        live = {tid for (s, _), tid in id_of.items() if epochs[tid][1] + MAX_IDLE >= now[s]}
        assert not live & {int(t) for t in store.order()}
    return in_store, id_of


# ---- (a) the periodic waste ----------------------------------------------------------------------
@pytest.mark.parametrize("device_upkeep", [True, False], ids=["device upkeep", "host upkeep"])
def test_wasted_tracks_are_in_the_store_with_their_banks(device_upkeep):
    D, scenes = 33, [3, 8]
    script = Script(D, 6, 1)
    life = {0: 1, 1: 2, 2: 3, 3: 4, 4: 5, 5: 5}   # frames an object is seen for

    def schedule(s, f):
        objs = [0, 1, 2] if s == 3 else [3, 4, 5]
        return [(o, (o + f) % 3 == 0 and not (o == 5 and f == 1)) for o in objs if f <= life[o]]   # every third observation has no feature

    trk, ref = tracker(D, device_upkeep), tracker(D, device_upkeep)
    store = store_on(trk, D)
    try:
        trk.waste_into(store, "latest")
        in_store, id_of = run(trk, ref, store, D, 12, scenes, script, schedule)
        assert in_store == set(id_of.values()) and len(in_store) == 6 == len(store)
        st = W.last(store)
        assert st["feature_bytes_h2d"] == 0 and st["feature_bytes_d2h"] == 0 and st["tracks"] >= 1
        # detached, the tracker removes as before: the store stays as it is
        trk.waste_into(None)
        before = store.order().tobytes()
        for f in range(5):
            same_tracks(trk.predict_with_scene(3, [T.VisualSortObservation(script.obs(0, 20 + f)[0], 0.5, box(0))]),
                        ref.predict_with_scene(3, [T.VisualSortObservation(script.obs(0, 20 + f)[0], 0.5, box(0))]))
        trk.skip_epochs_for_scene(3, 5), ref.skip_epochs_for_scene(3, 5)
        same_tracks(trk.wasted(), ref.wasted())
        assert store.order().tobytes() == before
    finally:
        store.close(), trk.close(), ref.close()


# ---- (b) the eviction of expired rows ------------------------------------------------------------
@pytest.mark.parametrize("device_upkeep", [True, False], ids=["device upkeep", "host upkeep"])
def test_evicted_rows_are_retired_at_eviction(device_upkeep):
    D, n = 8, 70
    script = Script(D, n + 1, 2)

    def schedule(s, f):
        return [(o, False) for o in range(n + 1)] if f == 1 else [(n, False)]   # 70 objects vanish at once, one stays

    trk, ref = tracker(D, device_upkeep), tracker(D, device_upkeep)
    store = store_on(trk, D)
    counts = []

    def before_wasted(f):
        # frame 4 is the first whose epoch the 70 tracks cannot match any more, and the periodic waste has not come round (the 6th
        # predict): the eviction inside predict() has taken the rows out of the table, and their banks are in the store already
        eng = Engine.borrowed(trk.lib, trk.lib.sa_tracker_engine(trk.h))
        counts.append((eng.count(0), len(store)))

    try:
        trk.waste_into(store, "latest")
        # (wasted() would waste them first: the frames up to the eviction run without it)
        history, epochs, ids = {}, {}, {}
        for f in range(1, 5):
            obs = [(o, script.obs(o, f)) for o, _ in schedule(0, f)]
            a = trk.predict_with_scene(0, [T.VisualSortObservation(feat, q, box(o)) for o, (feat, q) in obs])
            b = ref.predict_with_scene(0, [T.VisualSortObservation(feat, q, box(o)) for o, (feat, q) in obs])
            same_tracks(a, b)
            for (o, ob), t in zip(obs, a):
                assert ids.setdefault(o, t.id) == t.id
                history.setdefault(t.id, []).append(ob)
                epochs[t.id] = (epochs.get(t.id, (t.epoch,))[0], t.epoch)
            before_wasted(f)
        assert counts == [(n + 1, 0), (n + 1, 0), (n + 1, 0), (1, n)], counts
        same_tracks(trk.idle_tracks_with_scene(0), ref.idle_tracks_with_scene(0))
        wa, wb = trk.wasted(), ref.wasted()
        same_tracks(wa, wb)
        assert len(wa) == n
        seen = set()
        check_wasted(store, D, wa, history, epochs, seen)
        assert seen == {ids[o] for o in range(n)} and ids[n] not in {int(t) for t in store.order()}
    finally:
        store.close(), trk.close(), ref.close()


# ---- a batch tracker, three scenes through predict_batch_begin ----------------------------------
def test_a_batch_tracker_wastes_into_the_store():
    D, scenes = 33, [1, 2, 5]
    script = Script(D, 9, 3)

    def schedule(s, f):
        base = scenes.index(s) * 3
        return [(base + j, (j + f) % 4 == 3) for j in range(3) if f <= 1 + j + scenes.index(s)]

    trk, ref = tracker(D, True, batch=True), tracker(D, True, batch=True)
    store = store_on(trk, D, 5)   # a deeper store: Kp differs from the tracker's depth
    try:
        trk.waste_into(store, "latest", 3)
        in_store, id_of = run(trk, ref, store, D, 12, scenes, script, schedule, batch=True)
        assert in_store == set(id_of.values()) and len(in_store) == 9
    finally:
        store.close(), trk.close(), ref.close()


# ---- what is refused -----------------------------------------------------------------------------
def test_refused_trackers_and_stores():
    D = 33
    group = tracker(D, True, batch=True, devices=[0, 0])
    plain = T.Sort(device=0)
    trk, other = tracker(D, True), tracker(D, True)
    store, foreign, longer, shallow = store_on(trk, D), store_on(other, D), store_on(trk, D + 1), store_on(trk, D, K - 1)
    on_group = store_on(group, D)
    try:
        for t, s, kw, code, text in [(group, on_group, {}, abi.SA_ERR_UNSUPPORTED, "one store per shard"),
                                     (plain, store, {}, abi.SA_ERR_BAD_ARG, "VisualSORT"),
                                     (trk, foreign, {}, abi.SA_ERR_BAD_ARG, "another engine"),
                                     (trk, longer, {}, abi.SA_ERR_BAD_ARG, "feature_len"),
                                     (trk, shallow, {}, abi.SA_ERR_BAD_ARG, "bank depth"),
                                     (trk, store, dict(keep=9), abi.SA_ERR_BAD_ARG, "unknown keep"),
                                     (trk, store, dict(capacity=K + 1), abi.SA_ERR_BAD_ARG, "capacity")]:
            with pytest.raises(T.TrackerError) as err:
                t.waste_into(s, **kw)
            assert "error %d:" % code in str(err.value) and text in str(err.value), str(err.value)
        trk.waste_into(store, "best", K)
        trk.waste_into(None)
    finally:
        for s in (store, foreign, longer, shallow, on_group):
            s.close()
        for t in (group, plain, trk, other):
            t.close()
