"""A slot's result block (similari_amd/csrc/sa_slot_out.h) read through every call that hands it out.  Frames of 0, 1, 7, 8 and 9
candidates against 5 tracks — the sizes around the 8-byte rounding of the 9 n bytes of ids and votes, where a wrong offset first shows —
in ONE request set, so that an empty scene lies beside non-empty ones: sa_batch_fetch + sa_batch_fetch_cols, sa_batch_results and
sa_pipe_wait must hand out the same winners, vote types and columns, the oracle's; then the upkeep step (sa_tracks_apply on one set,
sa_batch_run_apply + sa_tracks_apply_collect on another) reads winners and columns out of the same block."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from similari_amd import abi, synth
from similari_amd.engine import Engine

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 7, 8, 9]
T = 5
PW, VW = np.float32(1 / 20), np.float32(1 / 160)
u64p, u8p, i32p, boxp, fp = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(abi.sa_box), C.POINTER(C.c_float)


def scene_id(n):
    return 10 + n


def make_set(rng, visual):
    """{n: (tracks, detections)}: 5 tracks per scene, n detections (the first min(n, 5) over tracks, in shuffled order, the rest new)."""
    out = {}
    for n in COUNTS:
        if visual:
            sc = synth.visual_scene(rng, T, n, 8, 1, canvas=(900.0, 700.0))
            tr = abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"], feat_present=sc["track_present"])
            det = abi.make_detections(sc["det_boxes"], feats=sc["det_feats"], feat_quality=sc["det_quality"])
        else:
            sc = synth.sort_scene(rng, T, n, canvas=(900.0, 700.0))
            tr = abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"])
            det = abi.make_detections(sc["det_boxes"])
        out[n] = (tr, det)
    return out


def columns_of(order, ids):
    col = {int(t): k for k, t in enumerate(order)}
    return np.array([col[int(t)] if t else -1 for t in ids], np.int32)


@pytest.mark.parametrize("visual", [False, True])
def test_every_fetch_call_hands_out_the_same_block(visual):
    rng = np.random.default_rng(500 + visual)
    cfg = (abi.make_config(positional="iou", positional_threshold=0.3, visual="cosine", visual_threshold=0.3, feature_len=8, max_observations=1,
                           visual_min_votes=1, visual_minimal_track_length=1, positional_min_confidence=0.1, max_idle_epochs=5)
           if visual else abi.make_config(positional="iou", positional_threshold=0.3, max_idle_epochs=5))
    data = make_set(rng, visual)
    eng = Engine(cfg)
    try:
        for n, (tr, _) in data.items():
            eng.upsert(scene_id(n), tr)
        ref = {n: O.associate(cfg, tr, 1, det, want_matrices=False) for n, (tr, det) in data.items()}
        assert sum(int((ref[n]["track_id"] != 0).sum()) for n in COUNTS) >= 12       # (the frames do match their tracks)
        want = {n: (ref[n]["track_id"], ref[n]["voting_type"], columns_of(eng.order(scene_id(n)), ref[n]["track_id"])) for n in COUNTS}

        def fetched(slot, n):
            ids, votes = eng.batch_fetch(slot, n)
            cols = np.full(n, 77, np.int32)
            eng._chk(eng.lib.sa_batch_fetch_cols(eng.h, slot, cols.ctypes.data_as(i32p)))
            return ids, votes, cols

        def viewed(slot, n):
            pi, pv, pc = u64p(), u8p(), i32p()
            eng._chk(eng.lib.sa_batch_results(eng.h, slot, C.byref(pi), C.byref(pv), C.byref(pc)))
            assert pi and pv and pc
            if not n:
                return np.zeros(0, np.uint64), np.zeros(0, np.uint8), np.zeros(0, np.int32)
            return np.ctypeslib.as_array(pi, (n,)).copy(), np.ctypeslib.as_array(pv, (n,)).copy(), np.ctypeslib.as_array(pc, (n,)).copy()

        def same(got, n, what):
            for g, w, name in zip(got, want[n], ("winners", "vote types", "columns")):
                np.testing.assert_array_equal(g, w, err_msg=f"{what}, n = {n}: {name}")

        # the synchronous set
        eng.batch_begin()
        slots = {n: eng.batch_add(scene_id(n), 1, det) for n, (_, det) in data.items()}
        eng.batch_run()
        for n in COUNTS:
            same(viewed(slots[n], n), n, "sa_batch_results")
            same(fetched(slots[n], n), n, "sa_batch_fetch + _cols")
        # the same request as a ticket: sa_pipe_wait's copies, then its bank through the two other calls
        req, res, outs = Engine.make_requests([(scene_id(n), 1, det) for n, (_, det) in data.items()])
        eng.pipe_wait(eng.pipe_submit(req), res)
        for k, n in enumerate(COUNTS):
            np.testing.assert_array_equal(outs[k][0], want[n][0], err_msg=f"sa_pipe_wait, n = {n}")
            np.testing.assert_array_equal(outs[k][1], want[n][1], err_msg=f"sa_pipe_wait, n = {n}")
            same(fetched(k, n), n, "sa_batch_fetch + _cols of a ticket")
            same(viewed(k, n), n, "sa_batch_results of a ticket")
    finally:
        eng.close()


def upkeep_set(rng):
    """{n: (ids, boxes, mean10, cov100, detections)}: scene n's track 2 (and the detection over it) is oriented."""
    out = {}
    for n in COUNTS:
        sc = synth.sort_scene(rng, T, n, canvas=(900.0, 700.0))
        tb, db = sc["track_boxes"], sc["det_boxes"]
        tb["angle"][2], tb["has_angle"][2] = 0.3, 1
        for i in np.nonzero(sc["truth"] == 3)[0]:
            db["angle"][i], db["has_angle"][i] = 0.31, 1
        mean = np.zeros((T, 10), np.float32)
        for f, k in (("xc", 0), ("yc", 1), ("angle", 2), ("aspect", 3), ("height", 4)):
            mean[:, k] = tb[f]
        cov = np.tile(np.diag(np.full(10, 4.0, np.float32)).ravel(), (T, 1)).astype(np.float32)
        out[n] = (sc["track_ids"], tb, mean, cov, db)
    return out


def seeded(cfg, data):
    eng = Engine(cfg)
    for n, (ids, tb, mean, cov, _) in data.items():
        eng.upsert(scene_id(n), abi.make_tracks(ids, tb, np.zeros(T, np.uint64)))
        for k, tid in enumerate(ids):
            eng._chk(eng.lib.sa_tracks_set_state(eng.h, scene_id(n), int(tid), mean[k].ctypes.data_as(fp), cov[k].ctypes.data_as(fp), None))
    return eng


def test_upkeep_reads_winners_and_columns_out_of_the_block():
    """sa_tracks_apply (new ids from the caller) on one engine, sa_batch_run_apply + sa_tracks_apply_collect (ids drawn on the device) on
    another, the same frames: the oracle's winners, the oracle's filter step for every candidate (predict + update of the winner's state, a
    fresh state for a track that starts), the ids base + 1 + candidate index, the same tables and polygons on both — the oriented row's
    through the polygon fix-up."""
    L = O.lib()
    rng = np.random.default_rng(510)
    cfg = abi.make_config(positional="iou", positional_threshold=0.3, max_idle_epochs=5)
    data = upkeep_set(rng)
    a, b = seeded(cfg, data), seeded(cfg, data)
    try:
        dets = {n: abi.make_detections(data[n][4]) for n in COUNTS}
        ref = {n: O.associate(cfg, abi.make_tracks(data[n][0], data[n][1], np.zeros(T, np.uint64)), 1, dets[n], want_matrices=False)["track_id"] for n in COUNTS}
        assert any(3 in ref[n] for n in COUNTS)                                    # (an oriented row is refreshed)
        base = {n: 1000 * (n + 1) for n in COUNTS}
        new_ids = {n: np.where(ref[n] == 0, base[n] + 1 + np.arange(n), 0).astype(np.uint64) for n in COUNTS}
        want_pred = {}
        for n in COUNTS:
            ids, tb, mean, cov, db = data[n]
            row = {int(t): k for k, t in enumerate(ids)}
            wp = np.zeros(n, abi.BOX_DTYPE)
            for i in range(n):
                sb, ob = np.zeros(1, abi.BOX_DTYPE), db[i:i + 1].copy()
                if ref[n][i]:
                    k = row[int(ref[n][i])]
                    m, c = mean[k].copy(), cov[k].copy()
                    L.or_make_prediction(PW, VW, 1, O.fptr(m), O.fptr(c), O.box_ptr(ob), O.box_ptr(sb))
                else:
                    m, c = np.zeros(10, np.float32), np.zeros(100, np.float32)
                    L.or_make_prediction(PW, VW, 0, O.fptr(m), O.fptr(c), O.box_ptr(ob), O.box_ptr(sb))
                wp[i] = sb[0]
            want_pred[n] = wp
        # a: fetch, then sa_tracks_apply with the caller's ids
        a.batch_begin()
        slots = {n: a.batch_add(scene_id(n), 1, dets[n]) for n in COUNTS}
        a.batch_run()
        got_a = {}
        for n in COUNTS:
            ids, _ = a.batch_fetch(slots[n], n)
            np.testing.assert_array_equal(ids, ref[n], err_msg=f"n = {n}")
            pred = np.zeros(n, abi.BOX_DTYPE)
            a._chk(a.lib.sa_tracks_apply(a.h, slots[n], new_ids[n].ctypes.data_as(u64p), C.cast(pred.ctypes.data, boxp)))
            got_a[n] = pred
        # b: the upkeep queued behind the association, ids drawn on the device
        b.batch_begin()
        slots = {n: b.batch_add(scene_id(n), 1, dets[n]) for n in COUNTS}
        bases = np.array([base[n] for n in COUNTS], np.uint64)
        b._chk(b.lib.sa_batch_run_apply(b.h, bases.ctypes.data_as(u64p), 1))
        for n in COUNTS:
            nid, pred = np.full(n, 77, np.uint64), np.zeros(n, abi.BOX_DTYPE)
            b._chk(b.lib.sa_tracks_apply_collect(b.h, slots[n], nid.ctypes.data_as(u64p), C.cast(pred.ctypes.data, boxp)))
            np.testing.assert_array_equal(nid, new_ids[n], err_msg=f"n = {n}")
            for f in ("xc", "yc", "angle", "aspect", "height"):
                np.testing.assert_array_equal(pred[f], want_pred[n][f], err_msg=f"collect, n = {n}: {f}")
                np.testing.assert_array_equal(got_a[n][f], want_pred[n][f], err_msg=f"apply, n = {n}: {f}")
        for n in COUNTS:
            sc = scene_id(n)
            np.testing.assert_array_equal(a.order(sc), np.concatenate([data[n][0], new_ids[n][new_ids[n] != 0]]))
            np.testing.assert_array_equal(b.order(sc), a.order(sc))
            pa, pb = a.tap_track_polygons(sc), b.tap_track_polygons(sc)
            np.testing.assert_array_equal(pa.view(np.uint64), pb.view(np.uint64), err_msg=f"n = {n}")
            if 3 in ref[n]:   # the refreshed oriented row: a rotated rectangle about the predicted centre, not an axis-aligned one
                i = int(np.nonzero(ref[n] == 3)[0][0])
                np.testing.assert_allclose(pa[2].mean(axis=0), [want_pred[n]["xc"][i], want_pred[n]["yc"][i]], atol=1e-3)
                edge = pa[2][1] - pa[2][0]
                assert abs(edge[0]) > 1e-3 and abs(edge[1]) > 1e-3
    finally:
        a.close()
        b.close()
