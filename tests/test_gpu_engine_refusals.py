"""The engine's refusals, word for word: code, text and untouched outputs of the calls that share a prologue in sa_engine.hip (the slot
look-up, the "... before sa_batch_run" checks, the five add calls and the associate pairs, the upkeep step's checks).  Plain SORT, a
table of 3 tracks, frames of 2 boxes.  The texts are written out here; they are the library's contract with callers that match on them."""
import ctypes as C

import numpy as np
import pytest

from similari_amd import abi, framerows
from similari_amd.engine import Engine

pytestmark = pytest.mark.gpu

BAD, STATE = abi.SA_ERR_BAD_ARG, abi.SA_ERR_STATE
SCENE = 7
u64p, u8p, i32p, u32p, boxp = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(abi.sa_box)
OUT_OF_RANGE = "slot 5 out of range (1 staged)"
NULL_BOXES = "detections.boxes is null"
BAD_ASPECT = "detections.boxes[1]: aspect and height must be > 0 (bbox.rs:453-456)"
BAD_CONFIDENCE = "detections.boxes[1]: confidence must lie in [0, 1] (bbox.rs:123-126)"


def frame(far=False, **bad):
    """Two boxes over the first two tracks (far: away from every track, so both start tracks); bad: a field of box 1 overwritten."""
    b = abi.make_boxes([102.0, 301.0], [900.0, 900.0] if far else [101.0, 99.0], [0.5, 0.5], [80.0, 80.0])
    for f, v in bad.items():
        b[f][1] = v
    return b


@pytest.fixture(scope="module")
def eng():
    e = Engine(abi.make_config(positional="iou", positional_threshold=0.3, max_idle_epochs=5))
    framerows.bind(e.lib)
    e.upsert(SCENE, abi.make_tracks([1, 2, 3], abi.make_boxes([100.0, 300.0, 500.0], [100.0] * 3, [0.5] * 3, [80.0] * 3), [0, 0, 0]))
    yield e
    e.close()


def err(e):
    return e.lib.sa_last_error(e.h).decode()


def refused(e, rc, code, text):
    assert rc == code, (rc, err(e))
    assert err(e) == text


def staged(e, boxes=None):
    """A fresh request set with one scene of two boxes, not run: (detections, slot)."""
    det = abi.make_detections(frame() if boxes is None else boxes)
    e.batch_begin()
    return det, e.batch_add(SCENE, 1, det)


def null_det():
    d = abi.sa_detections()
    d.n = 2
    return d


def test_slot_out_of_range(eng):
    det, _ = staged(eng)
    eng.batch_run()
    lib, h = eng.lib, eng.h
    ids, votes, cols = np.full(2, 77, np.uint64), np.full(2, 77, np.uint8), np.full(2, 77, np.int32)
    nid, pred = np.full(2, 77, np.uint64), np.full(2, 77, abi.BOX_DTYPE)
    pi, pv, pc = u64p(), u8p(), i32p()
    n, t, k = C.c_uint32(77), C.c_uint32(77), C.c_uint32(77)
    calls = {
        "sa_batch_fill": lambda: lib.sa_batch_fill(h, 5),
        "sa_batch_fetch": lambda: lib.sa_batch_fetch(h, 5, ids.ctypes.data_as(u64p), votes.ctypes.data_as(u8p)),
        "sa_batch_fetch_cols": lambda: lib.sa_batch_fetch_cols(h, 5, cols.ctypes.data_as(i32p)),
        "sa_batch_results": lambda: lib.sa_batch_results(h, 5, C.byref(pi), C.byref(pv), C.byref(pc)),
        "sa_tracks_apply_begin": lambda: lib.sa_tracks_apply_begin(h, 5, nid.ctypes.data_as(u64p)),
        "sa_tracks_apply_end": lambda: lib.sa_tracks_apply_end(h, 5, C.cast(pred.ctypes.data, boxp)),
        "sa_tracks_apply_collect": lambda: lib.sa_tracks_apply_collect(h, 5, nid.ctypes.data_as(u64p), C.cast(pred.ctypes.data, boxp)),
        "sa_tracks_apply_collect_table": lambda: lib.sa_tracks_apply_collect_table(h, 5, nid.ctypes.data_as(u64p)),
        "sa_tracks_apply_collect_slot": lambda: lib.sa_tracks_apply_collect_slot(h, 5, nid.ctypes.data_as(u64p), C.cast(pred.ctypes.data, boxp)),
        "sa_tap_dims": lambda: lib.sa_tap_dims(h, 5, C.byref(n), C.byref(t), C.byref(k)),
    }
    for name, call in calls.items():
        assert call() == BAD, name
        assert err(eng) == OUT_OF_RANGE, name
    assert (ids == 77).all() and (votes == 77).all() and (cols == 77).all() and (nid == 77).all()
    assert (pred.view(np.uint8) == np.full(2, 77, abi.BOX_DTYPE).view(np.uint8)).all()
    assert not pi and not pv and not pc
    assert (n.value, t.value, k.value) == (77, 77, 77)
    # the set itself is intact
    eng.batch_sync()
    got, _ = eng.batch_fetch(0, 2)
    np.testing.assert_array_equal(got, [1, 2])


def test_before_the_run(eng):
    staged(eng)
    lib, h = eng.lib, eng.h
    ids, votes, cols, nid = np.full(2, 77, np.uint64), np.full(2, 77, np.uint8), np.full(2, 77, np.int32), np.full(2, 77, np.uint64)
    pred = np.full(2, 77, abi.BOX_DTYPE)
    pi, pv, pc = u64p(), u8p(), i32p()
    refused(eng, lib.sa_batch_fetch(h, 0, ids.ctypes.data_as(u64p), votes.ctypes.data_as(u8p)), STATE, "sa_batch_fetch before sa_batch_run")
    refused(eng, lib.sa_batch_fetch_cols(h, 0, cols.ctypes.data_as(i32p)), STATE, "sa_batch_fetch_cols before sa_batch_run")
    refused(eng, lib.sa_batch_results(h, 0, C.byref(pi), C.byref(pv), C.byref(pc)), STATE, "sa_batch_results before sa_batch_run")
    refused(eng, lib.sa_tracks_apply(h, 0, nid.ctypes.data_as(u64p), C.cast(pred.ctypes.data, boxp)), STATE, "sa_tracks_apply before sa_batch_run")
    assert (ids == 77).all() and (votes == 77).all() and (cols == 77).all() and not pi and not pv and not pc
    assert (pred.view(np.uint8) == np.full(2, 77, abi.BOX_DTYPE).view(np.uint8)).all()
    assert eng.count(SCENE) == 3


def test_collect_without_the_fused_run(eng):
    staged(eng)
    eng.batch_run()
    lib, h = eng.lib, eng.h
    nid, pred = np.full(2, 77, np.uint64), np.full(2, 77, abi.BOX_DTYPE)
    np_, pp = nid.ctypes.data_as(u64p), C.cast(pred.ctypes.data, boxp)
    refused(eng, lib.sa_tracks_apply_collect(h, 0, np_, pp), STATE, "sa_tracks_apply_collect without sa_batch_run_apply (or collected already)")
    refused(eng, lib.sa_tracks_apply_collect_table(h, 0, np_), STATE, "sa_tracks_apply_collect_table without sa_batch_run_apply (or collected already)")
    refused(eng, lib.sa_tracks_apply_collect_slot(h, 0, np_, pp), STATE, "sa_tracks_apply_collect_slot without sa_batch_run_apply (or collected already)")
    assert (nid == 77).all() and (pred.view(np.uint8) == np.full(2, 77, abi.BOX_DTYPE).view(np.uint8)).all()
    eng.batch_sync()


def test_adds_null_arguments(eng):
    lib, h = eng.lib, eng.h
    eng.batch_begin()
    det = abi.make_detections(frame())
    rows = framerows.sa_dev_rows()
    slot = C.c_uint32(77)
    sl = C.byref(slot)
    refused(eng, lib.sa_batch_add(h, SCENE, 1, None, sl), BAD, "sa_batch_add: null argument")
    refused(eng, lib.sa_batch_add_rows(h, SCENE, 1, None, None, sl), BAD, "sa_batch_add: null argument")      # (answers as sa_batch_add)
    refused(eng, lib.sa_batch_add_deferred(h, SCENE, 1, None, None, sl), BAD, "sa_batch_add_deferred: null argument")
    refused(eng, lib.sa_batch_add_dev(h, SCENE, 1, None, C.byref(rows), sl), BAD, "sa_batch_add_dev: null argument")
    refused(eng, lib.sa_batch_add_deferred_dev(h, SCENE, 1, None, C.byref(rows), sl), BAD, "sa_batch_add_deferred_dev: null argument")
    refused(eng, lib.sa_batch_add_dev(h, SCENE, 1, C.byref(det), None, sl), BAD, "sa_batch_add_dev: null rows")
    refused(eng, lib.sa_batch_add_deferred_dev(h, SCENE, 1, C.byref(det), None, sl), BAD, "sa_batch_add_deferred_dev: null rows")
    # (a null detections struct is named before null rows)
    refused(eng, lib.sa_batch_add_dev(h, SCENE, 1, None, None, sl), BAD, "sa_batch_add_dev: null argument")
    nb = null_det()
    for name, call in {
        "sa_batch_add": lambda: lib.sa_batch_add(h, SCENE, 1, C.byref(nb), sl),
        "sa_batch_add_rows": lambda: lib.sa_batch_add_rows(h, SCENE, 1, C.byref(nb), None, sl),
        "sa_batch_add_deferred": lambda: lib.sa_batch_add_deferred(h, SCENE, 1, C.byref(nb), None, sl),
        "sa_batch_add_dev": lambda: lib.sa_batch_add_dev(h, SCENE, 1, C.byref(nb), C.byref(rows), sl),
        "sa_batch_add_deferred_dev": lambda: lib.sa_batch_add_deferred_dev(h, SCENE, 1, C.byref(nb), C.byref(rows), sl),
    }.items():
        eng.lib.sa_tap_dims(h, 5, None, None, None)      # (another text in the slot first)
        assert call() == BAD, name
        assert err(eng) == NULL_BOXES, name
    assert slot.value == 77
    # nothing was staged by any of them
    assert eng.batch_add(SCENE, 1, det) == 0


def test_associate_pairs_null_arguments(eng):
    lib, h = eng.lib, eng.h
    det = abi.make_detections(frame())
    rows = framerows.sa_dev_rows()
    ids, votes = np.full(2, 77, np.uint64), np.full(2, 77, np.uint8)
    ip, vp = ids.ctypes.data_as(u64p), votes.ctypes.data_as(u8p)
    refused(eng, lib.sa_associate(h, SCENE, 1, None, ip, vp), BAD, "sa_associate: null argument")
    refused(eng, lib.sa_associate_dev(h, SCENE, 1, None, C.byref(rows), ip, vp), BAD, "sa_associate_dev: null argument")
    refused(eng, lib.sa_associate_dev(h, SCENE, 1, C.byref(det), None, ip, vp), BAD, "sa_associate_dev: null rows")
    req, res, _ = Engine.make_requests([(SCENE, 1, det)])
    refused(eng, lib.sa_associate_batch(h, 1, None, res), BAD, "sa_associate_batch: null argument")
    refused(eng, lib.sa_associate_batch(h, 1, req, None), BAD, "sa_associate_batch: null argument")
    refused(eng, lib.sa_associate_batch_dev(h, 1, None, None, res), BAD, "sa_associate_batch_dev: null argument")
    refused(eng, lib.sa_associate_batch_dev(h, 1, req, None, None), BAD, "sa_associate_batch_dev: null argument")
    # null boxes, through every one of the four
    nb = null_det()
    nreq, nres, _ = Engine.make_requests([(SCENE, 1, nb)])
    nres[0].out_track_id, nres[0].out_voting_type = ip, vp
    rp = (framerows.ROWS_P * 1)(C.pointer(rows))
    refused(eng, lib.sa_associate(h, SCENE, 1, C.byref(nb), ip, vp), BAD, NULL_BOXES)
    lib.sa_tap_dims(h, 5, None, None, None)
    refused(eng, lib.sa_associate_dev(h, SCENE, 1, C.byref(nb), C.byref(rows), ip, vp), BAD, NULL_BOXES)
    lib.sa_tap_dims(h, 5, None, None, None)
    refused(eng, lib.sa_associate_batch(h, 1, nreq, nres), BAD, NULL_BOXES)
    lib.sa_tap_dims(h, 5, None, None, None)
    refused(eng, lib.sa_associate_batch_dev(h, 1, nreq, rp, nres), BAD, NULL_BOXES)
    lib.sa_tap_dims(h, 5, None, None, None)
    refused(eng, lib.sa_associate_batch_dev(h, 1, nreq, None, nres), BAD, NULL_BOXES)       # (no descriptor: the scene as sa_batch_add takes it)
    assert (ids == 77).all() and (votes == 77).all()


def test_null_engine(eng):
    """A null engine: some entries write the calling thread's creation-error slot, the *_dev ones answer without a text."""
    lib = eng.lib
    det = abi.make_detections(frame())
    rows = framerows.sa_dev_rows()
    slot = C.c_uint32(77)
    ids, votes = np.full(2, 77, np.uint64), np.full(2, 77, np.uint8)
    ip, vp = ids.ctypes.data_as(u64p), votes.ctypes.data_as(u8p)
    req, res, _ = Engine.make_requests([(SCENE, 1, det)])
    rp = (framerows.ROWS_P * 1)(C.pointer(rows))
    loud = {
        "sa_batch_add: null argument": [lambda: lib.sa_batch_add(None, SCENE, 1, C.byref(det), C.byref(slot)),
                                        lambda: lib.sa_batch_add_rows(None, SCENE, 1, C.byref(det), None, C.byref(slot))],
        "sa_batch_add_deferred: null argument": [lambda: lib.sa_batch_add_deferred(None, SCENE, 1, C.byref(det), None, C.byref(slot))],
        "sa_associate: null argument": [lambda: lib.sa_associate(None, SCENE, 1, C.byref(det), ip, vp)],
        "sa_associate_batch: null argument": [lambda: lib.sa_associate_batch(None, 1, req, res)],
    }
    for text, calls in loud.items():
        for call in calls:
            lib.sa_engine_create(None, None)      # (another text in the slot first)
            assert lib.sa_last_error(None) == b"sa_engine_create: null argument"
            assert call() == BAD, text
            assert lib.sa_last_error(None).decode() == text
    lib.sa_engine_create(None, None)
    silent = [lambda: lib.sa_batch_add_dev(None, SCENE, 1, C.byref(det), C.byref(rows), C.byref(slot)),
              lambda: lib.sa_batch_add_deferred_dev(None, SCENE, 1, C.byref(det), C.byref(rows), C.byref(slot)),
              lambda: lib.sa_associate_dev(None, SCENE, 1, C.byref(det), C.byref(rows), ip, vp),
              lambda: lib.sa_associate_batch_dev(None, 1, req, rp, res),
              lambda: lib.sa_batch_fill(None, 0),
              lambda: lib.sa_batch_fetch(None, 0, ip, vp)]
    for k, call in enumerate(silent):
        assert call() == BAD, k
        assert lib.sa_last_error(None) == b"sa_engine_create: null argument", k
    assert slot.value == 77 and (ids == 77).all() and (votes == 77).all()


def test_scene_twice_in_one_set(eng):
    det, sl0 = staged(eng)
    slot = C.c_uint32(77)
    for call in (lambda: eng.lib.sa_batch_add(eng.h, SCENE, 1, C.byref(det), C.byref(slot)),
                 lambda: eng.lib.sa_batch_add_rows(eng.h, SCENE, 1, C.byref(det), None, C.byref(slot)),
                 lambda: eng.lib.sa_batch_add_deferred(eng.h, SCENE, 1, C.byref(det), None, C.byref(slot))):
        eng.lib.sa_tap_dims(eng.h, 5, None, None, None)
        refused(eng, call(), STATE, "scene 7 is already part of this batch")
    assert slot.value == 77 and sl0 == 0
    # ... and the set still holds the one scene: the next slot number is 1
    assert eng.batch_add(SCENE + 1, 1, det) == 1


@pytest.mark.parametrize("field,value,text", [("aspect", 0.0, BAD_ASPECT), ("aspect", float("nan"), BAD_ASPECT), ("height", -1.0, BAD_ASPECT),
                                              ("confidence", 1.5, BAD_CONFIDENCE), ("confidence", float("nan"), BAD_CONFIDENCE)])
def test_bad_box_at_index_1(eng, field, value, text):
    lib, h = eng.lib, eng.h
    det = abi.make_detections(frame(**{field: value}))
    rows = framerows.sa_dev_rows()
    slot = C.c_uint32(77)
    eng.batch_begin()
    # immediate adds: refused at the add, nothing staged
    for name, call in {"sa_batch_add": lambda: lib.sa_batch_add(h, SCENE, 1, C.byref(det), C.byref(slot)),
                       "sa_batch_add_rows": lambda: lib.sa_batch_add_rows(h, SCENE, 1, C.byref(det), None, C.byref(slot)),
                       "sa_batch_add_dev": lambda: lib.sa_batch_add_dev(h, SCENE, 1, C.byref(det), C.byref(rows), C.byref(slot))}.items():
        lib.sa_tap_dims(h, 5, None, None, None)
        assert call() == BAD, name
        assert err(eng) == text, name
    assert slot.value == 77
    # a deferred add leaves the boxes to the fill
    eng._chk(lib.sa_batch_add_deferred(h, SCENE, 1, C.byref(det), None, C.byref(slot)))
    assert slot.value == 0
    refused(eng, lib.sa_batch_fill(h, 0), BAD, text)
    # through the one-call forms
    ids, votes = np.full(2, 77, np.uint64), np.full(2, 77, np.uint8)
    refused(eng, lib.sa_associate(h, SCENE, 1, C.byref(det), ids.ctypes.data_as(u64p), votes.ctypes.data_as(u8p)), BAD, text)
    assert (ids == 77).all() and (votes == 77).all()


def test_apply_begin_refuses_bad_new_ids(eng):
    """Both boxes lie away from every track: both start tracks, and sa_tracks_apply_begin checks their ids."""
    lib, h = eng.lib, eng.h
    staged(eng, frame(far=True))
    eng.batch_run()
    eng.batch_sync()
    ids, _ = eng.batch_fetch(0, 2)
    np.testing.assert_array_equal(ids, [0, 0])

    def begin(new):
        a = np.array(new, np.uint64)
        return lib.sa_tracks_apply_begin(h, 0, a.ctypes.data_as(u64p))
    refused(eng, lib.sa_tracks_apply_begin(h, 0, None), BAD, "candidate 0 starts a track and needs new_ids[0] > 0")
    refused(eng, begin([50, 0]), BAD, "candidate 1 starts a track and needs new_ids[1] > 0")
    refused(eng, begin([50, 2]), BAD, "new id 2 already exists in the scene")
    refused(eng, begin([50, 50]), BAD, "new id 50 given twice")
    assert eng.count(SCENE) == 3
    np.testing.assert_array_equal(eng.order(SCENE), [1, 2, 3])
    # the slot is still good for the step itself
    pred = np.zeros(2, abi.BOX_DTYPE)
    new = np.array([50, 51], np.uint64)
    eng._chk(lib.sa_tracks_apply(h, 0, new.ctypes.data_as(u64p), C.cast(pred.ctypes.data, boxp)))
    np.testing.assert_array_equal(eng.order(SCENE), [1, 2, 3, 50, 51])
    eng.remove(SCENE, [50, 51])
