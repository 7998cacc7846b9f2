"""The keypoint tracker on the MI355X (KeypointSort over include/similari_pose_sort.h) against tests/pose_sort_ref.py, the numpy model,
and against a twin PoseTrackBank whose life cycle Python keeps.  Equal means equal: ids, the bank's order, every state and the wasted
states bit for bit (two NaNs count as the same bits).  The gate is tested cell by cell through peek's tap; the gated vote on scenes
that tests/test_pose_sort_scenes_ref.py proves unique on the CPU, so no row is left out.

Shapes: the scenes (m, T) = (1, 1), (3, 5), (0, 4), (17, 70), (4, 0), (70, 17) of tests/test_gpu_pose_batch.py in one call (a scene
without poses, one without tracks, several tiles), P in {1, 17, 65} (65 crosses the 64-point LDS chunk), tracks idle 1, 2 and 4 epochs;
150 x 150 for the dense search; 2048 tracks in a scene for the limit."""
import ctypes as C

import numpy as np
import pytest

import devrows_ref as dref
import pose_ref as PR
import pose_sort_ref as SR
from similari_amd import abi
from similari_amd.devrows import DeviceRows
from similari_amd.engine import Engine, EngineError
from similari_amd.f16 import SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_F32
from similari_amd.points import SA_ROW_NONE
from similari_amd.pose_sort import KeypointSort
from similari_amd.pose_track import PoseTrackBank
from test_gpu_points import bits, device_block, to_source

pytestmark = pytest.mark.gpu
f32, u8, u32, u64 = np.float32, np.uint8, np.uint32, np.uint64
SHAPES = [(1, 1), (3, 5), (0, 4), (17, 70), (4, 0), (70, 17)]
SEVEN = SHAPES + [(17, 65)]


@pytest.fixture(scope="module")
def eng():
    e = Engine(abi.make_config(positional="iou", positional_threshold=0.3, device=0))
    yield e
    e.close()


def call_of(frame):
    return {s: (z, p) for s, z, p in frame}


def same_as_model(trk, mdl):
    bank = trk.bank()
    assert bank.order().tolist() == mdl.order
    for t in mdl.order:
        has, mean, cov = bank.state(t)
        mh, mm, mc = mdl.state[t]
        assert (has == mh).all() and bits(mean[has], mm[mh]) and bits(cov[has], mc[mh]), t
        assert np.isnan(mean[~has]).all() and np.isnan(cov[~has]).all()
    for s, e in mdl.epochs.items():
        assert trk.epoch(s) == e and trk.active(s) == len(mdl.lists[s])
    assert trk.active() == len(mdl.order)


def records_equal(got, frame, want):
    for f, recs in zip(frame, want):
        g = got[f[0]]
        assert [(int(r["id"]), int(r["scene"]), int(r["epoch"]), int(r["length"]), int(r["created"])) for r in g] == [tuple(r) for r in recs], f[0]
        assert np.isnan(g["weight"][g["created"] == 1]).all() and not np.isnan(g["weight"][g["created"] == 0]).any()


def wasted_equal(trk, mdl):
    got, want = trk.wasted(), mdl.wasted
    mdl.wasted = []
    assert [(w.id, w.scene, w.first_epoch, w.last_epoch, w.length) for w in got] == [(w["id"], w["scene"], w["first"], w["last"], w["length"]) for w in want]
    for a, b in zip(got, want):
        h = b["state"][0]
        assert (a.has == h).all() and bits(a.mean[h], b["state"][1][h]) and bits(a.cov[h], b["state"][2][h])
        assert np.isnan(a.mean[~h]).all() and np.isnan(a.cov[~h]).all()
    return len(got)


# ---- 1. the gate, cell by cell ---------------------------------------------------------------------------
@pytest.mark.parametrize("min_common", [1, 3])
@pytest.mark.parametrize("cons", [[], [(1, 1.0)], [(1, 0.5), (3, 2.0)]], ids=["none", "one", "two"])
@pytest.mark.parametrize("P", [1, 17, 65])
def test_peeks_tap_carries_the_models_bits(eng, P, cons, min_common):
    frames, centres = SR.warmup(7, SHAPES, P)
    shown = SR.shown_frame(7, SHAPES, P, centres)
    mdl = SR.RefSort(P, SR.WARM, cons, min_common=min_common)
    with KeypointSort(eng, P, max_idle_epochs=SR.WARM, constraints=cons, min_common=min_common) as trk:
        for fr in frames:
            records_equal(trk.predict(call_of(fr)), fr, mdl.predict(fr))
        same_as_model(trk, mdl)
        order, epochs = trk.bank().order().tolist(), [trk.epoch(s) for s in range(1, 7)]
        pl = mdl.plan([f[0] for f in shown])
        if P > 1 and min_common == 1:
            assert [len(t) for t in pl["tracks"]] == [T for _, T in SHAPES]
        assert len({float(x) for ls in pl["limits"] for x in ls}) == (len(cons) + 1 if cons else 1)   # idle 1, 2 and 4 epochs: every limit
        got = trk.peek(call_of(shown), matrix=True)
        st = trk.last()
        refused = 0
        for k, f in enumerate(SR.present_of(shown)):
            w, no, raw = mdl.weights(pl, k, f[1], f[2])
            assert got[f[0]][2].shape == w.shape and bits(got[f[0]][2], w), k
            refused += int(no.sum())
            hit = got[f[0]][0] != 0
            assert all(int(t) in pl["tracks"][k] for t in got[f[0]][0][hit]) and not np.isnan(got[f[0]][1][hit]).any()
        assert (st["gate_launches"], st["vote_launches"], st["refused_pairs"]) == (1 if cons else 0, 3, refused)
        assert bool(refused) == bool(cons)
        # the same frame where a network would leave it: rows in device memory, gathered, two poses without a row
        m = sum(len(f[1]) for f in shown)
        z = np.concatenate([f[1] for f in shown])
        mask = np.concatenate([f[2] for f in shown])
        index = np.random.default_rng(3).permutation(m + 9)[:m].astype(u32)
        index[[5, 40]] = SA_ROW_NONE
        block = np.zeros((m + 9, P * 2 + 3), f32)
        block[index[index != SA_ROW_NONE], : P * 2] = z[index != SA_ROW_NONE].reshape(-1, P * 2)
        with device_block(eng, block) as ptr:
            dev = trk.peek([f[0] for f in shown], rows=DeviceRows(ptr, m + 9, P * 2 + 3, SA_ELEM_F32, index), pose_counts=[len(f[1]) for f in shown],
                           present=mask, matrix=True)
        mask = mask & (index != SA_ROW_NONE)[:, None]
        ends = np.cumsum([len(f[1]) for f in shown])[:-1]
        for k, (f, ms) in enumerate(zip(shown, np.split(mask, ends))):
            w = mdl.weights(pl, k, f[1], ms & np.isfinite(f[1]).all(-1))[0]
            assert bits(dev[f[0]][2], w), k
        # a peek changes nothing
        assert trk.bank().order().tolist() == order and [trk.epoch(s) for s in range(1, 7)] == epochs and trk.wasted() == []
        same_as_model(trk, mdl)


# ---- 2. the gated vote ----------------------------------------------------------------------------------
def test_the_gated_vote_equals_the_models_in_every_row(eng):
    g = SR.gated_scenes(17)   # (proven on the CPU: every row is forced, a pair inside the gate is refused in every scene)
    mdl = SR.RefSort(17, SR.WARM, SR.GATED_CONS)
    with KeypointSort(eng, 17, max_idle_epochs=SR.WARM, constraints=SR.GATED_CONS) as trk:
        for fr in g["frames"]:
            records_equal(trk.predict(call_of(fr)), fr, mdl.predict(fr))
        got = trk.peek(call_of(g["frame"]))
        for k, f in enumerate(g["frame"]):
            tracks = np.array(g["plan"]["tracks"][k] + [0], u64)
            assert (got[f[0]][0] == tracks[g["votes"][k][0]]).all(), k    # (-1 reads the 0 at the end)
            assert (got[f[0]][0] != tracks[g["votes"][k][1]]).any(), k    # and not the ungated vote
        records_equal(trk.predict(call_of(g["frame"])), g["frame"], mdl.predict(g["frame"]))
        assert trk.last()["gate_launches"] == 1
        same_as_model(trk, mdl)


def test_a_crowd_of_150_under_a_limit(eng):
    c = SR.crowd()   # (on the CPU first: the greedy start leaves roots, the limit refuses pairs)
    assert PR.greedy_roots(c["wq"], c["thr_q"]) >= 1 and c["refused"].any()
    mdl = SR.RefSort(2, SR.WARM, [(1, 1.0)])
    with KeypointSort(eng, 2, max_idle_epochs=SR.WARM, constraints=[(1, 1.0)]) as trk:
        records_equal(trk.predict(call_of(c["frames"][0])), c["frames"][0], mdl.predict(c["frames"][0]))
        ids, w, tap = trk.peek(call_of(c["frame"]), matrix=True)[1]
        st = trk.last()
        assert bits(tap, c["w"]) and st["roots"] >= 1 and st["gate_launches"] == 1
        tracks = c["plan"]["tracks"][0]
        match = np.array([tracks.index(int(t)) if t else -1 for t in ids])
        hit = match >= 0
        assert not c["refused"][np.flatnonzero(hit), match[hit]].any()             # no refused pair is matched
        assert len(set(match[hit])) == int(hit.sum())
        assert PR.total_of(match, c["wq"], c["thr_q"]) == c["total"]               # an optimum of the gated matrix
        assert bits(w[hit], c["w"][np.flatnonzero(hit), match[hit]])


# ---- 3. eight frames: a twin without constraints, the model with them -------------------------------------
def eight_frames(P, seed=80):
    """Seven cameras: frame 0 shows the first T people of each, every later frame m of its max(m, T) + 3 — births, misses, and
    people who stay away long enough to expire at max_idle_epochs = 2; camera 4 is not named in frame 4, camera 2 shows nobody."""
    rng = np.random.default_rng(seed + P)
    people = [PR.people(rng, max(m, T) + 3, P, False) + 400.0 * s for s, (m, T) in enumerate(SEVEN)]
    frames = []
    for k in range(8):
        fr = []
        for s, (m, T) in enumerate(SEVEN):
            if k == 4 and s == 3:
                continue
            shown = np.arange(T) if k == 0 else rng.permutation(len(people[s]))[:m]
            z = (people[s][shown] + rng.normal(0, 0.04, (len(shown), P, 2))).astype(f32)
            fr.append((s + 1, z, rng.random((len(shown), P)) >= 0.25))
        frames.append(fr)
    return frames


@pytest.mark.parametrize("P", [1, 17, 65])
def test_without_constraints_the_call_leaves_the_twins_bits(eng, P):
    """The twin is the only route there was: PoseTrackBank.track_batch, with the life cycle and the id lists kept in Python."""
    mdl = SR.RefSort(P, 2)
    expired = created = 0
    with KeypointSort(eng, P, max_idle_epochs=2) as trk, PoseTrackBank(eng, P) as twin:
        for k, fr in enumerate(eight_frames(P)):
            scenes = [f[0] for f in fr]
            pl = mdl.plan(scenes)
            final = {t: twin.state(t) for t in pl["expired"]}
            if pl["expired"]:
                twin.remove(pl["expired"])
            ids = twin.track_batch([(np.array(t, u64), f[1], f[2]) for t, f in zip(pl["tracks"], fr)], mdl.next_id)
            cols = [[t.index(int(i)) if int(i) in t else -1 for i in got] for t, got in zip(pl["tracks"], ids)]
            want = mdl.apply(scenes, pl, cols)[0]
            got = trk.predict(call_of(fr))
            st = trk.last()
            records_equal(got, fr, want)
            assert bits(np.concatenate([got[s]["weight"] for s in scenes]), twin.last_weights()), k
            bank = trk.bank()
            assert bank.order().tolist() == twin.order().tolist() == mdl.order, k
            for t in mdl.order:
                x, y = bank.state(t), twin.state(t)
                assert (x[0] == y[0]).all() and bits(x[1], y[1]) and bits(x[2], y[2]), (k, t)
            ws = trk.wasted()
            assert [w.id for w in ws] == pl["expired"], k
            for w in ws:
                y = final[w.id]
                assert (w.has == y[0]).all() and bits(w.mean, y[1]) and bits(w.cov, y[2]), (k, w.id)
            mdl.wasted = []
            tw = twin.last_track()
            assert (st["vote_launches"], st["gate_launches"], st["step_launches"]) == (3 if k else 0, 0, 2 if k else 1), k
            assert (st["matched"], st["created"], st["coasted"], st["roots"]) == (tw["matched"], tw["created"], tw["coasted"], tw["roots"])
            assert st["expired"] == len(pl["expired"])
            assert st["bytes_d2h"] == (8 * st["poses"] + 4 * len(fr) if k else 0) + 81 * P * st["expired"], k
            expired += st["expired"]
            created += st["created"] if k else 0
        assert expired >= 10 and created >= 10


@pytest.mark.parametrize("P", [17, 65])
def test_with_constraints_the_call_leaves_the_models_bits(eng, P):
    cons = [(1, 1.0), (2, 2.0)]
    mdl = SR.RefSort(P, 2, cons)
    expired = 0
    with KeypointSort(eng, P, max_idle_epochs=2, constraints=cons) as trk:
        for k, fr in enumerate(eight_frames(P)):
            records_equal(trk.predict(call_of(fr)), fr, mdl.predict(SR.present_of(fr)))
            assert trk.last()["gate_launches"] == (1 if k else 0) and trk.last()["vote_launches"] == (3 if k else 0), k
            same_as_model(trk, mdl)
            expired += wasted_equal(trk, mdl)
        assert expired >= 10


# ---- 4. expiry -------------------------------------------------------------------------------------------
def test_expiry(eng):
    P = 17
    rng = np.random.default_rng(9)
    people = PR.people(rng, 70, P, False)
    every = np.ones((70, P), bool)
    show = lambda who: ((people[who] + rng.normal(0, 0.03, (len(who), P, 2))).astype(f32), every[: len(who)])
    mdl = SR.RefSort(P, 2)
    with KeypointSort(eng, P, max_idle_epochs=2) as trk:
        def both(fr):
            records_equal(trk.predict(call_of(fr)), fr, mdl.predict(fr))
            same_as_model(trk, mdl)

        both([(1,) + show(np.arange(60)), (2,) + show(np.arange(60, 64))])
        trk.bank().distance(mdl.order[:1], people[:1].astype(f32))   # (changes no state; its record shows the capacity)
        assert trk.bank().last()["capacity"] == 64
        both([(1,) + show(np.arange(30))])                       # scene 2 is not named: its epoch and its tracks stay
        trk.bank().distance(mdl.order[:1], people[:1].astype(f32))
        assert trk.bank().last()["capacity"] == 128              # 64 -> 128 inside the call: it reserves room for T + m tracks
        assert trk.epoch(2) == 1 and trk.active(2) == 4 and trk.epoch(1) == 2
        both([(1,) + show(np.arange(30))])
        before = {t: trk.bank().state(t) for t in mdl.lists[1][30:]}
        both([(1,) + show(np.arange(30, 70))])                   # epoch 4: tracks 31 .. 60 expire and 40 poses create 40 tracks in one call
        st = trk.last()
        assert (st["expired"], st["created"], st["matched"]) == (30, 40, 0) and len(trk.bank()) == 74
        ws = trk.wasted()
        assert [w.id for w in ws] == list(before) and all((w.first_epoch, w.last_epoch, w.length) == (1, 1, 1) for w in ws)
        for w in ws:                                              # the final states: get_state of the frame before
            y = before[w.id]
            assert (w.has == y[0]).all() and bits(w.mean, y[1]) and bits(w.cov, y[2])
        mdl.wasted = []
        both([(2, np.zeros((0, P, 2), f32), np.zeros((0, P), bool))])   # a scene named with zero poses: epoch 2, its tracks coast
        assert trk.epoch(2) == 2 and trk.last()["coasted"] == 4 and trk.last()["expired"] == 0
        trk.skip_epochs(2, 3)
        mdl.skip_epochs(2, 3)
        assert trk.epoch(2) == 5 and trk.active(2) == 4           # nothing expires before a predict names the scene
        both([(2, np.zeros((0, P, 2), f32), np.zeros((0, P), bool))])   # epoch 6: 6 - 1 > 2; neither a pose nor a track is left
        assert trk.last()["expired"] == 4 and trk.active(2) == 0 and wasted_equal(trk, mdl) == 4
        both([(3,) + show(np.arange(3)), (1,) + show(np.arange(30))])   # the next frame works
        assert wasted_equal(trk, mdl) == 0


# ---- 5. poses in device memory ---------------------------------------------------------------------------
@pytest.mark.parametrize("comps", [2, 3])
@pytest.mark.parametrize("elem", [SA_ELEM_F32, SA_ELEM_F16, SA_ELEM_BF16])
def test_poses_read_from_device_memory(eng, elem, comps):
    P, cons = 17, [(1, 1.0)]
    frames = eight_frames(P, seed=90)[:3]
    eb = 4 if elem == SA_ELEM_F32 else 2
    L, off = P * comps, 4
    W = L + 11   # a column slice of a wider output
    rng = np.random.default_rng(70 + elem)
    with KeypointSort(eng, P, max_idle_epochs=2, constraints=cons) as dev, KeypointSort(eng, P, max_idle_epochs=2, constraints=cons) as host:
        for k, fr in enumerate(frames):
            z, pres = np.concatenate([f[1] for f in fr]), np.concatenate([f[2] for f in fr])
            counts = [len(f[1]) for f in fr]
            m, B = len(z), len(z) + 7
            index = rng.permutation(B)[:m].astype(u32)
            index[[3, 50]] = SA_ROW_NONE
            got = index != SA_ROW_NONE
            vals = rng.uniform(-300, 300, (B, W)).astype(f32)
            block = np.zeros((B, P, comps), f32)
            block[index[got], :, :2] = z[got] / f32(4) if elem != SA_ELEM_F32 else z[got]   # (half precision keeps people apart only near 0)
            if comps == 3:
                block[..., 2] = rng.uniform(0, 1, (B, P))
            vals[:, off: off + L] = block.reshape(B, L)
            src = to_source(vals, elem)
            wide = dref.widen(src, elem)[:, off: off + L].reshape(B, P, comps)
            zh = np.zeros((m, P, comps), f32)
            zh[got] = wide[index[got]]
            mask = pres & got[:, None]
            ends = np.cumsum(counts)[:-1]
            with device_block(eng, src) as ptr:
                a = dev.predict([f[0] for f in fr], rows=DeviceRows(ptr + off * eb, B, W, elem, index), pose_counts=counts, present=pres, comps=comps,
                                min_score=0.4, xy=True)
            st = dev.last()
            b = host.predict({f[0]: (x, y) for f, x, y in zip(fr, np.split(zh, ends), np.split(mask, ends))}, min_score=0.4, xy=True)
            for f in fr:
                x, y = a[f[0]][0], b[f[0]][0]
                assert all((x[n] == y[n]).all() for n in ("id", "scene", "epoch", "length", "created")) and bits(x["weight"], y["weight"]), (k, f[0])
                assert bits(a[f[0]][1], b[f[0]][1]), (k, f[0])
            assert dev.bank().order().tolist() == host.bank().order().tolist()
            for t in dev.bank().order():
                x, y = dev.bank().state(t), host.bank().state(t)
                assert (x[0] == y[0]).all() and bits(x[1], y[1]) and bits(x[2], y[2]), (k, t)
            n = st["tracks"]
            gated = st["gate_launches"]
            assert gated == (1 if k else 0)
            assert st["bytes_h2d"] == 32 * len(fr) + 4 * n + 4 * n * gated + m * 4 + m * P   # no pose bytes
            assert st["src_bytes"] == int(got.sum()) * L * eb
            assert st["matched"] + st["created"] == m
        assert st["matched"] >= 10 or elem != SA_ELEM_F32   # (half precision blurs people this far from the origin; both trackers see the same blur)


# ---- 6. the limit and the refusals -----------------------------------------------------------------------
def test_2048_tracks_pass_and_2049_are_refused(eng):
    P = 2
    rng = np.random.default_rng(2048)
    people = PR.people(rng, 2049, P, False).astype(f32)
    with KeypointSort(eng, P, max_idle_epochs=9, constraints=[(1, 1.0)]) as trk:
        for lo in (0, 1024):
            trk.predict({7: people[lo: lo + 1024]})   # nobody near anybody: 1024 births a frame
        assert trk.active(7) == 2048
        got = trk.predict({7: people[:2048: 8]})
        assert (got[7]["created"] == 0).all() and trk.last()["gate_launches"] == 1
        trk.predict({7: people[2048:]})                # the 2049th track
        order, epoch = trk.bank().order().tolist(), trk.epoch(7)
        with pytest.raises(EngineError) as ei:
            trk.predict({8: people[:2], 7: people[:3]})
        assert ei.value.code == abi.SA_ERR_UNSUPPORTED and "scene 7 has 2049 tracks" in str(ei.value)
        assert trk.bank().order().tolist() == order and trk.epoch(7) == epoch and trk.epoch(8) == 0 and trk.last()["poses"] == 0
        got = trk.predict({8: people[:2]})             # the next good call works
        assert got[8]["id"].tolist() == [2050, 2051]


def test_every_refusal_leaves_everything_as_it_was(eng):
    P = 17
    frames = eight_frames(P, seed=95)
    lib = eng.lib
    for kw, word in ((dict(constraints=[(1, 0.0)]), "max_dist"), (dict(constraints=[(k, 1.0) for k in range(9)]), "at most 8"),
                     (dict(min_common=0), "min_common"), (dict(threshold=float("nan")), "threshold")):
        with pytest.raises(EngineError) as ei:
            KeypointSort(eng, P, **kw)
        assert ei.value.code == abi.SA_ERR_BAD_ARG and word in str(ei.value)
    with KeypointSort(eng, P, max_idle_epochs=1, constraints=[(1, 1.0)]) as trk:
        for fr in frames[:3]:
            trk.predict(call_of(fr))
        trk.predict(call_of(frames[3][:2]))   # (tracks of the other scenes are now one frame from expiry: a refused call must not expire them)
        left = trk.wasted()
        bank = trk.bank()
        order = bank.order().tolist()
        before = [bank.state(t) for t in order]
        epochs, active = [trk.epoch(s) for s in range(1, 9)], [trk.active(s) for s in range(1, 9)]
        fr = frames[4]
        z, pres = np.concatenate([f[1] for f in fr]), np.concatenate([f[2] for f in fr])
        B, U = abi.SA_ERR_BAD_ARG, abi.SA_ERR_UNSUPPORTED
        ids = np.array([f[0] for f in fr], u64)
        pc = np.array([len(f[1]) for f in fr], u32)
        twice = ids.copy()
        twice[-1] = twice[0]
        from similari_amd.points import sa_point_rows

        zp = np.ascontiguousarray(z).ctypes.data_as(C.POINTER(C.c_float))
        out = np.full(len(z) * 8, 77, u32)
        rows = lambda size=40, comps=2, host=zp: C.byref(sa_point_rows(size, comps, 0.0, 0, host, None, None))
        ip, cp = ids.ctypes.data_as(C.POINTER(C.c_uint64)), pc.ctypes.data_as(C.POINTER(C.c_uint32))
        f = lib.sa_pose_sort_predict
        many = np.zeros(65536, u32)
        cases = [
            (B, "twice", lambda: f(trk.h, len(ids), twice.ctypes.data_as(C.POINTER(C.c_uint64)), cp, rows(), out.ctypes.data, None)),
            (B, "null", lambda: f(trk.h, len(ids), None, cp, rows(), out.ctypes.data, None)),
            (B, "null", lambda: f(trk.h, len(ids), ip, None, rows(), out.ctypes.data, None)),
            (B, "null rows", lambda: f(trk.h, len(ids), ip, cp, None, out.ctypes.data, None)),
            (B, "struct_size", lambda: f(trk.h, len(ids), ip, cp, rows(size=32), out.ctypes.data, None)),
            (B, "comps", lambda: f(trk.h, len(ids), ip, cp, rows(comps=4), out.ctypes.data, None)),
            (B, "exactly one", lambda: f(trk.h, len(ids), ip, cp, rows(host=None), out.ctypes.data, None)),
            (B, "null out", lambda: f(trk.h, len(ids), ip, cp, rows(), None, None)),
            (U, "scenes", lambda: f(trk.h, 65536, np.arange(65536, dtype=u64).ctypes.data_as(C.POINTER(C.c_uint64)),
                                    many.ctypes.data_as(C.POINTER(C.c_uint32)), rows(), out.ctypes.data, None)),
        ]
        for k, (code, word, call) in enumerate(cases):
            assert call() == code, (k, lib.sa_last_error(eng.h).decode())
            assert word in lib.sa_last_error(eng.h).decode(), (k, lib.sa_last_error(eng.h).decode())
            assert (out == 77).all() and trk.last()["poses"] == 0 and trk.last()["scenes"] == 0, k
            assert bank.order().tolist() == order and [trk.epoch(s) for s in range(1, 9)] == epochs, k
            assert [trk.active(s) for s in range(1, 9)] == active and trk.wasted() == [], k
        with pytest.raises(EngineError):   # the same through peek
            trk.peek([1, 1], rows=DeviceRows(0x1000, 2, P * 2, SA_ELEM_F32), pose_counts=[1, 1])
        for x, t in zip(before, order):
            y = bank.state(t)
            assert (x[0] == y[0]).all() and bits(x[1], y[1]) and bits(x[2], y[2])
        got = trk.predict(call_of(fr))      # the next good call works, and now the idle tracks expire
        assert trk.last()["expired"] >= 1 and len(trk.wasted()) == trk.last()["expired"]
        assert [trk.epoch(f[0]) for f in fr] == [epochs[f[0] - 1] + 1 for f in fr]
