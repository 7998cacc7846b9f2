"""Point banks on the MI355X (similari_amd.points over include/similari_points.h) against the dense model tests/points_ref.py, which
tests/test_points_ref.py pins to the oracle: every out_xy, every distance and every state read back through get_state must carry the
model's bits.  "Bits" is the comparison of tests/test_points_emu.py: equal value bits, two NaNs counting as the same.

Shapes are the smallest that can go wrong: P in {1, 2, 17, 64, 65} (a single point, no power of two, a track that straddles a wave)
with n in {1, 3, 61} (n * P below, at and across blocks of 256 threads).  Device memory for the rows comes from tests/hipmem.py; the
torch tensors run in tests/points_child.py, because torch's HIP context wants to be the first of its process."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import devrows_ref as dref
import hipmem
import points_ref as R
from similari_amd import abi, synth
from similari_amd.devrows import DeviceRows
from similari_amd.engine import Engine, EngineError
from similari_amd.f16 import SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_F32
from similari_amd.points import SA_ROW_NONE, PointBank

pytestmark = pytest.mark.gpu
f32, u8, u16, u32, u64 = np.float32, np.uint8, np.uint16, np.uint32, np.uint64
WEIGHTS = [(R.PW, R.VW), (f32(0.11), f32(0.013))]
MODES = ("d2", "cost", "cost_inverted")


def bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(((a.view(u32) == b.view(u32)) | (np.isnan(a) & np.isnan(b))).all())


class Model:
    """tests/points_ref.Bank keyed by track id, and the order a bank keeps its tracks in."""

    def __init__(self, P, pw=R.PW, vw=R.VW, cap=512):
        self.P, self.b, self.row, self.ids, self.rows_used = P, R.Bank((cap, P), pw, vw), {}, [], 0

    def _sub(self, ids, create=False):
        for i in ids:
            if int(i) not in self.row:
                assert create, i
                self.row[int(i)] = self.rows_used   # a fresh row of the model: no state
                self.rows_used += 1
                self.ids.append(int(i))
        idx = np.array([self.row[int(i)] for i in ids], np.int64)
        sub = R.Bank((len(idx), self.P), self.b.pw, self.b.vw)
        sub.has, sub.mean, sub.cov = self.b.has[idx], self.b.mean[idx], self.b.cov[idx]
        return idx, sub

    def _back(self, idx, sub):
        self.b.has[idx], self.b.mean[idx], self.b.cov[idx] = sub.has, sub.mean, sub.cov

    def call(self, op, ids, *args, create=False):
        idx, sub = self._sub(ids, create)
        out = getattr(sub, op)(*args)
        self._back(idx, sub)
        return out

    def remove(self, ids):
        """sa_points_remove: the last track moves into each hole in turn, in call order."""
        for i in ids:
            if int(i) in self.row and int(i) in self.ids:
                at = self.ids.index(int(i))
                self.ids[at] = self.ids[-1]
                self.ids.pop()
                del self.row[int(i)]

    def state(self, i):
        r = self.row[int(i)]
        return self.b.has[r], self.b.mean[r], self.b.cov[r]


def check_states(bank, model, ids=None):
    ids = model.ids if ids is None else ids
    for i in ids:
        has, mean, cov = bank.state(i)
        mh, mm, mc = model.state(i)
        assert (has == mh).all(), i
        assert bits(mean[has], mm[mh]) and bits(cov[has], mc[mh]), i
        assert np.isnan(mean[~has]).all() and np.isnan(cov[~has]).all()
    assert bank.order().tolist() == model.ids


@pytest.fixture(scope="module")
def eng():
    e = Engine(abi.make_config(positional="iou", positional_threshold=0.3, device=0))
    yield e
    e.close()


def scene(rng, n, P, absent=0.0):
    z = rng.uniform(-200, 200, (n, P, 2)).astype(f32)
    pres = rng.random((n, P)) >= absent
    return z, pres


# ---- 1. the plain calls, every shape ---------------------------------------------------------------
@pytest.mark.parametrize("pw,vw", WEIGHTS)
@pytest.mark.parametrize("n", [1, 3, 61])
@pytest.mark.parametrize("P", [1, 2, 17, 64, 65])
def test_four_rounds_of_predict_distance_update(eng, P, n, pw, vw):
    rng = np.random.default_rng(P * 100 + n)
    ids = np.arange(10, 10 + n, dtype=u64)
    z, all_ = scene(rng, n, P)
    vel = rng.uniform(-3, 3, (n, P, 2))
    model = Model(P, pw, vw)
    with PointBank(eng, P, pw, vw) as bank:
        bank.initiate(ids, z)
        model.call("initiate", ids, z, all_, create=True)
        st = bank.last()
        assert (st["launches"], st["tracks"], st["points"], st["present"], st["capacity"]) == (1, n, n * P, n * P, 64)
        for k in range(4):
            assert bits(bank.predict(ids), model.call("predict", ids)), k
            assert bank.last()["launches"] == 1 and bank.last()["present"] == 0
            z = (z + vel + rng.normal(0, 0.7, z.shape)).astype(f32)
            for mode, name in enumerate(MODES):
                d = bank.distance(ids, z, mode=name)
                assert bits(d, model.call("distance", ids, z, all_, mode)), (k, name)
                assert np.isfinite(d).all() and bank.last()["launches"] == 1
            assert bits(bank.update(ids, z), model.call("update", ids, z, all_)), k
            assert bank.last()["launches"] == 1
        check_states(bank, model)


# ---- 2. step = initiate + predict + update = the model ---------------------------------------------
@pytest.mark.parametrize("P", [2, 17, 65])
def test_step_equals_the_plain_sequence_equals_the_model(eng, P):
    rng = np.random.default_rng(40 + P)
    n0, n1 = 23, 9   # n1 more ids are created mid-run
    ids = np.arange(1, n0 + n1 + 1, dtype=u64) * 7
    late = rng.random((n0 + n1, P)) < 0.25   # first sighted in round 3 at the earliest
    model = Model(P)
    with PointBank(eng, P) as a, PointBank(eng, P) as b:
        pos = rng.uniform(-100, 100, (n0 + n1, P, 2))
        for k in range(6):
            n = n0 if k < 2 else n0 + n1
            use = rng.permutation(n)[: max(n - 3, 1)] if k % 2 else np.arange(n)   # a call need not name every track
            pos += rng.normal(0, 1.5, pos.shape)
            z = pos[use].astype(f32)
            pres = (rng.random((len(use), P)) >= 0.3) & ~(late[use] & (k < 3))
            xy = a.step(ids[use], z, present=pres)
            assert a.last()["launches"] == 1 and a.last()["present"] == int(pres.sum())
            want = model.call("step", ids[use], z, pres, create=True)
            assert bits(xy, want), k
            # the plain calls: initiate what is first sighted, predict, update
            known = [i for i in ids[use] if int(i) in set(b.order().tolist())]
            has = np.zeros((len(use), P), bool)
            for j, i in enumerate(ids[use]):
                if i in known:
                    has[j] = b.state(i)[0]
            b.initiate(ids[use], z, present=pres & ~has)
            b.predict(ids[use])
            assert bits(b.update(ids[use], z, present=pres), want), k
            if k == 1:
                assert np.isnan(xy).any() and not np.isnan(xy).all()   # a point without a state reads NaN
        check_states(a, model)
        check_states(b, model)
        assert model.b.has[: n0 + n1].mean() > 0.9 and late.any()


# ---- 3. growth and removal -------------------------------------------------------------------------
def test_growth_keeps_the_states_and_removal_compacts(eng):
    P = 3
    rng = np.random.default_rng(50)
    model = Model(P)
    with PointBank(eng, P) as bank:
        caps = []
        first = 1
        for count in (40, 60, 100):   # 40, 100, 200 tracks: capacity 64, 128, 256
            ids = np.arange(first, first + count, dtype=u64)
            first += count
            z, pres = scene(rng, count, P, 0.2)
            assert bits(bank.step(ids, z, present=pres), model.call("step", ids, z, pres, create=True))
            caps.append(bank.last()["capacity"])
            check_states(bank, model)   # the earlier tracks' bits moved along
        assert caps == [64, 128, 256]
        assert bits(bank.predict(), model.call("predict", model.ids))
        # The first, a middle, the last and an unknown track, each named by where it lies NOW (after the first removal the track
        # that was last lies in slot 0).  Then the calls whose net moves are not one move per hole: [first, last, last but one]
        # and [first, last] — the call removes the track it has just moved into slot 0, and moves the next one there —;
        # [last but one, first] — the track moved into the last-but-one slot is moved again: a chain.  Then several at once with
        # unknown ids between.
        cases = (lambda m: [m[0]], lambda m: [m[len(m) // 2]], lambda m: [m[-1]], lambda m: [999],
                 lambda m: [m[0], m[-1], m[-2]], lambda m: [m[0], m[-1]], lambda m: [m[-2], m[0]],
                 lambda m: [m[4], m[-2], m[5], m[-3], m[100], 12345, m[6], m[-1]])
        gone = 0
        for k, pick in enumerate(cases):
            leaving = pick(list(model.ids))
            last_alone = leaving == [model.ids[-1]]
            bank.remove(np.array(leaving, u64))
            model.remove(leaving)
            gone += sum(1 for i in leaving if i not in (999, 12345))
            assert bank.last()["launches"] == (0 if last_alone or leaving == [999] else 1), k   # the last slot leaves without a move
            assert len(bank) == 200 - gone, k
            check_states(bank, model)
        assert gone == 17
        keep = np.array(model.ids[::3], u64)
        z, pres = scene(rng, len(keep), P, 0.2)
        assert bits(bank.step(keep, z, present=pres), model.call("step", keep, z, pres))
        bank.remove(np.array(model.ids, u64))
        model.remove(list(model.ids))
        assert len(bank) == 0 and bank.order().tolist() == []
        assert bank.predict().shape == (0, P, 2)
        ids = np.array([3, 1], u64)   # old ids come back as new tracks without a state
        z, pres = scene(rng, 2, P, 0.5)
        model = Model(P)
        assert bits(bank.step(ids, z, present=pres), model.call("step", ids, z, pres, create=True))
        check_states(bank, model)


# ---- 4. seeded states ------------------------------------------------------------------------------
def test_set_state_with_off_diagonal_mass_and_an_indefinite_covariance(eng):
    P = 5
    rng = np.random.default_rng(60)
    model = Model(P)
    ids = np.array([4, 9], u64)
    with PointBank(eng, P) as bank:
        z, pres = scene(rng, 2, P)
        bank.initiate(ids, z)
        model.call("initiate", ids, z, pres, create=True)
        a = rng.normal(0, 1, (2, P, 4, 4))
        cov = (a @ np.swapaxes(a, -1, -2) + np.eye(4) * 1e-3).astype(f32)   # SPD, every entry non-zero
        cov[1, :3] = -cov[1, :3]                                          # track 9, points 0..2: indefinite
        mean = rng.uniform(-5, 5, (2, P, 4)).astype(f32)
        has = np.ones((2, P), bool)
        has[0, 4] = False
        for j, i in enumerate(ids):
            bank.set_state(i, has[j], mean[j], cov[j])
            r = model.row[int(i)]
            model.b.has[r] = has[j]
            model.b.mean[r][has[j]], model.b.cov[r][has[j]] = mean[j][has[j]], cov[j][has[j]]
        check_states(bank, model)
        z = (mean[..., :2] + rng.normal(0, 1, (2, P, 2))).astype(f32)
        for mode, name in enumerate(MODES):
            d = bank.distance(ids, z, mode=name)
            assert bits(d, model.call("distance", ids, z, pres, mode)), name
            assert np.isnan(d[1, :3]).all() and np.isnan(d[0, 4]) and np.isfinite(d[0, :4]).all() and np.isfinite(d[1, 3:]).all()
        for k in range(2):
            assert bits(bank.update(ids, z), model.call("update", ids, z, pres)), k
            assert bits(bank.predict(ids), model.call("predict", ids)), k
        check_states(bank, model)
        assert np.isfinite(model.b.cov[model.row[9]]).all()


# ---- 5. presence -----------------------------------------------------------------------------------
def test_what_makes_a_point_present(eng):
    P = 4
    rng = np.random.default_rng(70)
    ids = np.arange(1, 9, dtype=u64)
    with PointBank(eng, P) as bank:
        z = rng.uniform(-9, 9, (8, P, 3)).astype(f32)
        z[..., 2] = rng.uniform(0, 1, (8, P))
        z[0, 0, 0], z[0, 1, 1], z[0, 2, 0], z[0, 3, 1] = np.nan, np.inf, -np.inf, np.nan
        z[1, 0, 2], z[1, 1, 2], z[1, 2, 2], z[1, 3, 2] = np.nan, 0.5, np.nextafter(f32(0.5), f32(0)), np.inf
        mask = rng.random((8, P)) > 0.3
        mask[1] = True
        for comps, ms, m in ((2, 0.0, None), (3, 0.5, None), (3, 0.5, mask), (2, 0.0, mask)):
            pts = np.ascontiguousarray(z[..., :comps])
            want = R.present_of(pts, ms, m)
            model = Model(P)
            bank.remove(ids)
            xy = bank.step(ids, pts, present=m, min_score=ms)
            assert bits(xy, model.call("step", ids, pts[..., :2], want, create=True)), (comps, m is None)
            assert bank.last()["present"] == int(want.sum())
            assert (np.isnan(xy[..., 0]) == ~want).all()
            if comps == 3 and m is None:
                assert want[1].tolist() == [False, True, False, True] and not want[0].any()
            check_states(bank, model)


# ---- 6. rows in device memory ----------------------------------------------------------------------
def to_source(x, elem):
    x = np.ascontiguousarray(x, f32)
    if elem == SA_ELEM_F32:
        return x
    if elem == SA_ELEM_F16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(u16)
    return (x.view(u32) >> 16).astype(u16)


@contextlib.contextmanager
def device_block(engine, image, register=True):
    ptr = hipmem.malloc(image.nbytes)
    try:
        hipmem.upload(ptr, image)
        if register:
            engine.register_device_block(ptr, image.nbytes, 0)
        yield ptr
    finally:
        if register:
            engine.unregister_device_block(ptr)
        hipmem.free(ptr)


@pytest.mark.parametrize("comps", [2, 3])
@pytest.mark.parametrize("elem", [SA_ELEM_F32, SA_ELEM_F16, SA_ELEM_BF16])
def test_rows_read_from_device_memory(eng, elem, comps):
    P, B, off = 17, 30, 4
    L = P * comps
    W = L + 11   # a column slice of a wider output: the row stride exceeds P * comps
    rng = np.random.default_rng(80 + elem)
    eb = 4 if elem == SA_ELEM_F32 else 2
    ids = np.arange(1, 24, dtype=u64)
    n = len(ids)
    model = Model(P)
    with PointBank(eng, P) as dev, PointBank(eng, P) as host:
        for k in range(3):
            vals = rng.uniform(-300, 300, (B, W)).astype(f32)
            if comps == 3:
                vals[:, off + 2: off + L: comps] = rng.uniform(0, 1, (B, P))   # the scores
            vals[3, off] = np.nan   # a point that is not finite in the source
            src = to_source(vals, elem)
            wide = dref.widen(src, elem)[:, off: off + L].reshape(B, P, comps)
            index = rng.integers(0, B, n).astype(u32)
            index[5] = index[2]          # a row named twice
            index[7] = index[11] = SA_ROW_NONE
            index[0] = 3
            z = np.zeros((n, P, comps), f32)
            got = index != SA_ROW_NONE
            z[got] = wide[index[got]]
            mask = np.repeat(got[:, None], P, 1)   # the host twin: a track without a row has every point absent
            with device_block(eng, src) as ptr:
                rows = DeviceRows(ptr + off * eb, B, W, elem, index)
                xy = dev.step(ids, rows=rows, comps=comps, min_score=0.4)
                st = dev.last()
                want = host.step(ids, z, present=mask, min_score=0.4)
                assert bits(xy, want), k
                pres = R.present_of(z, 0.4, mask)
                assert bits(xy, model.call("step", ids, z[..., :2], pres, create=True)), k
                assert st["launches"] == 1 and st["present"] == int(pres.sum())
                assert st["bytes_h2d"] == n * 4 + n * 4   # the slot table and the index: no point data
                assert st["src_bytes"] == int(got.sum()) * L * eb
                assert host.last()["bytes_h2d"] == n * 4 + z.nbytes + n * P and host.last()["src_bytes"] == 0
                for name in MODES:
                    assert bits(dev.distance(ids, rows=rows, comps=comps, min_score=0.4, mode=name),
                                host.distance(ids, z, present=mask, min_score=0.4, mode=name)), name
                # without an index: track i reads row i
                d0 = dev.distance(ids, rows=DeviceRows(ptr + off * eb, B, W, elem), comps=comps, mode="d2")
                assert bits(d0, host.distance(ids, np.ascontiguousarray(wide[:n]), mode="d2"))
                assert dev.last()["bytes_h2d"] == n * 4
        check_states(dev, model)
        check_states(host, model)
        assert not model.b.has[model.row[8]].any()   # index 7 never had a row


def test_rows_outside_a_registered_block_are_refused(eng):
    P = 6
    ids = np.arange(1, 5, dtype=u64)
    img = np.zeros((8, P * 2), f32)
    with PointBank(eng, P) as bank:
        bank.step(ids, np.zeros((4, P, 2), f32))
        before = [bank.state(i) for i in ids]
        with device_block(eng, img, register=False) as ptr:
            with pytest.raises(EngineError) as ei:
                bank.step(ids, rows=DeviceRows(ptr, 8, P * 2, SA_ELEM_F32))
            assert ei.value.code == abi.SA_ERR_BAD_ARG and "registered" in str(ei.value)
        with device_block(eng, img) as ptr:
            bank.step(ids, rows=DeviceRows(ptr, 8, P * 2, SA_ELEM_F32))   # inside: accepted
            before = [bank.state(i) for i in ids]
            for bad in (DeviceRows(ptr, 9, P * 2, SA_ELEM_F32), DeviceRows(ptr + 4, 8, P * 2, SA_ELEM_F32),
                        DeviceRows(ptr, 8, P * 2 + 1, SA_ELEM_F32), DeviceRows(ptr, 8, P * 2 - 1, SA_ELEM_F32),
                        DeviceRows(ptr, 8, P * 2, SA_ELEM_F32, [0, 1, 8, 2]), DeviceRows(ptr, 3, P * 2, SA_ELEM_F32),
                        DeviceRows(ptr + 2, 4, P * 2, SA_ELEM_F32), DeviceRows(ptr, 8, P * 2, 99)):
                with pytest.raises(EngineError) as ei:
                    bank.step(ids, rows=bad)
                assert ei.value.code == abi.SA_ERR_BAD_ARG
                assert bank.last()["launches"] == 0
            eng.register_device_block(ptr, img.nbytes, 1)   # the same block, said to lie on another device
            with pytest.raises(EngineError) as ei:
                bank.step(ids, rows=DeviceRows(ptr, 8, P * 2, SA_ELEM_F32))
            assert ei.value.code == abi.SA_ERR_BAD_ARG and "device 1" in str(ei.value)
        after = [bank.state(i) for i in ids]
        for x, y in zip(before, after):
            assert (x[0] == y[0]).all() and bits(x[1], y[1]) and bits(x[2], y[2])


# ---- 7. refusals -----------------------------------------------------------------------------------
def test_every_refusal_leaves_the_bank_as_it_was(eng):
    import ctypes as C

    from similari_amd import points as PT

    P = 3
    lib = eng.lib
    with PointBank(eng, P) as bank:
        ids = np.array([5, 6, 7], u64)
        z = np.random.default_rng(90).uniform(-5, 5, (3, P, 2)).astype(f32)
        bank.step(ids, z)
        before = [bank.state(i) for i in ids]
        order = bank.order().tolist()
        xy = np.zeros((3, P, 2), f32)
        fp, idp = xy.ctypes.data_as(C.POINTER(C.c_float)), ids.ctypes.data_as(C.POINTER(C.c_uint64))
        zp = z.ctypes.data_as(C.POINTER(C.c_float))
        flags = np.ones(P, u8)
        hp = flags.ctypes.data_as(C.POINTER(C.c_uint8))

        def rows(size=40, comps=2, host=zp, dev=None):
            return C.byref(PT.sa_point_rows(size, comps, 0.0, 0, host, None, dev))

        def arr(*v):
            a = np.array(v, u64)
            return a.ctypes.data_as(C.POINTER(C.c_uint64)), a

        d = DeviceRows(0x1000, 3, P * 2, SA_ELEM_F32).struct()
        B, NF = abi.SA_ERR_BAD_ARG, abi.SA_ERR_NOT_FOUND
        zero, twice, unknown = arr(5, 0, 7), arr(5, 6, 5), arr(5, 6, 8)
        cases = [
            (B, lambda: lib.sa_points_step(bank.h, 3, None, rows(), fp)),
            (B, lambda: lib.sa_points_step(bank.h, 3, idp, None, fp)),
            (B, lambda: lib.sa_points_step(bank.h, 3, zero[0], rows(), fp)),
            (B, lambda: lib.sa_points_step(bank.h, 3, twice[0], rows(), fp)),
            (B, lambda: lib.sa_points_initiate(bank.h, 3, twice[0], rows())),
            (B, lambda: lib.sa_points_step(bank.h, 3, idp, rows(size=32), fp)),
            (B, lambda: lib.sa_points_step(bank.h, 3, idp, rows(comps=1), fp)),
            (B, lambda: lib.sa_points_step(bank.h, 3, idp, rows(comps=4), fp)),
            (B, lambda: lib.sa_points_step(bank.h, 3, idp, rows(host=None), fp)),
            (B, lambda: lib.sa_points_step(bank.h, 3, idp, rows(dev=C.pointer(d)), fp)),
            (B, lambda: lib.sa_points_update(bank.h, 3, idp, rows(host=None, dev=C.pointer(d)), fp)),   # a span in no registered block
            (B, lambda: lib.sa_points_distance(bank.h, 3, idp, rows(), 3, fp)),
            (B, lambda: lib.sa_points_distance(bank.h, 3, idp, rows(), 0, None)),
            (B, lambda: lib.sa_points_predict(bank.h, 3, zero[0], fp)),
            (B, lambda: lib.sa_points_remove(bank.h, 3, twice[0])),
            (B, lambda: lib.sa_points_remove(bank.h, 3, zero[0])),
            (B, lambda: lib.sa_points_get_state(bank.h, 0, None, None, None)),
            (B, lambda: lib.sa_points_get_state(bank.h, 5, None, fp, fp)),
            (NF, lambda: lib.sa_points_predict(bank.h, 3, unknown[0], fp)),
            (NF, lambda: lib.sa_points_update(bank.h, 3, unknown[0], rows(), fp)),
            (NF, lambda: lib.sa_points_distance(bank.h, 3, unknown[0], rows(), 0, fp)),
            (NF, lambda: lib.sa_points_get_state(bank.h, 8, hp, fp, fp)),
            (NF, lambda: lib.sa_points_set_state(bank.h, 8, hp, fp, fp)),
        ]
        for k, (code, f) in enumerate(cases):
            assert f() == code, k
            assert lib.sa_last_error(eng.h), k
            assert bank.last()["launches"] == 0, k
        assert bank.order().tolist() == order
        for x, i in zip(before, ids):
            y = bank.state(i)
            assert (x[0] == y[0]).all() and bits(x[1], y[1]) and bits(x[2], y[2])
        # creation
        h = PT.POINTS()
        o = PT.sa_points_options()
        lib.sa_points_options_default(C.byref(o))
        o.points = 0
        assert lib.sa_points_create(eng.h, C.byref(o), C.byref(h)) == B and not h.value
        o.points, o.struct_size = 3, 12
        assert lib.sa_points_create(eng.h, C.byref(o), C.byref(h)) == B and not h.value
        assert lib.sa_points_create(eng.h, None, C.byref(h)) == B
    # tracks x points >= 2^31: refused before anything is allocated
    with PointBank(eng, 1 << 30) as big:
        with pytest.raises(EngineError) as ei:
            big.predict(np.array([1], u64))
        assert ei.value.code == abi.SA_ERR_NOT_FOUND
        o = PT.sa_point_rows(40, 2, 0.0, 0, zp, None, None)
        two = np.array([1, 2], u64)
        assert lib.sa_points_step(big.h, 2, two.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(o), None) == abi.SA_ERR_UNSUPPORTED
        assert len(big) == 0


# ---- 8. one launch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,P", [(1, 1), (61, 65)])
def test_one_launch_whatever_n_and_p_are(eng, n, P):
    rng = np.random.default_rng(95)
    ids = np.arange(1, n + 1, dtype=u64)
    z, pres = scene(rng, n, P)
    with PointBank(eng, P) as bank:
        for call in (lambda: bank.initiate(ids, z), lambda: bank.predict(ids), lambda: bank.predict(), lambda: bank.update(ids, z),
                     lambda: bank.distance(ids, z), lambda: bank.step(ids, z)):
            call()
            st = bank.last()
            assert st["launches"] == 1 and st["points"] == n * P and st["device_ms"] >= 0
        bank.remove(ids[: max(n // 2, 1)])
        assert bank.last()["launches"] == (1 if n > 1 else 0)


def test_predict_of_every_track_is_predict_of_the_order(eng):
    P = 17
    rng = np.random.default_rng(96)
    ids = rng.permutation(np.arange(1, 40, dtype=u64))
    z, pres = scene(rng, len(ids), P, 0.3)
    with PointBank(eng, P) as a, PointBank(eng, P) as b:
        for bank in (a, b):
            bank.step(ids, z, present=pres)
            bank.remove(ids[3:9])
        assert a.order().tolist() == b.order().tolist()
        xa = a.predict()
        assert a.last()["bytes_h2d"] == 0
        assert bits(xa, b.predict(b.order()))
        for i in a.order():
            x, y = a.state(i), b.state(i)
            assert (x[0] == y[0]).all() and bits(x[1], y[1]) and bits(x[2], y[2])


# ---- 9. beside the engine's own work ---------------------------------------------------------------
def test_a_bank_stepped_between_frames_changes_neither_result():
    rng = np.random.default_rng(97)
    sc = synth.sort_scene(rng, 50, 60)
    det = abi.make_detections(sc["det_boxes"])
    P = 17
    ids = np.arange(1, 31, dtype=u64)
    frames = [scene(rng, len(ids), P, 0.3) for _ in range(3)]

    def run(with_bank):
        e = Engine(abi.make_config(positional="iou", positional_threshold=0.3, device=0))
        try:
            e.upsert(3, abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"]))
            out, xy = [], []
            bank = PointBank(e, P) if with_bank else None
            for k, (z, pres) in enumerate(frames):
                got = e.associate(3, 1 + k, det)
                out.append((np.array(got[0]).copy(), np.array(got[1]).copy()))
                if bank:
                    xy.append(bank.step(ids, z, present=pres))
            if bank:
                bank.close()
            return out, xy
        finally:
            e.close()

    plain, _ = run(False)
    mixed, xy = run(True)
    for (a, b), (c, d) in zip(plain, mixed):
        assert (a == c).all() and (b == d).all()
    assert (plain[0][0] != 0).sum() > 25
    model = Model(P)
    for (z, pres), got in zip(frames, xy):
        assert bits(got, model.call("step", ids, z, pres, create=True))


def test_an_engine_destroyed_first_leaves_a_bank_that_refuses():
    e = Engine(abi.make_config(positional="iou", positional_threshold=0.3, device=0))
    bank = PointBank(e, 2)
    ids = np.array([1], u64)
    bank.step(ids, np.zeros((1, 2, 2), f32))
    lib, h = e.lib, bank.h
    e.close()
    n = u32(0)
    import ctypes as C

    xy = np.zeros((1, 2, 2), f32)
    assert lib.sa_points_predict(h, 1, ids.ctypes.data_as(C.POINTER(C.c_uint64)), xy.ctypes.data_as(C.POINTER(C.c_float))) == abi.SA_ERR_STATE
    assert lib.sa_points_predict(h, 0, None, None) == abi.SA_ERR_STATE
    assert lib.sa_points_remove(h, 1, ids.ctypes.data_as(C.POINTER(C.c_uint64))) == abi.SA_ERR_STATE
    assert lib.sa_points_count(h, C.byref(C.c_uint32())) == abi.SA_ERR_STATE
    assert b"destroyed" in lib.sa_last_error(None)
    lib.sa_points_destroy(h)
    bank.h = None


# ---- 10. the tensor interface ----------------------------------------------------------------------
def test_points_of_a_torch_tensor_on_the_gpu():
    """register_tensor and DeviceRows.from_tensor of a column slice of an f32, an f16 and a bf16 tensor, an index with repeats and
    SA_ROW_NONE, against a host-fed twin.  Runs tests/points_child.py: torch's HIP context wants to be the first one of its process."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "points_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "POINT-ROWS-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
