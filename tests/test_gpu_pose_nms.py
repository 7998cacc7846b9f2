"""Pose NMS by OKS on the MI355X (similari_amd.pose_nms over include/similari_pose_nms.h) against the numpy model tests/pose_nms_ref.py:
the tap carries the model's order and bits, the keeps are the model's index for index, a batch is its single calls, device rows leave
the bits of the host-fed call, every refusal leaves the outputs alone, and KeypointSort behind it creates one track per person.  "Bits"
is the comparison of tests/test_gpu_points.py.

Shapes: m' in {1, 2, 15, 16, 17, 63, 64, 65, 130} (the block edges of 16 rows, the word edge of 64 columns, the diagonal word's
i < j rule) x P in {1, 2, 17, 65} (65 crosses the 64-point LDS chunk) x min_common in {1, 3}; 4100 and 8200 survivors at P = 3 for the
sweep classes 2 and 4; 16385 for the limit."""
import ctypes as C

import numpy as np
import pytest

import devrows_ref as dref
import oks_ref as OR
import pose_nms_ref as NR
from similari_amd import abi
from similari_amd import pose_nms as N
from similari_amd.devrows import DeviceRows
from similari_amd.engine import Engine, EngineError
from similari_amd.f16 import SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_F32
from similari_amd.points import SA_ROW_NONE, sa_point_rows
from similari_amd.pose_sort import KeypointSort
from test_gpu_points import bits, device_block, to_source
from test_pose_nms_ref import chain

pytestmark = pytest.mark.gpu
f32, u8, u32 = np.float32, np.uint8, np.uint32
SIZES = [1, 2, 15, 16, 17, 63, 64, 65, 130]
MIN_SCORE, SCORE_THR, NMS_THR = 0.15, 0.2, 0.5
ZERO_STATS = dict(scenes=0, poses=0, launches=0, host_waits=0, bytes_h2d=0, bytes_d2h=0, src_bytes=0, device_ms=0.0)


@pytest.fixture(scope="module")
def eng():
    e = Engine(abi.make_config(positional="iou", positional_threshold=0.3, device=0))
    yield e
    e.close()


_scenes, _models = {}, {}


def scene(n, P, seed=0):
    """n + 3 poses of which n pass the score filter: clusters of jittered duplicates with a point score and a present mask, a fifth of
    the points NaN; from 15 survivors on also a single-point pose, a collinear one, an exact duplicate and one without any point.
    -> (pts [m, P, 3], scores [m], mask [m, P]), read-only."""
    key = (n, P, seed)
    if key not in _scenes:
        m = n + 3
        pts, scores, _ = NR.crowd(900 + 7 * n + P + 1000 * seed, max(1, n // 4), m, P, jitter=0.04, absent=0.2, comps=3)
        rng = np.random.default_rng(n * 100 + P + seed)
        scores = np.clip(scores, 0.25, None)
        scores[rng.permutation(m)[:3]] = [np.nan, 0.1, SCORE_THR]   # three that the filter drops, the last at the threshold itself
        mask = rng.random((m, P)) > 0.1
        if n >= 15:
            a, b, c, d, e = np.flatnonzero(scores > SCORE_THR)[:5]
            pts[a, 1:, 0] = np.nan                 # a single point
            pts[b, :, 1] = 3.0                     # collinear, axis-parallel
            pts[c], mask[c] = pts[d], mask[d]      # an exact duplicate
            pts[e, :, 0] = np.nan                  # no point at all
        for x in (pts, scores, mask):
            x.setflags(write=False)
        _scenes[key] = (pts, scores, mask)
    return _scenes[key]


def model(n, P, min_common, seed=0):
    key = (n, P, min_common, seed)
    if key not in _models:
        pts, scores, mask = scene(n, P, seed)
        _models[key] = NR.nms(pts, scores, OR.sigmas_for(P), NMS_THR, SCORE_THR, min_common, mask, MIN_SCORE, want_matrix=True)
    return _models[key]


def kw(P, min_common=1, mask=None):
    return dict(sigmas=OR.sigmas_for(P), score_threshold=SCORE_THR, min_common=min_common, present=mask, min_score=MIN_SCORE)


# ---- 1. the tap ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_common", [1, 3])
@pytest.mark.parametrize("P", [1, 2, 17, 65])
@pytest.mark.parametrize("n", SIZES)
def test_the_tap_carries_the_models_order_and_bits(eng, n, P, min_common):
    pts, scores, mask = scene(n, P)
    keep, order, w = model(n, P, min_common)
    got_order, got_w = N.pose_nms_matrix(eng, pts, scores, **kw(P, min_common, mask))
    st = N.last(eng)
    assert len(order) == n and got_order.tolist() == order.tolist()
    assert bits(got_w, w)   # NaNs in the same places: on and below the diagonal, refused pairs, pairs that do not exist
    assert (st["scenes"], st["poses"], st["launches"], st["host_waits"]) == (1, n, 2, 1)
    assert st["bytes_h2d"] == 24 + 4 * n + 4 * P + n * P * 12 + n * P and st["bytes_d2h"] == 4 * n * n and st["src_bytes"] == 0
    if P == 1:
        assert np.isnan(got_w).all()
    elif n >= 15 and P >= 3 and min_common == 1:
        real = got_w[np.isfinite(got_w)]
        assert (real == 1.0).any() and ((real > 0) & (real < 1)).any() and np.isnan(got_w[np.triu_indices(n, 1)]).any()


# ---- 2. the keeps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_common", [1, 3])
@pytest.mark.parametrize("P", [1, 2, 17, 65])
@pytest.mark.parametrize("n", SIZES)
def test_the_keeps_are_the_models(eng, n, P, min_common):
    pts, scores, mask = scene(n, P)
    keep, order, w = model(n, P, min_common)
    got = N.pose_nms(eng, pts, scores, nms_threshold=NMS_THR, **kw(P, min_common, mask))
    st = N.last(eng)
    assert got.dtype == np.uint32 and got.tolist() == keep.tolist()
    assert (st["scenes"], st["poses"], st["launches"], st["host_waits"], st["bytes_d2h"]) == (1, n, 3, 1, n)
    if n >= 15 and P >= 17 and min_common == 1:
        assert len(keep) < n   # somebody was suppressed


def test_the_nms_threshold_is_strict_at_a_weight_that_occurs(eng):
    pts, scores, mask = scene(65, 17)
    keep, order, w = model(65, 17, 1)
    real = np.sort(w[np.isfinite(w) & (w > 0.2) & (w < 1)])
    for thr in (real[len(real) // 2], real[-1], f32(1.0)):   # (1.0 occurs too: the exact duplicate is not suppressed at it)
        i, j = np.argwhere(w == thr)[0]
        pair = np.array([order[i], order[j]])
        want = NR.nms(pts, scores, OR.sigmas_for(17), float(thr), SCORE_THR, 1, mask, MIN_SCORE)
        assert N.pose_nms(eng, pts, scores, nms_threshold=float(thr), **kw(17, 1, mask)).tolist() == want.tolist()
        assert N.pose_nms(eng, pts[pair], scores[pair], nms_threshold=float(thr), **kw(17, 1, mask[pair])).tolist() == [0, 1]
        below = float(np.nextafter(thr, f32(0)))
        assert N.pose_nms(eng, pts[pair], scores[pair], nms_threshold=below, **kw(17, 1, mask[pair])).tolist() == [0]


def test_the_score_threshold_is_strict_at_a_score_that_occurs(eng):
    pts, scores, mask = scene(64, 17)
    thr = float(np.sort(scores[np.isfinite(scores)])[30])
    want = NR.nms(pts, scores, OR.sigmas_for(17), NMS_THR, thr, 1, mask, MIN_SCORE, want_matrix=True)
    args = kw(17, 1, mask)
    args["score_threshold"] = thr
    got = N.pose_nms(eng, pts, scores, nms_threshold=NMS_THR, **args)
    order, _ = N.pose_nms_matrix(eng, pts, scores, **args)
    assert got.tolist() == want[0].tolist() and order.tolist() == want[1].tolist()
    assert int(np.flatnonzero(scores == f32(thr))[0]) not in order.tolist() and len(order) == int((scores > f32(thr)).sum())


def test_the_chain_case_and_equal_scores(eng):
    pts, scores, thr = chain()
    sig = OR.sigmas_for(17)
    assert N.pose_nms(eng, pts, scores, sig, nms_threshold=thr).tolist() == [0, 2]
    assert N.pose_nms(eng, pts[1:], scores[1:], sig, nms_threshold=thr).tolist() == [0]
    pts, _, mask = scene(130, 17)
    same = np.full(len(pts), 0.5, f32)
    want = NR.nms(pts, same, sig, NMS_THR, None, 1, mask, MIN_SCORE, want_matrix=True)
    assert want[1].tolist() == list(range(len(pts)))   # the caller's order
    assert N.pose_nms(eng, pts, same, sig, NMS_THR, present=mask, min_score=MIN_SCORE).tolist() == want[0].tolist()
    assert N.pose_nms_matrix(eng, pts, same, sig, present=mask, min_score=MIN_SCORE)[0].tolist() == want[1].tolist()


# ---- 3. the sweep classes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4100, 8200])
def test_scenes_of_the_wider_sweep_classes(eng, n):
    """65 and 129 mask words per row: k_nms_sweep<2> and <4>.  Clustered duplicates, so that thousands are suppressed."""
    pts, scores, _ = NR.crowd(n, 150, n, 3, jitter=0.02, absent=0.05)
    sig = OR.sigmas_for(3)
    want = NR.nms_lazy(pts, scores, sig, NMS_THR, min_common=2)
    got = N.pose_nms(eng, pts, scores, sig, NMS_THR, min_common=2)
    st = N.last(eng)
    assert got.tolist() == want.tolist() and 100 < len(want) < n - 2000
    assert (st["poses"], st["launches"], st["host_waits"], st["bytes_d2h"]) == (n, 3, 1, n)


def test_16385_survivors_are_refused(eng):
    n = 16385
    pts, scores = np.zeros((n, 3, 2), f32), np.full(n, 0.5, f32)
    o_keep = np.full(n, 77, u32)
    sig, o = N.options(eng.lib, OR.sigmas_for(3))
    r = sa_point_rows(C.sizeof(sa_point_rows), 2, 0.0, 0, pts.ctypes.data_as(N.F32_P), None, None)
    cnt = C.c_uint32(77)
    rc = eng.lib.sa_pose_nms(eng.h, C.byref(o), n, C.byref(r), scores.ctypes.data_as(N.F32_P), o_keep.ctypes.data_as(N.U32_P), C.byref(cnt))
    assert rc == abi.SA_ERR_UNSUPPORTED and b"16384" in eng.lib.sa_last_error(eng.h)
    assert cnt.value == 77 and (o_keep == 77).all() and N.last(eng) == ZERO_STATS
    scores[0] = np.nan   # one fewer passes the filter
    assert len(N.pose_nms(eng, pts, scores, OR.sigmas_for(3))) == n - 1   # P = 3 at one spot: nobody has a body size


# ---- 4. the batch ----------------------------------------------------------------------------------------------------------------
COUNTS = [0, 1, 64, 0, 65, 130, 17]


def batch_scenes():
    """Scenes of COUNTS poses, some of which the filter drops; the scene of 64 is the first 64 poses of the scene of 65 behind it, at
    identical coordinates."""
    return [tuple(x[:n] for x in scene(65 if n == 64 else max(n, 1), 17, seed=1)) for n in COUNTS]


def test_a_batch_is_its_single_calls(eng):
    scenes = batch_scenes()
    assert [len(s[1]) for s in scenes] == COUNTS
    args = dict(sigmas=OR.sigmas_for(17), nms_threshold=NMS_THR, score_threshold=SCORE_THR, min_score=MIN_SCORE)
    singles, launches = [], set()
    for pts, scores, mask in scenes:
        singles.append(N.pose_nms(eng, pts, scores, present=mask, **args))
        if (scores > f32(SCORE_THR)).any():   # (a call in which no pose passes the filter launches nothing)
            launches.add(N.last(eng)["launches"])
    got = N.pose_nms_batch(eng, scenes, **args)
    st = N.last(eng)
    assert [g.tolist() for g in got] == [s.tolist() for s in singles]
    assert launches == {3} and (st["scenes"], st["launches"], st["host_waits"]) == (7, 3, 1)
    survivors = sum(int((s[1] > f32(SCORE_THR)).sum()) for s in scenes)
    assert st["poses"] == survivors and st["bytes_d2h"] == survivors
    assert st["bytes_h2d"] == 7 * 24 + 4 * survivors + 4 * 17 + survivors * 17 * 12 + survivors * 17
    assert any(len(g) < int((s[1] > f32(SCORE_THR)).sum()) for g, s in zip(got, scenes))
    for g, s in zip(got, scenes):   # and each scene is the model's
        assert g.tolist() == NR.nms(s[0], s[1], OR.sigmas_for(17), NMS_THR, SCORE_THR, 1, s[2], MIN_SCORE).tolist()


def test_scenes_never_see_each_other_and_empty_calls(eng):
    pts, scores, thr = chain()
    sig = OR.sigmas_for(17)
    one = (pts[:1], scores[:1])
    assert [g.tolist() for g in N.pose_nms_batch(eng, [one, one, one], sig, nms_threshold=0.1)] == [[0], [0], [0]]
    assert N.pose_nms(eng, np.concatenate([pts[:1]] * 3), scores[:1] * 3, sig, nms_threshold=0.1).tolist() == [0]   # in ONE scene they do
    assert N.pose_nms_batch(eng, [], sig) == [] and N.last(eng) == ZERO_STATS
    empty = (np.zeros((0, 17, 2), f32), np.zeros(0, f32))
    assert [g.tolist() for g in N.pose_nms_batch(eng, [empty, empty], sig)] == [[], []]
    assert N.last(eng) == dict(ZERO_STATS, scenes=2)
    assert N.pose_nms(eng, empty[0], empty[1], sig).tolist() == [] and N.last(eng) == dict(ZERO_STATS, scenes=1)
    order, w = N.pose_nms_matrix(eng, empty[0], empty[1], sig)
    assert order.tolist() == [] and w.shape == (0, 0)
    assert N.pose_nms(eng, pts, [np.nan] * 3, sig).tolist() == []   # all filtered


# ---- 5. device rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("comps", [2, 3])
@pytest.mark.parametrize("elem", [SA_ELEM_F32, SA_ELEM_F16, SA_ELEM_BF16])
def test_poses_read_from_device_memory(eng, elem, comps):
    """Rows in f32, f16 and bf16, a column slice of a wider block (strided), gathered by an index with SA_ROW_NONE and a row named twice."""
    P, m, B, off = 17, 70, 90, 4
    L = P * comps
    W = L + 11
    eb = 4 if elem == SA_ELEM_F32 else 2
    rng = np.random.default_rng(17 + elem + comps)
    poses, scores, mask = scene(m - 3, P, seed=2)
    index = rng.permutation(B)[:m].astype(u32)
    index[3] = index[9] = SA_ROW_NONE
    index[5] = index[2]   # a duplicate by name
    got = index != SA_ROW_NONE
    vals = rng.uniform(-300, 300, (B, W)).astype(f32)
    block = np.zeros((B, P, comps), f32)
    block[index[got]] = poses[got][..., :comps]
    vals[:, off: off + L] = block.reshape(B, L)
    src = to_source(vals, elem)
    wide = dref.widen(src, elem)[:, off: off + L].reshape(B, P, comps)
    z = np.full((m, P, comps), np.nan, f32)
    z[got] = wide[index[got]]
    sig = OR.sigmas_for(P)
    args = dict(sigmas=sig, score_threshold=SCORE_THR, min_score=MIN_SCORE, present=mask)
    with device_block(eng, src) as ptr:
        rows = DeviceRows(ptr + off * eb, B, W, elem, index)
        keep_d = N.pose_nms(eng, None, scores, nms_threshold=NMS_THR, rows=rows, comps=comps, **args)
        st = N.last(eng)
        order_d, w_d = N.pose_nms_matrix(eng, None, scores, rows=rows, comps=comps, **args)
        keep_h = N.pose_nms(eng, z, scores, nms_threshold=NMS_THR, **args)
        order_h, w_h = N.pose_nms_matrix(eng, z, scores, **args)
        n = m - 3
        assert keep_d.tolist() == keep_h.tolist() and order_d.tolist() == order_h.tolist() and bits(w_d, w_h) and len(order_d) == n
        assert keep_d.tolist() == NR.nms(z, scores, sig, NMS_THR, SCORE_THR, 1, mask, MIN_SCORE).tolist()
        read = int((got & (scores > f32(SCORE_THR))).sum())
        assert st["bytes_h2d"] == 24 + 4 * n + 4 * P + n * P and st["src_bytes"] == read * L * eb   # the table, var2, the flags: no pose
        assert st["bytes_d2h"] == n and (st["launches"], st["host_waits"]) == (3, 1)
        # no index, no mask: the rows as they lie; and as a batch of three scenes over the same rows
        plain = DeviceRows(ptr + off * eb, B, W, elem)
        sc_all = np.random.default_rng(3).uniform(0.3, 1, B).astype(f32)
        keep_p = N.pose_nms(eng, None, sc_all, sig, NMS_THR, min_score=MIN_SCORE, rows=plain, comps=comps)
        assert N.last(eng)["bytes_h2d"] == 24 + 4 * B + 4 * P
        assert keep_p.tolist() == N.pose_nms(eng, np.ascontiguousarray(wide), sc_all, sig, NMS_THR, min_score=MIN_SCORE).tolist()
        cuts = [(0, 20), (20, 20), (20, 90)]
        got_b = N.pose_nms_batch(eng, [(None, sc_all[a:b]) for a, b in cuts], sig, NMS_THR, min_score=MIN_SCORE, rows=plain, comps=comps)
        for (a, b), g in zip(cuts, got_b):
            assert g.tolist() == N.pose_nms(eng, np.ascontiguousarray(wide[a:b]), sc_all[a:b], sig, NMS_THR, min_score=MIN_SCORE).tolist()


def test_keep_rows_composes_the_index():
    rows = DeviceRows(0x1000, 50, 40, SA_ELEM_F16)
    k = N.keep_rows(rows, [7, 3, 9])
    assert k.index.tolist() == [7, 3, 9] and (k.ptr, k.n_rows, k.row_stride, k.elem) == (0x1000, 50, 40, SA_ELEM_F16)
    k2 = N.keep_rows(DeviceRows(0x1000, 50, 40, SA_ELEM_F16, [10, 11, SA_ROW_NONE, 13]), [3, 2, 0])
    assert k2.index.tolist() == [13, SA_ROW_NONE, 10]


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_outputs_and_zeroes_the_stats(eng):
    P, m = 17, 6
    pts, scores, _ = NR.crowd(5, 2, m, P)
    lib = eng.lib
    keep, cnt = np.full(m, 77, u32), C.c_uint32(77)
    order, w = np.full(m, 77, u32), np.full((m, m), 77, f32)

    def call(o, rows, sc=scores, n=m, which="nms"):
        N.pose_nms(eng, pts, scores, OR.sigmas_for(P))   # something for the refusal to zero
        assert N.last(eng)["launches"] == 3
        scp = None if sc is None else sc.ctypes.data_as(N.F32_P)
        ro = None if rows is None else C.byref(rows)
        if which == "nms":
            rc = lib.sa_pose_nms(eng.h, None if o is None else C.byref(o), n, ro, scp, keep.ctypes.data_as(N.U32_P), C.byref(cnt))
        elif which == "matrix":
            rc = lib.sa_pose_nms_matrix(eng.h, None if o is None else C.byref(o), n, ro, scp, order.ctypes.data_as(N.U32_P), w.ctypes.data_as(N.F32_P),
                                        C.byref(cnt))
        else:
            counts = np.array([2, n - 2], u32)
            outs = (N.U32_P * 2)(keep.ctypes.data_as(N.U32_P), keep[2:].ctypes.data_as(N.U32_P))
            on = np.full(2, 77, u32)
            rc = lib.sa_pose_nms_batch(eng.h, None if o is None else C.byref(o), 2, counts.ctypes.data_as(N.U32_P), ro, scp, outs, on.ctypes.data_as(N.U32_P))
            assert (on == 77).all()
        assert cnt.value == 77 and (keep == 77).all() and (order == 77).all() and (w == 77).all()
        assert N.last(eng) == ZERO_STATS
        return rc, lib.sa_last_error(eng.h).decode()

    def opts(**over):
        sig, o = N.options(lib, OR.sigmas_for(P))
        for k, v in over.items():
            setattr(o, k, v)
        return sig, o

    def host_rows(**over):
        r = sa_point_rows(C.sizeof(sa_point_rows), 2, 0.0, 0, pts.ctypes.data_as(N.F32_P), None, None)
        for k, v in over.items():
            setattr(r, k, v)
        return r

    sig, good = opts()
    for which in ("nms", "matrix", "batch"):
        assert call(None, host_rows(), which=which)[0] == abi.SA_ERR_BAD_ARG
        assert call(good, None, which=which)[0] == abi.SA_ERR_BAD_ARG
        assert call(good, host_rows(), sc=None, which=which)[0] == abi.SA_ERR_BAD_ARG
        for over in (dict(struct_size=28), dict(points=0, n_sigmas=0), dict(n_sigmas=16), dict(min_common=0), dict(sigmas=None)):
            s2, bad = opts(**over)
            assert call(bad, host_rows(), which=which)[0] == abi.SA_ERR_BAD_ARG, over
        for v in (0.0, -1.0, np.inf, np.nan):
            s3 = OR.sigmas_for(P).copy()
            s3[11] = v
            s4, bad = N.options(lib, s3)
            rc, text = call(bad, host_rows(), which=which)
            assert rc == abi.SA_ERR_BAD_ARG and "sigmas[11]" in text
        for over in (dict(struct_size=36), dict(comps=4), dict(host=None)):
            assert call(good, host_rows(**over), which=which)[0] == abi.SA_ERR_BAD_ARG, over
        # the descriptor's checks: a span outside every registered block, an index beyond n_rows
        dev = DeviceRows(0x10000, m, P * 2, SA_ELEM_F32)
        st = dev.struct()
        assert call(good, host_rows(host=None, dev=C.pointer(st)), which=which)[0] == abi.SA_ERR_BAD_ARG
        both = host_rows(dev=C.pointer(st))
        assert call(good, both, which=which)[0] == abi.SA_ERR_BAD_ARG
    # null outputs
    assert lib.sa_pose_nms(eng.h, C.byref(good), m, C.byref(host_rows()), scores.ctypes.data_as(N.F32_P), None, C.byref(cnt)) == abi.SA_ERR_BAD_ARG
    assert lib.sa_pose_nms_matrix(eng.h, C.byref(good), m, C.byref(host_rows()), scores.ctypes.data_as(N.F32_P), None, None, C.byref(cnt)) == abi.SA_ERR_BAD_ARG
    assert cnt.value == 77
    with device_block(eng, np.zeros((m, P * 2), f32)) as ptr:
        dev = DeviceRows(ptr, m, P * 2, SA_ELEM_F32, np.array([0, 1, 2, 3, 4, m], u32))
        st = dev.struct()
        rc, text = call(good, host_rows(host=None, dev=C.pointer(st)))
        assert rc == abi.SA_ERR_BAD_ARG and "index[5]" in text
    # a batch names the scene: 16385 survivors in scene 1
    big = np.array([3, 16385], u32)
    zp, zs = np.zeros((int(big.sum()), 3, 2), f32), np.full(int(big.sum()), 0.5, f32)
    s5, o3 = N.options(lib, OR.sigmas_for(3))
    bk = np.full(int(big.sum()), 77, u32)
    outs = (N.U32_P * 2)(bk.ctypes.data_as(N.U32_P), bk[3:].ctypes.data_as(N.U32_P))
    on = np.full(2, 77, u32)
    r3 = sa_point_rows(C.sizeof(sa_point_rows), 2, 0.0, 0, zp.ctypes.data_as(N.F32_P), None, None)
    rc = lib.sa_pose_nms_batch(eng.h, C.byref(o3), 2, big.ctypes.data_as(N.U32_P), C.byref(r3), zs.ctypes.data_as(N.F32_P), outs, on.ctypes.data_as(N.U32_P))
    assert rc == abi.SA_ERR_UNSUPPORTED and b"scene 1" in lib.sa_last_error(eng.h) and (on == 77).all() and (bk == 77).all()
    # more than 65535 scenes
    many = np.zeros(65536, u32)
    outs = (N.U32_P * 65536)()
    on = np.full(65536, 77, u32)
    rc = lib.sa_pose_nms_batch(eng.h, C.byref(good), 65536, many.ctypes.data_as(N.U32_P), None, None, outs, on.ctypes.data_as(N.U32_P))
    assert rc == abi.SA_ERR_UNSUPPORTED and (on == 77).all() and N.last(eng) == ZERO_STATS
    # the tap beyond its cap
    n = N.SA_POSE_NMS_TAP_MAX + 1
    zp, zs = np.zeros((n, 3, 2), f32), np.full(n, 0.5, f32)
    r4 = sa_point_rows(C.sizeof(sa_point_rows), 2, 0.0, 0, zp.ctypes.data_as(N.F32_P), None, None)
    rc = lib.sa_pose_nms_matrix(eng.h, C.byref(o3), n, C.byref(r4), zs.ctypes.data_as(N.F32_P), order.ctypes.data_as(N.U32_P), w.ctypes.data_as(N.F32_P),
                                C.byref(cnt))
    assert rc == abi.SA_ERR_UNSUPPORTED and cnt.value == 77 and (order == 77).all() and (w == 77).all() and N.last(eng) == ZERO_STATS
    with pytest.raises(EngineError) as err:   # and the Python face raises what the library answers
        N.pose_nms(eng, pts, scores, OR.sigmas_for(P), min_common=0)
    assert err.value.code == abi.SA_ERR_BAD_ARG


# ---- 7. with the tracker ---------------------------------------------------------------------------------------------------------
def test_the_tracker_behind_it_keeps_one_track_per_person(eng):
    """Two frames of 7 people, each seen as 2 to 4 jittered skeletons.  KeypointSort on the network's rows composed with the kept
    indices returns, and leaves in its bank, what a twin fed the host-filtered poses does: 7 tracks; without the NMS there are more."""
    P, people = 17, 7
    sig = OR.sigmas_for(P)
    pts0, scores0, who = NR.crowd(70, people, 21, P, jitter=0.01, spread=2000.0)
    assert len(set(who.tolist())) == people
    frames = [(pts0, scores0), ((pts0 + f32(0.01)).astype(f32), np.roll(scores0, 5))]   # the same people, a step on, other scores
    with KeypointSort(eng, P) as dev, KeypointSort(eng, P) as twin, KeypointSort(eng, P) as raw:
        for f, (pts, scores) in enumerate(frames):
            block = np.zeros((len(pts), P * 2 + 6), f32)
            block[:, 4: 4 + P * 2] = pts.reshape(len(pts), -1)
            with device_block(eng, block) as ptr:
                rows = DeviceRows(ptr + 4 * 4, len(pts), P * 2 + 6, SA_ELEM_F32)
                keep = N.pose_nms(eng, None, scores, sig, nms_threshold=0.5, rows=rows)
                assert N.last(eng)["bytes_h2d"] == 24 + 4 * len(pts) + 4 * P
                assert keep.tolist() == NR.nms(pts, scores, sig, 0.5).tolist() and len(keep) == people
                a = dev.predict([1], rows=N.keep_rows(rows, keep), pose_counts=[len(keep)])[1]
            b = twin.predict({1: pts[keep]})[1]
            c = raw.predict({1: pts})[1]
            for k in ("id", "scene", "epoch", "length", "created"):
                assert a[k].tolist() == b[k].tolist(), k
            assert bits(a["weight"], b["weight"])
            if f == 0:   # the reason for the feature: one track per person, three without the NMS
                assert int(a["created"].sum()) == people == dev.active() and int(c["created"].sum()) == 21 == raw.active()
        assert dev.active() == twin.active() < raw.active()
        bd, bt = dev.bank(), twin.bank()
        assert bd.order().tolist() == bt.order().tolist()
        for t in bd.order():
            (h1, m1, c1), (h2, m2, c2) = bd.state(t), bt.state(t)
            assert (h1 == h2).all() and bits(m1, m2) and bits(c1, c2)


# ---- 8. the box path beside it ---------------------------------------------------------------------------------------------------
def test_box_nms_is_what_it_was_around_a_pose_call(eng):
    rng = np.random.default_rng(8)
    boxes = np.zeros(40, abi.BOX_DTYPE)
    boxes["xc"], boxes["yc"] = rng.uniform(0, 60, 40), rng.uniform(0, 60, 40)
    boxes["aspect"], boxes["height"], boxes["confidence"] = rng.uniform(0.5, 1.5, 40), rng.uniform(8, 20, 40), 1.0
    sc = rng.uniform(0.1, 1, 40).astype(f32)
    before = eng.nms(boxes, sc, 0.3, 0.2)
    pts, scores, mask = scene(65, 17)
    N.pose_nms(eng, pts, scores, nms_threshold=NMS_THR, **kw(17, 1, mask))
    after = eng.nms(boxes, sc, 0.3, 0.2)
    assert before.tolist() == after.tolist() and 0 < len(before) < 40
