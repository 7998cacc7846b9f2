"""A frame's feature rows read from device memory on the MI355X (similari_amd.framerows over include/similari_framerows.h).

The contract admits no tolerance: a *_dev call returns, and leaves in the engine's track tables, exactly the bits of the existing call
fed widen(x) as host f32 for every source element.  So every test runs a twin ON THE SAME ENGINE (the upkeep tests: on a twin engine /
tracker) — one frame fed from device memory, one fed tests/devrows_ref.widen of the same source from the host — and compares with
assert_array_equal on bit patterns.  Device memory comes from tests/hipmem.py, no torch; every block is unregistered and freed in a
finally.  T = 40 tracks, K = 1, cosine unless a test says otherwise; more than half of a frame's votes must be visual, so the rows
really were read."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import devrows_ref as ref
import hipmem
from similari_amd import abi, framerows as FR, synth, trackers as TR
from similari_amd.devrows import DeviceRows, sa_dev_rows
from similari_amd.engine import Engine, EngineError
from similari_amd.f16 import SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_F32

pytestmark = pytest.mark.gpu
u8, u16, u32, u64 = np.uint8, np.uint16, np.uint32, np.uint64
F32, BF16, F16 = SA_ELEM_F32, SA_ELEM_BF16, SA_ELEM_F16
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
EB = {F32: 4, BF16: 2, F16: 2}
NONE = FR.SA_ROW_NONE
T, N = 40, 70
SCENE = 5


def vcfg(d, kind="cosine", k=1, flags=abi.SA_FLAG_TAP, **kw):
    return abi.make_config(positional="iou", positional_threshold=0.3, visual=kind, visual_threshold=0.2 if kind == "cosine" else 0.6,
                           feature_len=d, max_observations=k, visual_min_votes=1, visual_minimal_track_length=1,
                           positional_min_confidence=0.1, max_idle_epochs=5, device=0, flags=flags, **kw)


def to_source(x, elem):
    """f32 values as they lie in device memory in `elem`: themselves, or the uint16 bit patterns of their f16 / bf16 roundings."""
    x = np.ascontiguousarray(x, np.float32)
    if elem == F32:
        return x
    if elem == F16:
        return x.astype(np.float16).view(u16)
    return (x.view(u32) >> 16).astype(u16)


def lay_rows(bits, stride, offset):
    """The image of a block that holds `bits` rows `stride` elements apart from element `offset` on and ENDS with the last row's last
    element; every element that is no row's is a NaN pattern."""
    n, D = bits.shape
    img = np.full(offset + (n - 1) * stride + D, 0x7FFF if bits.dtype == u16 else np.nan, bits.dtype)
    for r in range(n):
        img[offset + r * stride: offset + r * stride + D] = bits[r]
    return img


@contextlib.contextmanager
def device_block(engine, image, device=0):
    ptr = hipmem.malloc(image.nbytes)
    try:
        hipmem.upload(ptr, image)
        engine.register_device_block(ptr, image.nbytes, device)
        yield ptr
    finally:
        engine.unregister_device_block(ptr)
        hipmem.free(ptr)


def expected_wide(ptr, stride, elem, D, table):
    """The rule of DESIGN.md ("A frame's rows from device memory"): a row is read with 16-byte loads iff its address is a multiple of
    16 and D % 4 == 0."""
    return sum(1 for t in table if int(t) != NONE and D % 4 == 0 and (ptr + int(t) * stride * EB[elem]) % 16 == 0)


def bits32(a):
    return np.ascontiguousarray(a).view(u32 if a.dtype.itemsize == 4 else u64)


def taps(eng, slot=0):
    rw, ri, cw, ci, kind = eng.tap_votes(slot)
    return [bits32(eng.tap_visual(slot)), bits32(rw), ri, bits32(cw), ci, np.array([kind])]


def same(a, b, what=""):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x, y, err_msg="%s: output %d" % (what, i))


def upsert_scene(eng, scene, sc):
    eng.upsert(scene, abi.make_tracks(sc["track_ids"], sc["track_boxes"], sc["track_epochs"], feats=sc["track_feats"],
                                      feat_present=sc["track_present"]))


def host_frame(eng, scene, det):
    ids, votes = eng.associate(scene, 1, det)
    return [ids, votes] + taps(eng)


def dev_frame(eng, scene, det, rows):
    ids, votes = FR.associate_rows(eng, scene, 1, det, rows)
    return [ids, votes] + taps(eng)


# ---- 1. the widen kernel, every regime -------------------------------------------------------------
class Rig:
    """One engine per (D, metric) with the scene's 40 tracks in place, and the host-fed twin of every source once."""

    def __init__(self, d, kind):
        self.d, self.kind = d, kind
        self.eng = Engine(vcfg(d, kind))
        self.sc = synth.visual_scene(np.random.default_rng(1000 + d), T, N, d, 1, canvas=(1500.0, 900.0))
        upsert_scene(self.eng, SCENE, self.sc)
        self.twins = {}

    def source(self, elem):
        return to_source(self.sc["det_feats"], elem)

    def twin(self, elem, index):
        key = (elem, None if index is None else tuple(index))
        if key not in self.twins:
            w = ref.widen(self.source(elem), elem)
            w = w if index is None else w[index]
            det = abi.make_detections(self.sc["det_boxes"], feats=w, feat_quality=self.sc["det_quality"])
            self.twins[key] = host_frame(self.eng, SCENE, det)
        return self.twins[key]


@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(d, kind="cosine"):
        if (d, kind) not in made:
            made[(d, kind)] = Rig(d, kind)
        return made[(d, kind)]

    yield get
    for r in made.values():
        r.eng.close()


def run_regime(rig, elem, layout):
    d = rig.d
    bits = rig.source(elem)
    stride, offset, index = {"contiguous": (d, 0, None), "stride8": (d + 8, 0, None), "odd": (d + 1, 1, None),
                             "reversed": (d, 0, np.arange(N, dtype=u32)[::-1].copy())}[layout]
    if index is not None:
        index[0] = index[1]   # one row named twice
    img = lay_rows(bits, stride, offset)
    with device_block(rig.eng, img) as ptr:
        base = ptr + offset * EB[elem]
        assert ptr % 16 == 0
        rows = DeviceRows(base, N, stride, elem, index)
        det = abi.make_detections(rig.sc["det_boxes"], feat_quality=rig.sc["det_quality"])
        got = dev_frame(rig.eng, SCENE, det, rows)
        st = FR.framerows_stats(rig.eng)
    want = rig.twin(elem, index)
    same(got, want, "%s %s D=%d" % (NAME[elem], layout, d))
    assert (got[1] == abi.SA_VOTE_VISUAL).sum() > N // 2, "the rows were not read"
    table = np.arange(N) if index is None else index
    if elem == F32 and layout == "contiguous":   # today's pointer route: read in place, nothing widened
        assert st == {"launches": 0, "rows": 0, "wide_rows": 0, "src_bytes": 0}
    else:
        wide = expected_wide(base, stride, elem, d, table)
        assert st == {"launches": 1, "rows": N, "wide_rows": wide, "src_bytes": N * d * EB[elem]}, st
        if layout == "odd" and d % 4 == 0:   # wide and narrow rows alternate
            assert 0 < wide < N
        if d % 4:
            assert wide == 0


@pytest.mark.parametrize("layout", ["contiguous", "stride8", "odd", "reversed"])
@pytest.mark.parametrize("d", [512, 68, 33])
@pytest.mark.parametrize("elem", [F32, F16, BF16], ids=lambda e: NAME[e])
def test_widen_kernel_every_regime(rigs, elem, d, layout):
    """70 detections (18 workgroups of four rows) out of f32 / f16 / bf16 sources at D = 512 (no padding, wide loads), 68 (padded,
    D % 4 == 0, a 16-bit row ends in one 8-byte load) and 33 (element by element); contiguous, strided, strided by an odd count from
    a base one element past a 16-byte boundary, and through a reversed index that names one row twice.  ids, vote types, the visual
    distances and the vote words equal the host-fed frame's; sa_framerows_last counts the rows and the wide ones by address."""
    run_regime(rigs(d), elem, layout)


def test_widen_kernel_euclidean(rigs):
    run_regime(rigs(68, "euclidean"), F16, "stride8")


# ---- 2. edges ------------------------------------------------------------------------------------
def test_edges_one_detection_none_and_nobody_with_a_feature(rigs):
    rig = rigs(68)
    eng, sc = rig.eng, rig.sc
    bits = rig.source(F16)
    with device_block(eng, lay_rows(bits, 68, 0)) as ptr:
        rows = DeviceRows(ptr, N, 68, F16)
        # N = 1
        det1 = abi.make_detections(sc["det_boxes"][:1], feat_quality=sc["det_quality"][:1])
        host1 = abi.make_detections(sc["det_boxes"][:1], feats=ref.widen(bits[:1], F16), feat_quality=sc["det_quality"][:1])
        same(dev_frame(eng, SCENE, det1, rows), host_frame(eng, SCENE, host1), "N = 1")
        assert FR.framerows_stats(eng) == {"launches": 1, "rows": 1, "wide_rows": 1, "src_bytes": 136}
        # N = 0 with a descriptor: fine, nothing is launched
        det0 = abi.make_detections(sc["det_boxes"][:0])
        ids, votes = FR.associate_rows(eng, SCENE, 1, det0, rows)
        assert len(ids) == 0 and len(votes) == 0
        assert FR.framerows_stats(eng) == {"launches": 0, "rows": 0, "wide_rows": 0, "src_bytes": 0}
        # nobody has a feature: nothing is launched, the frame equals the host-fed one with the same presence
        pres = np.zeros(N, u8)
        deta = abi.make_detections(sc["det_boxes"], feat_present=pres, feat_quality=sc["det_quality"])
        hosta = abi.make_detections(sc["det_boxes"], feats=np.zeros((N, 68), np.float32), feat_present=pres, feat_quality=sc["det_quality"])
        got, want = dev_frame(eng, SCENE, deta, rows), host_frame(eng, SCENE, hosta)
        same(got, want, "nobody present")
        assert (got[1] == abi.SA_VOTE_VISUAL).sum() == 0
        assert FR.framerows_stats(eng) == {"launches": 0, "rows": 0, "wide_rows": 0, "src_bytes": 0}


# ---- 3. absence ----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [68, 512])
def test_absent_detections_by_either_flag(rigs, d):
    """A third of the detections has no feature — every other one of them by feat_present, the rest by SA_ROW_NONE; the index entries of
    those absent by feat_present are out of range, and never looked at.  The frame equals the host-fed one with the same presence
    (and zero rows for the absent)."""
    rig = rigs(d)
    eng, sc = rig.eng, rig.sc
    bits = rig.source(BF16)
    index = np.random.default_rng(3).permutation(N).astype(u32)
    pres_in = np.ones(N, u8)
    has = np.ones(N, bool)
    for j, i in enumerate(range(0, N, 3)):
        has[i] = False
        if j % 2:
            index[i] = NONE
        else:
            pres_in[i], index[i] = 0, 4000000000
    w = np.zeros((N, d), np.float32)
    w[has] = ref.widen(bits, BF16)[index[has]]
    with device_block(eng, lay_rows(bits, d + 2, 0)) as ptr:
        rows = DeviceRows(ptr, N, d + 2, BF16, index)
        det = abi.make_detections(sc["det_boxes"], feat_present=pres_in, feat_quality=sc["det_quality"])
        got = dev_frame(eng, SCENE, det, rows)
        st = FR.framerows_stats(eng)
    host = abi.make_detections(sc["det_boxes"], feats=w, feat_present=has.astype(u8), feat_quality=sc["det_quality"])
    same(got, host_frame(eng, SCENE, host), "absence")
    assert st["launches"] == 1 and st["rows"] == int(has.sum()) and st["src_bytes"] == int(has.sum()) * d * 2
    assert st["wide_rows"] == expected_wide(ptr, d + 2, BF16, d, index[has])
    assert (got[1][has] == abi.SA_VOTE_VISUAL).sum() > has.sum() // 2


# ---- 4. a set of eight scenes, mixed -------------------------------------------------------------
def test_a_mixed_set_of_eight_scenes_is_one_launch():
    d, B, W = 128, 256, 160
    rng = np.random.default_rng(44)
    eng = Engine(vcfg(d))
    blocks = []
    try:
        ns = [70, 33, 50, 41, 64, 70, 29, 57]
        scs = [synth.visual_scene(rng, T, n, d, 1, canvas=(1500.0, 900.0)) for n in ns]
        for k, sc in enumerate(scs):
            upsert_scene(eng, 10 + k, sc)
        # scenes 0-2: f16 rows of ONE shared [B, W] block (column slice from 8 on), each scene its own rows
        shared = np.full((B, W), 0x7FFF, u16)
        perm = rng.permutation(B).astype(u32)
        idx, off = [], 0
        for k in range(3):
            ix = perm[off:off + ns[k]]
            shared[ix, 8:8 + d] = to_source(scs[k]["det_feats"], F16)
            idx.append(ix)
            off += ns[k]
        p_sh = hipmem.malloc(shared.nbytes); blocks.append(p_sh)
        hipmem.upload(p_sh, shared); eng.register_device_block(p_sh, shared.nbytes, 0)
        widened = [ref.widen(to_source(scs[k]["det_feats"], F16), F16) for k in range(3)]
        rows = [DeviceRows(p_sh + 16, B, W, F16, idx[k]) for k in range(3)]
        # scene 3: bf16, strided
        b3 = to_source(scs[3]["det_feats"], BF16)
        img3 = lay_rows(b3, d + 3, 0)
        p3 = hipmem.malloc(img3.nbytes); blocks.append(p3)
        hipmem.upload(p3, img3); eng.register_device_block(p3, img3.nbytes, 0)
        widened.append(ref.widen(b3, BF16)); rows.append(DeviceRows(p3, ns[3], d + 3, BF16))
        # scene 4: f32 through a descriptor that qualifies for the in-place read; scene 5: the old pointer route
        for k in (4, 5):
            f = np.ascontiguousarray(scs[k]["det_feats"])
            p = hipmem.malloc(f.nbytes); blocks.append(p)
            hipmem.upload(p, f); eng.register_device_block(p, f.nbytes, 0)
            widened.append(f)
            rows.append(DeviceRows(p, ns[k], d, F32) if k == 4 else None)
        p5 = blocks[-1]
        # scenes 6, 7: host-fed
        widened += [scs[6]["det_feats"], scs[7]["det_feats"]]
        rows += [None, None]

        def det(k, how):
            kw = dict(feat_quality=scs[k]["det_quality"])
            if how == "host":
                kw["feats"] = widened[k]
            elif how == "pointer":
                kw["feats_device_ptr"] = p5
            return abi.make_detections(scs[k]["det_boxes"], **kw)

        def fetch_all():
            return [list(eng.batch_fetch(k, ns[k])) + taps(eng, k) for k in range(8)]

        eng.batch_begin()
        for k in range(8):
            if rows[k] is not None:
                assert FR.batch_add_rows(eng, 10 + k, 1, det(k, "rows"), rows[k]) == k
            else:
                assert eng.batch_add(10 + k, 1, det(k, "pointer" if k == 5 else "host")) == k
        eng.batch_run(); eng.batch_sync()
        got = fetch_all()
        st = FR.framerows_stats(eng)
        launches = eng.last_frame_launches()
        # the same staged set once more: nothing is uploaded or widened again, the bits are the same
        eng.batch_run(); eng.batch_sync()
        again = fetch_all()
        assert FR.framerows_stats(eng) == st and eng.last_frame_launches() == launches
        # the host-fed twin set
        eng.batch_begin()
        for k in range(8):
            eng.batch_add(10 + k, 1, det(k, "host"))
        eng.batch_run(); eng.batch_sync()
        want = fetch_all()
        assert eng.last_frame_launches() == launches   # the frame's own launches do not know where the rows came from
        for k in range(8):
            same(got[k], want[k], "scene %d" % k)
            same(again[k], want[k], "scene %d, second run" % k)
            assert (got[k][1] == abi.SA_VOTE_VISUAL).sum() > min(ns[k], T) // 2
        n_rows = sum(ns[:4])
        wide = sum(expected_wide(p_sh + 16, W, F16, d, idx[k]) for k in range(3)) + expected_wide(p3, d + 3, BF16, d, range(ns[3]))
        assert st == {"launches": 1, "rows": n_rows, "wide_rows": wide, "src_bytes": n_rows * d * 2}, st
    finally:
        eng.close()
        for p in blocks:
            eng.unregister_device_block(p)
            hipmem.free(p)


# ---- 5. upkeep -----------------------------------------------------------------------------------
def test_upkeep_banks_and_kalman_state_equal_the_host_fed_twin():
    """Two frames through sa_batch_run_apply on two engines, one fed f16 rows from device memory (out of order, strided), one fed
    widen(x) from the host.  The rows hold f16 subnormals, the largest finite f16 and +-0.  After each frame every track's state
    (Kalman mean and covariance, bank presence, qualities, bank rows) is bit-identical, and the bank rows of the tracks the first
    frame starts equal widen(x) bit for bit.  Non-finite values are left out: what a frame does with an inf or NaN feature is not
    pinned by the oracle."""
    d, k, n = 64, 2, 24
    rng = np.random.default_rng(55)
    a, b = Engine(vcfg(d, k=k, flags=0)), Engine(vcfg(d, k=k, flags=0))
    blocks = []
    u64p, boxp, fp, u8p = C.POINTER(C.c_uint64), C.POINTER(abi.sa_box), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    try:
        ident = synth.reid_identities(rng, n + 6, d)
        world = synth.dense_boxes(rng, n, (900.0, 700.0))
        first_rows = None
        for f in range(2):
            if f == 1:
                world = np.concatenate([synth.jitter_boxes(rng, world, 1.5), synth.dense_boxes(rng, 6, (900.0, 700.0))])
            m = len(world)
            x = synth.observe(rng, ident[:m]).astype(np.float16)
            x[1] = rng.uniform(-6e-5, 6e-5, d).astype(np.float16)      # f16 subnormals
            x[2, :4] = [0.0, -0.0, 65504.0, -65504.0]                  # +-0 and the largest finite f16
            x[3, ::2] = 65504.0
            bits = x.view(u16)
            q = rng.uniform(0.3, 1.0, m).astype(np.float32)
            perm = rng.permutation(m).astype(u32)                      # detection i reads block row perm[i]
            img = np.full((m, d + 5), 0x7FFF, u16)
            img[perm, :d] = bits
            p = hipmem.malloc(img.nbytes); blocks.append(p)
            hipmem.upload(p, img); a.register_device_block(p, img.nbytes, 0)
            w = ref.widen(bits, F16)
            if f == 0:
                first_rows = w
            base = np.array([1000 * f], u64)
            out = []
            for eng, fed in ((a, "rows"), (b, "host")):
                eng.batch_begin()
                if fed == "rows":
                    sl = FR.batch_add_rows(eng, SCENE, f + 1, abi.make_detections(world, feat_quality=q), DeviceRows(p, m, d + 5, F16, perm))
                else:
                    sl = eng.batch_add(SCENE, f + 1, abi.make_detections(world, feats=w, feat_quality=q))
                eng._chk(eng.lib.sa_batch_run_apply(eng.h, base.ctypes.data_as(u64p), 1))
                eng.batch_sync()
                ids, votes = eng.batch_fetch(sl, m)
                nid, pred = np.zeros(m, u64), np.zeros(m, abi.BOX_DTYPE)
                eng._chk(eng.lib.sa_tracks_apply_collect(eng.h, sl, nid.ctypes.data_as(u64p), C.cast(pred.ctypes.data, boxp)))
                out.append([ids, votes, nid, pred.view(u8)])
            same(out[0], out[1], "frame %d" % f)
            if f == 0:
                assert (out[0][0] == 0).all()
                assert FR.framerows_stats(a) == {"launches": 1, "rows": m, "wide_rows": expected_wide(p, d + 5, F16, d, perm), "src_bytes": m * d * 2}
            else:
                assert (out[0][1][:n] == abi.SA_VOTE_VISUAL).sum() > n // 2
            order = a.order(SCENE)
            np.testing.assert_array_equal(order, b.order(SCENE))
            assert len(order) >= m
            for tid in order:
                states = []
                for eng in (a, b):
                    mean, cov = np.zeros(10, np.float32), np.zeros(100, np.float32)
                    qq, pres, ft = np.zeros(k, np.float32), np.zeros(k, u8), np.zeros((k, d), np.float32)
                    eng._chk(eng.lib.sa_tracks_get_state(eng.h, SCENE, int(tid), mean.ctypes.data_as(fp), cov.ctypes.data_as(fp),
                                                         qq.ctypes.data_as(fp), pres.ctypes.data_as(u8p), ft.ctypes.data_as(fp)))
                    states.append([bits32(mean), bits32(cov), bits32(qq), pres, bits32(ft)])
                same(states[0], states[1], "frame %d track %d" % (f, tid))
                if f == 0:   # the track candidate i started (id = base + 1 + i) holds exactly widen(x[i]) in its first bank slot
                    i = int(tid) - 1
                    assert states[0][3][0] == 1
                    np.testing.assert_array_equal(states[0][4][0], bits32(first_rows[i]))
    finally:
        a.close()
        b.close()
        for p in blocks:
            a.unregister_device_block(p)
            hipmem.free(p)


# ---- 6. pipeline ---------------------------------------------------------------------------------
def test_pipelined_tickets_of_f16_rows(rigs):
    """Four request sets of f16 rows, three tickets in flight, then the fourth.  Every set also carries a host-fed scene large enough
    (300 x 128 floats) that the set is staged on the copy stream: the widen launch is then the upload's last launch and carries the
    hand-over event.  Each ticket equals the host-fed result."""
    d = 128
    rng = np.random.default_rng(66)
    eng = Engine(vcfg(d, flags=0))
    blocks = []
    try:
        big = synth.visual_scene(rng, T, 300, d, 1, canvas=(3000.0, 2000.0))
        upsert_scene(eng, 30, big)
        big_det = abi.make_detections(big["det_boxes"], feats=big["det_feats"], feat_quality=big["det_quality"])
        big_ids, big_votes = eng.associate(30, 1, big_det)
        sets, wants = [], []
        for f in range(4):
            sc = synth.visual_scene(rng, T, N - 9 * f, d, 1, canvas=(1500.0, 900.0))
            n = N - 9 * f
            upsert_scene(eng, 20 + f, sc)
            bits = to_source(sc["det_feats"], F16)
            index = rng.permutation(n).astype(u32)
            img = np.full((n, d + 8 * f), 0x7FFF, u16)
            img[index, :d] = bits
            p = hipmem.malloc(img.nbytes); blocks.append(p)
            hipmem.upload(p, img); eng.register_device_block(p, img.nbytes, 0)
            host = abi.make_detections(sc["det_boxes"], feats=ref.widen(bits, F16), feat_quality=sc["det_quality"])
            wants.append(eng.associate(20 + f, 1, host))
            dev = abi.make_detections(sc["det_boxes"], feat_quality=sc["det_quality"])
            sets.append(FR.make_requests_rows([(20 + f, 1, dev, DeviceRows(p, n, d + 8 * f, F16, index)), (30, 1, big_det, None)]))
        tks = [FR.pipe_submit_rows(eng, sets[f][0], sets[f][1]) for f in range(3)]
        for f in range(3):
            eng.pipe_wait(tks[f], sets[f][2])
        tk = FR.pipe_stage_rows(eng, sets[3][0], sets[3][1])
        eng.pipe_launch(tk)
        eng.pipe_wait(tk, sets[3][2])
        for f in range(4):
            (ids, votes), (bi, bv) = sets[f][3]
            same([ids, votes, bi, bv], [wants[f][0], wants[f][1], big_ids, big_votes], "ticket %d" % f)
            assert (votes == abi.SA_VOTE_VISUAL).sum() > min(N - 9 * f, T) // 2
    finally:
        eng.close()
        for p in blocks:
            eng.unregister_device_block(p)
            hipmem.free(p)


# ---- 7. refusals ---------------------------------------------------------------------------------
def test_every_refusal_leaves_the_set_as_it_was(rigs):
    """Each refusal of the header once: SA_ERR_BAD_ARG and a message, nothing staged — the same scene is then added to the same set the
    right way and the set returns the right result.  A block registered for device 1 is refused by an engine on device 0 on the host,
    by the registry's bookkeeping alone."""
    rig = rigs(68)
    eng, sc, d = rig.eng, rig.sc, 68
    bits = rig.source(F16)
    img = lay_rows(bits, d, 8)       # the rows begin 16 bytes into the block
    want = rig.twin(F16, None)[:2]
    det = abi.make_detections(sc["det_boxes"], feat_quality=sc["det_quality"])
    with_feats = abi.make_detections(sc["det_boxes"], feats=ref.widen(bits, F16), feat_quality=sc["det_quality"])
    ptr = hipmem.malloc(img.nbytes)
    try:
        hipmem.upload(ptr, img)
        eng.register_device_block(ptr, img.nbytes, 0)
        base = ptr + 16
        good = DeviceRows(base, N, d, F16)

        def st(**kw):
            s = good.struct()
            for k, v in kw.items():
                setattr(s, k, v)
            return s

        bad_index = np.arange(N, dtype=u32)
        bad_index[7] = N
        keep = DeviceRows(base, N, d, F16, bad_index)
        cases = [
            ("null rows", det, None, "null rows"),
            ("struct_size", det, st(struct_size=32), "struct_size"),
            ("elem", det, st(elem=7), "element type"),
            ("alignment", det, st(base=base + 1), "aligned"),
            ("row_stride", det, st(row_stride=d - 1), "row_stride"),
            ("n_rows 0", det, st(n_rows=0), "n_rows"),
            ("n_rows 2^32 - 1", det, st(n_rows=0xFFFFFFFF), "n_rows"),
            ("span", det, st(n_rows=N + 1), "registered"),
            ("span before the block", det, st(base=ptr - 2, n_rows=4), "registered"),
            ("index", det, keep.struct(), "index[7]"),
            ("no index, too few rows", det, st(n_rows=N - 1), "n_rows"),
            ("feats and rows", with_feats, good.struct(), "feats"),
        ]
        for name, dd, rows, word in cases:
            eng.batch_begin()
            with pytest.raises(EngineError) as ex:
                FR.batch_add_rows(eng, SCENE, 1, dd, rows)
            assert ex.value.code == abi.SA_ERR_BAD_ARG and word in str(ex.value), (name, str(ex.value))
            assert FR.batch_add_rows(eng, SCENE, 1, det, good) == 0, name    # nothing was staged: slot 0, and the scene is not "already part"
            eng.batch_run(); eng.batch_sync()
            same(list(eng.batch_fetch(0, N)), want, name)
        # the other entry points refuse the same way, and leave no ticket behind
        req, ra, res, outs = FR.make_requests_rows([(SCENE, 1, det, st(elem=7))])
        for call in (FR.associate_batch_rows, None):
            with pytest.raises(EngineError) as ex:
                FR.associate_batch_rows(eng, req, ra, res) if call else FR.pipe_submit_rows(eng, req, ra)
            assert ex.value.code == abi.SA_ERR_BAD_ARG and "element type" in str(ex.value)
        with pytest.raises(EngineError):
            FR.associate_rows(eng, SCENE, 1, det, None)
        req, ra, res, outs = FR.make_requests_rows([(SCENE, 1, det, good)])
        tk = FR.pipe_submit_rows(eng, req, ra)
        eng.pipe_wait(tk, res)
        same(list(outs[0]), want, "a ticket after the refusals")
        # a block registered for another device: refused on the host, without a device call
        eng.unregister_device_block(ptr)
        eng.register_device_block(ptr, img.nbytes, 1)
        eng.batch_begin()
        with pytest.raises(EngineError) as ex:
            FR.batch_add_rows(eng, SCENE, 1, det, good)
        assert ex.value.code == abi.SA_ERR_BAD_ARG and "device 1" in str(ex.value)
        eng.unregister_device_block(ptr)
        eng.register_device_block(ptr, img.nbytes, 0)
        assert FR.batch_add_rows(eng, SCENE, 1, det, good) == 0
        eng.batch_run(); eng.batch_sync()
        same(list(eng.batch_fetch(0, N)), want, "after the block of device 1")
        # an engine without a visual metric
        plain = Engine(abi.make_config(positional="iou", positional_threshold=0.3, device=0))
        try:
            plain.batch_begin()
            boxes_only = abi.make_detections(sc["det_boxes"])
            with pytest.raises(EngineError) as ex:
                FR.batch_add_rows(plain, SCENE, 1, boxes_only, good)
            assert ex.value.code == abi.SA_ERR_BAD_ARG and "visual" in str(ex.value)
            assert plain.batch_add(SCENE, 1, boxes_only) == 0
            plain.batch_run(); plain.batch_sync()
            assert len(plain.batch_fetch(0, N)[0]) == N
        finally:
            plain.close()
    finally:
        eng.unregister_device_block(ptr)
        hipmem.free(ptr)


# ---- 8. the facade -------------------------------------------------------------------------------
TRACK_DTYPE = np.dtype([("id", "<u8"), ("epoch", "<u8"), ("predicted", abi.BOX_DTYPE), ("observed", abi.BOX_DTYPE), ("scene_id", "<u8"),
                        ("length", "<u8"), ("voting_type", "<i4"), ("has_custom", "<i4"), ("custom", "<i8")])


def track_bits(tracks):
    """[SortTrack] -> every field as integers: ids, epochs, lengths, vote types, and the boxes' floats as bit patterns."""
    def box(b):
        a = np.array([b.xc, b.yc, -1.0 if b.angle is None else b.angle, b.aspect, b.height, b.confidence], np.float32).view(u32)
        return tuple(int(v) for v in a) + (b.angle is None,)
    return [(t.id, t.epoch, t.scene_id, t.length, t.voting_type, t.custom_object_id, box(t.predicted_bbox), box(t.observed_bbox)) for t in tracks]


def u2d(b):
    return [TR.Universal2DBox(float(r["xc"]), float(r["yc"]), None, float(r["aspect"]), float(r["height"]), float(r["confidence"])) for r in b]


def facade_opts():
    return (TR.VisualSortOptions().max_idle_epochs(3).kept_history_length(3).visual_metric(TR.VisualSortMetricType.cosine(0.5))
            .positional_metric(TR.PositionalMetricType.iou(0.3)).visual_minimal_track_length(1).visual_minimal_quality_use(0.3)
            .visual_minimal_quality_collect(0.4).visual_max_observations(3).visual_min_votes(1))


def facade_frame(rng, ident, world, d, f):
    """One frame's observations twice — with feature pointers to widen(x), and bare beside an f16 block image with its index (two
    SA_ROW_NONE) — and the image."""
    n = len(world)
    bits = to_source(synth.observe(rng, ident, 0.01), F16)
    w = ref.widen(bits, F16)
    index = rng.permutation(n).astype(u32)
    img = np.full((n, d + 24), 0x7FFF, u16)
    img[index, 16:16 + d] = bits
    absent = {(2 * f) % n, (2 * f + 11) % n}
    q = rng.uniform(0.2, 1.0, n)
    fed, bare = [], []
    for i, bx in enumerate(u2d(world)):
        cid = 100 + i if i % 4 == 0 else None
        fed.append(TR.VisualSortObservation(None if i in absent else np.ascontiguousarray(w[i]), float(q[i]), bx, cid))
        bare.append(TR.VisualSortObservation(None, float(q[i]), bx, cid))
    for i in absent:
        index[i] = NONE
    return fed, bare, img, index


def test_facade_visual_sort_with_rows():
    d, n = 128, 30
    rng = np.random.default_rng(88)
    g = TR.VisualSort(opts=facade_opts(), feature_len=d, device=0, device_upkeep=True)
    h = TR.VisualSort(opts=facade_opts(), feature_len=d, device=0, device_upkeep=True)
    blocks = []
    try:
        ident = synth.reid_identities(rng, n, d)
        world = synth.dense_boxes(rng, n, (900.0, 700.0))
        for f in range(6):
            world = synth.jitter_boxes(rng, world, 2.0)
            fed, bare, img, index = facade_frame(rng, ident, world, d, f)
            p = hipmem.malloc(img.nbytes); blocks.append(p)
            hipmem.upload(p, img)
            assert g.lib.sa_device_block_register(C.c_void_p(p), img.nbytes, 0) == 0
            got = FR.predict_rows(g, 0, bare, DeviceRows(p + 32, n, d + 24, F16, index))
            want = h.predict(fed)
            assert track_bits(got) == track_bits(want), "frame %d" % f
            if f:
                assert sum(1 for t in got if t.voting_type == abi.SA_VOTE_VISUAL) > n // 2
        for t in got:
            assert g.track_info(t.id) == h.track_info(t.id)
        assert sum(g.track_info(t.id)["visual_features_collected_count"] for t in got) > n
        # a feature pointer together with rows is refused
        with pytest.raises(TR.TrackerError) as ex:
            FR.predict_rows(g, 0, fed, DeviceRows(p + 32, n, d + 24, F16, index))
        assert "error -1:" in str(ex.value) and "feature" in str(ex.value)
    finally:
        g.close()
        h.close()
        for p in blocks:
            g.lib.sa_device_block_unregister(C.c_void_p(p))
            hipmem.free(p)


def test_facade_batch_visual_sort_with_rows():
    d, n = 128, 30
    rng = np.random.default_rng(89)
    g = TR.BatchVisualSort(opts=facade_opts(), feature_len=d, device=0, device_upkeep=True)
    h = TR.BatchVisualSort(opts=facade_opts(), feature_len=d, device=0, device_upkeep=True)
    blocks = []
    try:
        scenes = (3, 8)
        ident = {s: synth.reid_identities(rng, n, d) for s in scenes}
        world = {s: synth.dense_boxes(rng, n, (900.0, 700.0)) for s in scenes}
        for f in range(6):
            rq_fed, rq_bare, rows = TR.PredictionBatchRequest(), TR.PredictionBatchRequest(), {}
            for s in scenes:
                world[s] = synth.jitter_boxes(rng, world[s], 2.0)
                fed, bare, img, index = facade_frame(rng, ident[s], world[s], d, f)
                p = hipmem.malloc(img.nbytes); blocks.append(p)
                hipmem.upload(p, img)
                assert g.lib.sa_device_block_register(C.c_void_p(p), img.nbytes, 0) == 0
                rows[s] = DeviceRows(p + 32, n, d + 24, F16, index)
                for o1, o2 in zip(fed, bare):
                    rq_fed.add(s, o1)
                    rq_bare.add(s, o2)
            res = FR.predict_batch_rows(g, rq_bare, rows)
            got = dict(res.get() for _ in scenes)
            res.close()
            want = h.predict(rq_fed)
            for s in scenes:
                assert track_bits(got[s]) == track_bits(want[s]), "frame %d scene %d" % (f, s)
                if f:
                    assert sum(1 for t in got[s] if t.voting_type == abi.SA_VOTE_VISUAL) > n // 2
        for s in scenes:
            for t in got[s]:
                assert g.track_info(t.id) == h.track_info(t.id)
    finally:
        g.close()
        h.close()
        for p in blocks:
            g.lib.sa_device_block_unregister(C.c_void_p(p))
            hipmem.free(p)


def test_facade_host_upkeep_is_unsupported():
    d, n = 128, 4
    rng = np.random.default_rng(90)
    g = TR.VisualSort(opts=facade_opts(), feature_len=d, device=0, device_upkeep=False)
    try:
        bare = [TR.VisualSortObservation(None, 0.9, bx, None) for bx in u2d(synth.dense_boxes(rng, n, (900.0, 700.0)))]
        with pytest.raises(TR.TrackerError) as ex:
            FR.predict_rows(g, 0, bare, DeviceRows(0x7f0000000000, n, d, F16))
        assert "error %d:" % abi.SA_ERR_UNSUPPORTED in str(ex.value) and "device_upkeep" in str(ex.value)
        assert len(g.predict(bare)) == n   # the tracker is as it was
    finally:
        g.close()
