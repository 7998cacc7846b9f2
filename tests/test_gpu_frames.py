"""Frame preprocessing for a whole batch (include/similari_frames.h): sa_own_areas_batch and sa_nms_batch against a loop of the
single calls on the same engine and against the oracle.  A single call is the plan of one scene on the same host path and the same
kernels, so the comparison with the oracle is the one that proves either.

own areas : scene s of a batch equals Engine.own_areas on scene s to 1e-6 (the gate tests/test_own_areas.py holds between two
            summation orders of the same arithmetic) and the oracle to the reference test's EPS; scenes never see each other; boxes
            the LDS-resident kernel gives up on take the spill path inside a batch.
nms       : exactly the single call's and the oracle's indices, in order, for every filtered size around the 64-box word, for mixed
            sweep classes in one call, with and without scores.
launches  : as many for 30 scenes as for 2; refusals leave every output untouched.
single    : sa_own_areas / sa_nms leave sa_frames_last alone, refuse in the words they always had, and equal the oracle at the sizes
            around one 64-box turn of a segment."""
import numpy as np
import pytest

import oracle_lib as O
from similari_amd import abi, frames, synth

pytestmark = pytest.mark.gpu
EPS = 1e-5
SENTINEL_F, SENTINEL_U = np.float32(-7.0), np.uint32(0xDEADBEEF)


@pytest.fixture(scope="module")
def eng():
    from similari_amd.engine import Engine

    e = Engine(abi.make_config())
    yield e
    e.close()


def bits_differ(a, b):
    return int((np.asarray(a, np.float32).view(np.uint32) != np.asarray(b, np.float32).view(np.uint32)).sum())


# ---- own areas -------------------------------------------------------------------------------------------------------------------
def check_own_batch(eng, scenes):
    got = frames.own_areas_batch(eng, scenes)
    st = frames.last_stats(eng)
    differ = 0
    for s, (b, g) in enumerate(zip(scenes, got)):
        assert len(g) == len(b)
        if not len(b):
            continue
        single = eng.own_areas(b)
        assert np.abs(g - O.own_area_shares(b)).max() < EPS, s
        assert np.abs(g - single).max() < 1e-6, s
        differ += bits_differ(g, single)
    assert st["scenes"] == len(scenes) and st["boxes"] == sum(len(b) for b in scenes)
    return got, st, differ


@pytest.mark.parametrize("oriented", [False, True])
def test_own_areas_batch_equals_the_single_calls(eng, oriented):
    rng = np.random.default_rng(40 + oriented)
    scenes = [synth.dense_boxes(rng, n, (900.0, 600.0), oriented=oriented) for n in (0, 1, 3, 64, 65, 130)]
    assert (O.own_area_shares(scenes[-1]) < 0.999).mean() > 0.5, "most boxes must overlap something"
    for order in (scenes, scenes[::-1]):   # the empty scene once first, once last
        _, st, differ = check_own_batch(eng, order)
        print("shares that differ from the single call in any bit:", differ, "of", st["boxes"])
        assert st["launches"] == 1 and st["host_waits"] == 1 and st["spilled"] == 0
        assert st["bytes_d2h"] == 4 * (st["boxes"] + len(order)) and st["device_ms"] > 0.0


def test_own_areas_scenes_do_not_see_each_other(eng):
    one = abi.ltwh([10.0], [20.0], [30.0], [40.0])
    alone = eng.own_areas(one)
    assert alone[0] > 0.999
    assert eng.own_areas(np.concatenate([one, one])).max() < EPS   # (together they own nothing: the input can tell)
    got = frames.own_areas_batch(eng, [one, one])
    assert got[0][0] == alone[0] and got[1][0] == alone[0]
    # two scenes whose boxes interleave in coordinates: a row of overlapping boxes dealt out alternately
    row = abi.ltwh(list(np.arange(40) * 3.0), [0.0] * 40, [10.0] * 40, [10.0] * 40)
    a, b = row[0::2], row[1::2]
    got = frames.own_areas_batch(eng, [a, b])
    assert np.abs(got[0] - eng.own_areas(a)).max() < 1e-6 and np.abs(got[1] - eng.own_areas(b)).max() < 1e-6
    assert np.abs(got[0][1:-1] - 0.2).max() < 1e-4 and np.abs(eng.own_areas(row)[1:-1] - 0.0).max() < 1e-4   # 2 of 10 free | 4 + 4 covered twice over


def test_own_areas_spill_inside_a_batch(eng):
    """Scene A: 200 identical boxes — each overlaps 199 others, more than the 127 the LDS-resident kernel holds: all 200 spill.
    Scene B: a bar cut by 40 posts — 40 disjoint covered stretches on one edge of the bar, more than 24: the bar spills, the posts
    (one neighbour each) do not.  Scene C: 65 ordinary boxes."""
    rng = np.random.default_rng(5)
    A = np.repeat(abi.ltwh([0.0], [0.0], [10.0], [10.0]), 200)
    B = np.concatenate([abi.ltwh([-1.0], [4.0], [125.0], [2.0]), abi.ltwh(list(np.arange(40) * 3.0), [0.0] * 40, [1.0] * 40, [10.0] * 40)])
    Cs = synth.dense_boxes(rng, 65, (1920.0, 1080.0), oriented=True)
    got = frames.own_areas_batch(eng, [A, B, Cs])
    st = frames.last_stats(eng)
    for b, g in zip((A, B, Cs), got):
        assert np.abs(g - O.own_area_shares(b)).max() < EPS
    assert got[0].max() < EPS and abs(float(got[1][0]) - (125.0 - 40.0) / 125.0) < 1e-4
    assert np.abs(got[2] - eng.own_areas(Cs)).max() < 1e-6
    assert st["spilled"] == 200 + 1
    assert st["host_waits"] == 2 and st["launches"] == 1 + -(-201 // 64)


# ---- NMS -------------------------------------------------------------------------------------------------------------------------
def dup_scene(rng, n, oriented):
    """n boxes: about two thirds at random and near-duplicates of half of them, as a detector emits them."""
    m = max(1, (2 * n + 2) // 3)
    b = synth.dense_boxes(rng, m, (1200.0, 800.0), oriented=oriented)
    dup = synth.jitter_boxes(rng, b[: n - m], 3.0, size_rel=0.05, angle_sigma=0.05 if oriented else 0.0)
    return np.concatenate([b, dup])[rng.permutation(n)]


def check_nms_batch(eng, scenes, scores, thr, sthr):
    got = frames.nms_batch(eng, scenes, scores, thr, sthr)
    for s, b in enumerate(scenes):
        sc = None if scores is None else scores[s]
        np.testing.assert_array_equal(got[s], O.nms(b, sc, thr, sthr), err_msg=f"scene {s} against the oracle")
        np.testing.assert_array_equal(got[s], eng.nms(b, sc, thr, sthr), err_msg=f"scene {s} against the single call")
    return got


@pytest.mark.parametrize("oriented", [False, True])
@pytest.mark.parametrize("with_scores", [False, True])
def test_nms_batch_equals_the_single_calls(eng, oriented, with_scores):
    rng = np.random.default_rng(300 + 2 * oriented + with_scores)
    sizes = [1, 63, 64, 65, 129]
    scenes, scores = [np.zeros(0, abi.BOX_DTYPE)], [None]
    for k in sizes:
        if not with_scores:   # every box passes: the filtered size is k
            scenes.append(dup_scene(rng, k, oriented))
            scores.append(None)
            continue
        # k boxes above the score threshold of 0.2 (every seventh without a score: it passes and ranks by height) and some below it
        low = k // 3 + 1
        b = dup_scene(rng, k + low, oriented)
        s = rng.uniform(0.25, 1.0, k + low).astype(np.float32)
        s[::7] = np.nan
        s[rng.permutation(np.nonzero(~np.isnan(s))[0])[:low]] = 0.1
        assert (np.isnan(s) | (s > 0.2)).sum() == k
        scenes.append(b)
        scores.append(s)
    if with_scores:   # every score below the threshold: nothing of the scene reaches the device
        scenes.append(dup_scene(rng, 40, oriented))
        scores.append(np.full(40, 0.1, np.float32))
        scenes.append(dup_scene(rng, 20, oriented))   # (a scene without scores among scenes with them: all of it passes)
        scores.append(None)
    suppressed = 0
    for thr, sthr in ((0.5, None), (0.3, 0.2), (-1.0, None)):
        got = check_nms_batch(eng, scenes, scores if with_scores else None, thr, sthr)
        st = frames.last_stats(eng)
        assert st["launches"] == 2 and st["host_waits"] == 1 and st["scenes"] == len(scenes)
        if with_scores and sthr == 0.2:
            assert st["boxes"] == sum(sizes) + 20 and len(got[-2]) == 0
        if sthr is None and thr == 0.5:
            assert st["boxes"] == sum(len(b) for b in scenes)
            suppressed = st["boxes"] - sum(len(g) for g in got)
    assert suppressed > 20, "the duplicates must be suppressed"


NMS_BLOCK = 4096


def chain_scene_4097(oriented):
    """The 4097-box chain scene of tests/test_nms.py without scores (all heights equal: the input order is the rank order): a sparse
    grid of base boxes, near-duplicates of a sixteenth of them at random ranks, a chain of three equal boxes A, B, C inside the first
    4096-rank block (B shifted by 0.4 of the width, C by 0.8: A removes B, and B — removed — must not remove C), and a pair whose B
    holds rank 4096, the one rank the sweep keeps in a second word of its removed-bitmap.  -> boxes, [(ranks, must be kept)]"""
    n = 4097
    rng = np.random.default_rng(7 * n + 2 * oriented)
    pair = (int(rng.integers(0, NMS_BLOCK)), NMS_BLOCK)
    free = np.ones(n, bool)
    free[list(pair)] = False
    triple = sorted(int(r) for r in rng.choice(np.nonzero(free[:NMS_BLOCK])[0], 3, replace=False))
    free[triple] = False
    chains = [(pair, (-0.4, 0.0), [True, False]), (tuple(triple), (-0.4, 0.0, 0.4), [True, False, True])]
    n_dup = n // 16
    n_base = n - 5 - n_dup
    rest = rng.permutation(np.nonzero(free)[0])
    base_ranks, dup_ranks = rest[:n_base], rest[n_base:]
    cells = n_base + len(chains)
    side = int(np.ceil(np.sqrt(cells)))
    cell = rng.permutation(side * side)[:cells]
    cx, cy = (cell % side) * 100.0 + 50.0, (cell // side) * 100.0 + 50.0
    xc, yc, asp, ang = (np.zeros(n, np.float32) for _ in range(4))
    hgt = np.full(n, 24.0, np.float32)
    xc[base_ranks], yc[base_ranks] = cx[:n_base], cy[:n_base]
    asp[base_ranks] = rng.uniform(0.5, 1.5, n_base)
    ang[base_ranks] = rng.uniform(-3.0, 3.0, n_base)
    src = base_ranks[rng.choice(n_base, n_dup, replace=False)]
    xc[dup_ranks], yc[dup_ranks] = xc[src] + rng.normal(0, 3.0, n_dup), yc[src] + rng.normal(0, 3.0, n_dup)
    asp[dup_ranks], ang[dup_ranks] = asp[src] * rng.uniform(0.95, 1.05, n_dup), ang[src] + (rng.normal(0, 0.05, n_dup) if oriented else 0.0)
    for k, (ranks, shifts, _) in enumerate(chains):
        a, th = rng.uniform(0.8, 1.5), (rng.uniform(-3.0, 3.0) if oriented else 0.0)
        for r, shift in zip(ranks, shifts):
            xc[r] = cx[n_base + k] + shift * a * 24.0 * np.cos(th)
            yc[r] = cy[n_base + k] + shift * a * 24.0 * np.sin(th)
            asp[r], ang[r] = a, th
    return abi.make_boxes(xc, yc, asp, hgt, angle=ang if oriented else None), [(r, k) for r, _, k in chains]


@pytest.mark.parametrize("oriented", [False, True])
def test_nms_mixed_sweep_classes_in_one_call(eng, oriented):
    """4097 boxes need two words of removed-bitmap per lane, 17 and 200 boxes one: the call runs k_nms_sweep<2> for all three."""
    rng = np.random.default_rng(77 + oriented)
    big, chains = chain_scene_4097(oriented)
    scenes = [dup_scene(rng, 17, oriented), big, dup_scene(rng, 200, oriented)]
    got = check_nms_batch(eng, scenes, None, 0.5, None)
    assert frames.last_stats(eng)["launches"] == 2
    kept = np.zeros(len(big), bool)
    kept[got[1]] = True
    for ranks, want in chains:
        assert kept[list(ranks)].tolist() == want, ranks
    assert len(big) - len(got[1]) > len(big) // 64
    check_nms_batch(eng, scenes[::-1], None, 0.5, None)


def test_nms_scenes_do_not_see_each_other(eng):
    two = abi.make_boxes([0.0, 0.0], [0.0, 0.0], [1.0, 1.0], [5.0, 5.0])
    assert eng.nms(np.concatenate([two, two]), None, 0.5, None).tolist() == [0]
    got = frames.nms_batch(eng, [two, two], None, 0.5, None)
    assert [g.tolist() for g in got] == [[0], [0]]


# ---- launches and refusals -------------------------------------------------------------------------------------------------------
def test_launches_do_not_depend_on_the_scene_count(eng):
    rng = np.random.default_rng(9)
    scenes = [dup_scene(rng, 17, bool(s & 1)) for s in range(30)]
    seen = {}
    for n in (2, 30):
        _, own, _ = check_own_batch(eng, scenes[:n])
        check_nms_batch(eng, scenes[:n], None, 0.5, None)
        nms = frames.last_stats(eng)
        assert own["scenes"] == nms["scenes"] == n
        seen[n] = [(st["launches"], st["host_waits"]) for st in (own, nms)]
    assert seen[2] == seen[30] == [(1, 1), (2, 1)]


def zero_stats(eng):
    st = frames.last_stats(eng)
    return all(v == 0 for v in st.values())


def test_refusals_leave_the_outputs_untouched(eng):
    from similari_amd.engine import EngineError

    rng = np.random.default_rng(3)
    small = [dup_scene(rng, n, False) for n in (5, 0, 9)]
    # NMS: 16385 boxes of one scene pass the filter
    g = np.arange(16385)
    huge = abi.make_boxes((g % 129) * 100.0, (g // 129) * 100.0, np.full(len(g), 1.0), np.full(len(g), 24.0))
    scenes = small[:2] + [huge] + small[2:]
    out = [np.full(len(b), SENTINEL_U, np.uint32) for b in scenes]
    out_n = np.full(len(scenes), SENTINEL_U, np.uint32)
    frames.nms_batch(eng, small, None, 0.5, None)
    assert not zero_stats(eng)
    with pytest.raises(EngineError) as err:
        frames.nms_batch(eng, scenes, None, 0.5, None, out=out, out_n=out_n)
    assert err.value.code == abi.SA_ERR_UNSUPPORTED and "scene 2" in str(err.value) and "at most 16384 boxes" in str(err.value)
    assert all((o == SENTINEL_U).all() for o in out) and (out_n == SENTINEL_U).all() and zero_stats(eng)
    # ... and with that scene's last box under a score threshold the call goes through (k_nms_sweep<4> at the ceiling)
    sc = [None, None, np.concatenate([np.full(16384, 0.9, np.float32), [0.1]]).astype(np.float32), None]
    got = frames.nms_batch(eng, scenes, sc, 0.5, 0.5)
    assert len(got[2]) == 16384 and frames.last_stats(eng)["boxes"] == 16384 + 5 + 9
    # own areas: a box without height in scene 2
    bad = [b.copy() for b in small]
    bad[2]["height"][4] = 0.0
    shares = [np.full(len(b), SENTINEL_F, np.float32) for b in bad]
    with pytest.raises(EngineError) as err:
        frames.own_areas_batch(eng, bad, out=shares)
    assert err.value.code == abi.SA_ERR_BAD_ARG and "scene 2" in str(err.value) and "boxes[4]" in str(err.value)
    assert all((o == SENTINEL_F).all() for o in shares) and zero_stats(eng)
    # more than 65535 scenes
    empty = [np.zeros(0, abi.BOX_DTYPE)] * 65536
    for call in (lambda: frames.own_areas_batch(eng, empty), lambda: frames.nms_batch(eng, empty, None, 0.5, None)):
        with pytest.raises(EngineError) as err:
            call()
        assert err.value.code == abi.SA_ERR_UNSUPPORTED and "65535 scenes" in str(err.value)
    got = frames.own_areas_batch(eng, empty[:65535])   # (65535 empty scenes are legal)
    assert len(got) == 65535 and not any(len(g) for g in got)
    assert frames.last_stats(eng)["scenes"] == 65535
    assert frames.own_areas_batch(eng, []) == [] and frames.nms_batch(eng, [], None, 0.5, None) == []


# ---- the single calls: the plan of one scene ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["own", "nms"])
def test_single_calls_leave_the_batch_stats_alone(eng, first):
    """sa_frames_last is the last *_batch call: sa_own_areas and sa_nms run the same path and write nothing there."""
    rng = np.random.default_rng(12)
    scenes = [dup_scene(rng, n, False) for n in (3, 65)]
    if first == "own":
        frames.own_areas_batch(eng, scenes)
    else:
        frames.nms_batch(eng, scenes, None, 0.5, None)
    before = frames.last_stats(eng)
    assert before["scenes"] == 2 and before["boxes"] == 68 and before["launches"] == (1 if first == "own" else 2) and before["device_ms"] > 0.0
    eng.own_areas(scenes[1])
    eng.nms(scenes[1], None, 0.5, None)
    assert frames.last_stats(eng) == before


def refused(eng, rc):
    msg = eng.lib.sa_last_error(eng.h)
    return rc, msg.decode() if msg else ""


def test_single_call_refusals_keep_their_words(eng):
    """The refusals of sa_nms and sa_own_areas that come before any launch, word for word — no scene is named —, through the ABI's own
    prototypes with the caller's arrays: they still hold their sentinels afterwards."""
    import ctypes as C

    F32_P, U32_P, BOX_P = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(abi.sa_box)
    L, h = eng.lib, eng.h
    nan = float("nan")
    four = np.ascontiguousarray(abi.ltwh([0.0, 20.0, 40.0, 60.0], [0.0] * 4, [10.0] * 4, [10.0] * 4), abi.BOX_DTYPE)
    share = np.full(4, SENTINEL_F, np.float32)
    keep = np.full(16385, SENTINEL_U, np.uint32)
    out_n = C.c_uint32(int(SENTINEL_U))
    box_p = lambda b: C.cast(b.ctypes.data, BOX_P)
    # null arguments, in the order the checks come in
    assert refused(eng, L.sa_nms(h, 4, box_p(four), None, 0.5, nan, keep.ctypes.data_as(U32_P), None)) == (abi.SA_ERR_BAD_ARG, "sa_nms: null argument")
    assert refused(eng, L.sa_nms(h, 4, None, None, 0.5, nan, keep.ctypes.data_as(U32_P), C.byref(out_n))) == (abi.SA_ERR_BAD_ARG, "sa_nms: null argument")
    assert refused(eng, L.sa_nms(h, 4, box_p(four), None, 0.5, nan, None, C.byref(out_n))) == (abi.SA_ERR_BAD_ARG, "sa_nms: null argument")
    assert out_n.value == int(SENTINEL_U)
    assert L.sa_nms(h, 0, None, None, 0.5, nan, None, C.byref(out_n)) == abi.SA_OK and out_n.value == 0   # no boxes: nothing is read
    assert refused(eng, L.sa_own_areas(h, 4, None, share.ctypes.data_as(F32_P))) == (abi.SA_ERR_BAD_ARG, "sa_own_areas: null argument")
    assert refused(eng, L.sa_own_areas(h, 4, box_p(four), None)) == (abi.SA_ERR_BAD_ARG, "sa_own_areas: null argument")
    assert L.sa_own_areas(h, 0, None, None) == abi.SA_OK
    # a box without height at index 2 of 4, a confidence beyond 1 at index 3: check_box's own words
    bad = four.copy()
    bad["height"][2] = 0.0
    assert refused(eng, L.sa_own_areas(h, 4, box_p(bad), share.ctypes.data_as(F32_P))) == (
        abi.SA_ERR_BAD_ARG, "boxes[2]: aspect and height must be > 0 (bbox.rs:453-456)")
    bad = four.copy()
    bad["confidence"][3] = 1.5
    assert refused(eng, L.sa_own_areas(h, 4, box_p(bad), share.ctypes.data_as(F32_P))) == (
        abi.SA_ERR_BAD_ARG, "boxes[3]: confidence must lie in [0, 1] (bbox.rs:123-126)")
    assert (share == SENTINEL_F).all()
    # 16385 boxes pass the filter
    g = np.arange(16385)
    huge = np.ascontiguousarray(abi.make_boxes((g % 129) * 100.0, (g // 129) * 100.0, np.full(len(g), 1.0), np.full(len(g), 24.0)), abi.BOX_DTYPE)
    out_n = C.c_uint32(int(SENTINEL_U))
    assert refused(eng, L.sa_nms(h, len(huge), box_p(huge), None, 0.5, nan, keep.ctypes.data_as(U32_P), C.byref(out_n))) == (
        abi.SA_ERR_UNSUPPORTED, "sa_nms: at most 16384 boxes pass to the pair stage (got 16385)")
    assert (keep == SENTINEL_U).all() and out_n.value == 0   # (*out_n is zeroed before the boxes are looked at, as it always was)


def test_single_call_refuses_an_edge_cut_into_more_than_512_stretches(eng):
    """A bar cut by 520 posts: 520 disjoint covered stretches on one edge of the bar, more than the spill path's 512.  The one refusal
    of sa_own_areas that comes back from the device; the caller's array keeps its sentinels."""
    import ctypes as C

    posts = abi.ltwh(list(np.arange(520) * 3.0), [0.0] * 520, [1.0] * 520, [10.0] * 520)
    sc = np.ascontiguousarray(np.concatenate([abi.ltwh([-1.0], [4.0], [520 * 3.0], [2.0]), posts]), abi.BOX_DTYPE)
    share = np.full(len(sc), SENTINEL_F, np.float32)
    rc = eng.lib.sa_own_areas(eng.h, len(sc), C.cast(sc.ctypes.data, C.POINTER(abi.sa_box)), share.ctypes.data_as(C.POINTER(C.c_float)))
    assert refused(eng, rc) == (abi.SA_ERR_UNSUPPORTED, "sa_own_areas: more than 512 disjoint stretches of one box edge are covered by other boxes")
    assert (share == SENTINEL_F).all()
    from similari_amd.engine import EngineError

    with pytest.raises(EngineError) as err:
        frames.own_areas_batch(eng, [sc[:3], sc])
    assert err.value.code == abi.SA_ERR_UNSUPPORTED
    assert "sa_own_areas_batch: scene 1: more than 512 disjoint stretches of one box edge are covered by other boxes" in str(err.value)


@pytest.mark.parametrize("oriented", [False, True])
def test_single_own_areas_around_the_64_box_scan(eng, oriented):
    """sa_own_areas against the oracle at the sizes at which one segment's neighbour scan (64 boxes a turn) can go wrong and which
    tests/test_own_areas.py does not run: 3, 64 and 130 boxes (it runs 0, 1, 65 and 1000)."""
    rng = np.random.default_rng(60 + oriented)
    for n in (3, 64, 130):
        b = synth.dense_boxes(rng, n, (900.0, 600.0), oriented=oriented)
        got = eng.own_areas(b)
        assert len(got) == n and np.abs(got - O.own_area_shares(b)).max() < EPS, n


@pytest.mark.parametrize("oriented", [False, True])
@pytest.mark.parametrize("with_scores", [False, True])
def test_single_nms_around_the_64_box_word(eng, oriented, with_scores):
    """sa_nms against the oracle, index for index, at filtered sizes of 63, 64, 65 and 129 boxes — one word, the last box of it, the
    first of a second and of a third — which tests/test_nms.py does not run (1, 25, 300, 1500 and the chain scenes from 4096 on)."""
    rng = np.random.default_rng(500 + 2 * oriented + with_scores)
    for k in (63, 64, 65, 129):
        if with_scores:   # k boxes above the score threshold of 0.2 (every seventh without a score: it passes) and some below it
            low = k // 3 + 1
            b = dup_scene(rng, k + low, oriented)
            s = rng.uniform(0.25, 1.0, k + low).astype(np.float32)
            s[::7] = np.nan
            s[rng.permutation(np.nonzero(~np.isnan(s))[0])[:low]] = 0.1
            assert (np.isnan(s) | (s > 0.2)).sum() == k
        else:
            b, s = dup_scene(rng, k, oriented), None
        for thr, sthr in ((0.5, 0.2 if with_scores else None), (-1.0, 0.2 if with_scores else None)):
            np.testing.assert_array_equal(eng.nms(b, s, thr, sthr), O.nms(b, s, thr, sthr), err_msg=f"{k} boxes, threshold {thr}")
