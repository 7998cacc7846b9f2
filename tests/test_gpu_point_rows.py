"""One presence rule behind every keypoint call on the MI355X: the same five poses go through the three consumers of
similari_amd/csrc/sa_point_rows.h — the bank's filter (PointBank.step), the vote (PoseBank.associate, its tap) and pose NMS
(pose_nms_matrix) — from four sources, and each consumer must show the presence table that the rule of include/similari_points.h
gives for that source: x and y finite, score >= min_score when comps == 3, the mask byte of the ITEM, no SA_ROW_NONE.

Shapes: P = 3, five poses.  The narrowest input on which a mask indexed by row instead of by item, a wrong stride or element size, a
dropped SA_ROW_NONE or a comps-dependent offset shows: the indexed source names one row twice under two different mask rows.  Every value
is exact in f16 and in bf16, so the sources differ in nothing but where the points lie.  The tables and the references are computed once."""
import functools

import numpy as np
import pytest

import devrows_ref as dref
import oks_ref as OR
import points_ref as R
import pose_nms_ref as NR
import pose_ref as PR
from similari_amd import abi
from similari_amd import pose_nms as N
from similari_amd.devrows import DeviceRows
from similari_amd.engine import Engine
from similari_amd.f16 import SA_ELEM_BF16, SA_ELEM_F16
from similari_amd.points import SA_ROW_NONE, PointBank
from similari_amd.pose import PoseBank
from test_gpu_points import bits, device_block, to_source

f32, u8, u32, u64 = np.float32, np.uint8, np.uint32, np.uint64
P, M, MIN_SCORE, MIN_COMMON, NMS_COMMON = 3, 5, 0.5, 2, 1   # (min_common of the vote, of NMS)
NAN = np.nan
BASE = np.array([[4, 5], [12, 6], [8, 14]], f32)   # one person; every pose is it moved by eighths: 7 bits, exact in bf16 and f16
JITTER = np.array([[[0, 0], [1, -1], [2, 1]], [[1, 2], [-2, 1], [0, -3]], [[-1, 1], [3, 0], [1, 1]], [[2, -2], [1, 3], [-3, -1]], [[-2, -1], [0, 2], [3, 2]]], f32) / 8
POINT_SCORES = np.array([[.75, .75, .75], [.25, .75, .5], [.75, .75, .75], [.25, .75, .75], [.75, .75, .75]], f32)   # .25: below the floor, .5: at it
POSES = np.concatenate([BASE + JITTER, POINT_SCORES[..., None]], axis=2).astype(f32)
POSES[2, 2, 0] = NAN                                                           # one coordinate is missing
MASK = np.array([[1, 1, 1], [1, 1, 1], [1, 0, 1], [1, 0, 1], [1, 1, 0]], u8)   # by item
SCORES = np.array([0.5, 0.9, 0.7, 0.8, 0.6], f32)   # the NMS rank: 1, 3, 2, 4, 0
# three tracks, every point with a state, each a sixteenth or so off the person: a pair's weight tells which points went into it
TRACKS = (BASE + np.array([[[1, 0], [0, 1], [1, 1]], [[-1, 1], [1, -1], [0, 2]], [[0, -1], [2, 0], [-1, 0]]], f32) / 16).astype(f32)
T = len(TRACKS)
SOURCES = ["host_f32", "f16_strided_indexed", "bf16_plain", "host_comps2"]
OFF, PAD = 4, 7   # the indexed block: a column slice of wider rows


@functools.lru_cache(maxsize=None)
def source(name):
    """-> dict: comps, min_score as passed, the items' points z [M, P, comps] as the kernels must see them (NaN rows for SA_ROW_NONE),
    the table [M, P] and, per cause, the points it removes; for a device source the block's image, its shape and the index."""
    s = dict(comps=3, min_score=MIN_SCORE, image=None, index=None, z=POSES)
    if name == "f16_strided_indexed":
        # rows 1, 4, 5, 2 hold poses 1, 2, 4, 3; items 0 and 3 both name row 1, item 1 names none
        block = np.full((6, P * 3 + PAD), 7.0, f32)
        for row, pose in ((1, 1), (4, 2), (5, 4), (2, 3)):
            block[row, OFF: OFF + P * 3] = POSES[pose].reshape(-1)
        s.update(elem=SA_ELEM_F16, image=to_source(block, SA_ELEM_F16), index=np.array([1, SA_ROW_NONE, 4, 1, 5], u32))
        wide = dref.widen(s["image"], SA_ELEM_F16)[:, OFF: OFF + P * 3].reshape(6, P, 3)
        s["z"] = np.stack([np.full((P, 3), NAN, f32) if r == SA_ROW_NONE else wide[r] for r in s["index"]])
    elif name == "bf16_plain":
        s.update(elem=SA_ELEM_BF16, image=to_source(POSES.reshape(M, P * 3), SA_ELEM_BF16))
        s["z"] = dref.widen(s["image"], SA_ELEM_BF16).reshape(M, P, 3)
    elif name == "host_comps2":
        s.update(comps=2, min_score=0.9, z=np.ascontiguousarray(POSES[..., :2]))   # (a floor above every score: it must be ignored)
    z = s["z"]
    none = np.zeros((M, 1), bool) if s["index"] is None else (s["index"] == SA_ROW_NONE)[:, None]
    with np.errstate(invalid="ignore"):
        s["causes"] = dict(none=np.broadcast_to(none, (M, P)), nan=~(np.isfinite(z[..., 0]) & np.isfinite(z[..., 1])) & ~none,
                           score=~(z[..., 2] >= f32(MIN_SCORE)) & ~none if s["comps"] == 3 else np.zeros((M, P), bool), mask=MASK == 0)
    s["table"] = ~np.any(list(s["causes"].values()), axis=0)
    for a in (z, s["table"]):
        a.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def tracks_model():
    tracks = R.Bank((T, P))
    tracks.initiate(TRACKS, np.ones((T, P), bool))
    return tracks.has, tracks.mean, tracks.cov


@functools.lru_cache(maxsize=None)
def references(name):
    """-> (xy [M, P, 2] of the step on fresh tracks, w [M, T] of the vote's tap, (order, w [M, M]) of the NMS tap), all from the table"""
    s = source(name)
    z, table = s["z"], s["table"]
    z2 = np.where(table[..., None], z[..., :2], f32(0)).astype(f32)
    fresh = R.Bank((M, P))
    xy = fresh.step(z2, table)
    w = PR.weights(z2, table, *tracks_model(), R.PW, MIN_COMMON)
    order = NR.rank(SCORES)
    return xy, w, (order, NR.matrix(z[order], table[order], OR.sigmas_for(P), NMS_COMMON))


def check_not_vacuous(name):
    """Every cause that applies to the source removes a point that nothing else removes, and leaves one; the references show both."""
    s = source(name)
    causes, table = s["causes"], s["table"]
    applies = dict(none=s["index"] is not None, nan=True, score=s["comps"] == 3, mask=True)
    for c, on in applies.items():
        others = np.any([v for k, v in causes.items() if k != c], axis=0)
        assert bool((causes[c] & ~others).any()) == on, (name, c)
    assert table.any() and not table.all()
    assert table.tolist() == NR.present_of(s["z"], MASK, s["min_score"]).tolist() == R.present_of(s["z"], s["min_score"], MASK).tolist()
    xy, w, (order, wn) = references(name)
    assert (~np.isnan(xy[..., 0])).tolist() == table.tolist()
    assert np.isnan(w).all(axis=1).tolist() == (table.sum(axis=1) < MIN_COMMON).tolist() and not np.isnan(w).all() and np.isnan(w).any()
    assert np.isnan(w).any(axis=1).tolist() == np.isnan(w).all(axis=1).tolist()   # every track point has a state: a row is NaN or it is not
    assert order.tolist() == [1, 3, 2, 4, 0] and np.isfinite(wn[np.triu_indices(M, 1)]).any()
    # ... and both taps depend on the table: the finite points alone, without floor, mask and index, give other bits
    finite = np.isfinite(POSES[..., 0]) & np.isfinite(POSES[..., 1])
    assert not bits(w, PR.weights(np.where(finite[..., None], POSES[..., :2], f32(0)), finite, np.ones((T, P), bool), *tracks_model()[1:], R.PW, MIN_COMMON))
    assert not bits(wn, NR.matrix(POSES[order], finite[order], OR.sigmas_for(P), NMS_COMMON))
    if name == "f16_strided_indexed":   # one row under two mask rows: by item the tables differ, by row they could not
        assert bits(s["z"][0], s["z"][3]) and table[0].tolist() != table[3].tolist()


@pytest.mark.parametrize("name", SOURCES)
def test_no_comparison_is_vacuous(name):
    check_not_vacuous(name)


@pytest.fixture(scope="module")
def eng():
    e = Engine(abi.make_config(positional="iou", positional_threshold=0.3, device=0))
    yield e
    e.close()


@pytest.fixture(scope="module")
def tracks(eng):
    b = PoseBank(eng, P)
    b.initiate(np.arange(11, 11 + T), TRACKS)
    yield b
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SOURCES)
def test_the_three_consumers_show_one_presence_table(eng, tracks, name):
    check_not_vacuous(name)
    s = source(name)
    table, comps = s["table"], s["comps"]
    xy, w, (order, wn) = references(name)

    def run(kw):
        # 1. the filter: on fresh tracks a point has a state afterwards iff it was present
        with PointBank(eng, P) as fresh:
            got = fresh.step(np.arange(1, M + 1, dtype=u64), present=MASK, min_score=s["min_score"], **kw)
            st = fresh.last()
        print(name, "step seen", (~np.isnan(got[..., 0])).astype(int).tolist(), "present", st["present"], "src_bytes", st["src_bytes"])
        assert (~np.isnan(got[..., 0])).tolist() == table.tolist() and st["present"] == int(table.sum())
        assert bits(got, xy)
        # 2. the vote: a pose has a pair with the fully present tracks iff MIN_COMMON of its points are present, and the pair's bits
        _, _, tap = tracks.associate(present=MASK, min_score=s["min_score"], min_common=MIN_COMMON, matrix=True, **kw)
        print(name, "vote tap", tap.tolist())
        assert np.isnan(tap).tolist() == np.broadcast_to((table.sum(axis=1) < MIN_COMMON)[:, None], (M, T)).tolist()
        assert bits(tap, w)
        # 3. pose NMS: the tap in rank order
        got_order, got_w = N.pose_nms_matrix(eng, kw.get("pts"), SCORES, sigmas=OR.sigmas_for(P), min_common=NMS_COMMON, present=MASK,
                                             min_score=s["min_score"], rows=kw.get("rows"), comps=comps)
        print(name, "nms tap", got_w.tolist())
        assert got_order.tolist() == order.tolist() and bits(got_w, wn)
        return st

    if s["image"] is None:
        run(dict(pts=s["z"]))
        return
    eb = 2
    with device_block(eng, s["image"]) as ptr:
        if s["index"] is None:
            rows = DeviceRows(ptr, M, P * comps, s["elem"])
            read = M
        else:
            rows = DeviceRows(ptr + OFF * eb, len(s["image"]), s["image"].shape[1], s["elem"], s["index"])
            read = int((s["index"] != SA_ROW_NONE).sum())
        st = run(dict(rows=rows, comps=comps))
        assert st["src_bytes"] == read * P * comps * eb
