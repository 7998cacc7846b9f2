"""The frame planner (similari_amd/csrc/sa_plan.h) on its own (host-only): which vote form, preparation blocks, assignment tail and first
phase a frame runs, and whether it can go lazy / reports its leftover rows.  sa_frame_visual_ok is a stub here: it records what the planner
asks it and answers as each test says."""
import ctypes as C
import subprocess

import pytest

from similari_amd import abi

CSRC = __import__("pathlib").Path(__file__).resolve().parent.parent / "similari_amd" / "csrc"

SRC = r'''
#include "sa_plan.h"
struct Stub { int ok_class, ok_words, ok_plain, calls, eu_mfma, vote_words, class_words; };
static bool visual_ok(const void* c, bool eu_mfma, bool vote_words, bool class_words) {
  Stub* s = (Stub*)c;
  s->calls++; s->eu_mfma = eu_mfma; s->vote_words = vote_words; s->class_words = class_words;
  return class_words ? s->ok_class : vote_words ? s->ok_words : s->ok_plain;
}
extern "C" void plan(int pos, int vis, unsigned flags, unsigned K, unsigned caps, unsigned N, unsigned T, int feats, int backing_off,
                     Stub* stub, int* out) {
  const SaPlanInputs in{pos, vis, flags, K, N, T, (caps & 1) != 0, (caps & 2) != 0, (caps & 4) != 0, (caps & 8) != 0, feats != 0,
                        backing_off != 0, visual_ok, stub};
  const SaFramePlan p = sa_frame_plan(in);
  const int o[9] = {(int)p.vote, (int)p.prep, (int)p.tail, p.eu_mfma, p.partials, p.fused, p.lazy_possible, p.lazy, p.reports_left};
  for (int i = 0; i < 9; ++i) out[i] = o[i];
}
'''

RESOLVE, CELL, TILE, CLASS = range(4)                 # SaVote
NONE, ALL, ONLY, RESET = range(4)                     # SaPrep
SMALL, SMALL_TC2, SMALL2, SMALL2_1X4, GENERAL = range(5)   # SaTail
FIELDS = ("vote", "prep", "tail", "eu_mfma", "partials", "fused", "lazy_possible", "lazy", "reports_left")
VIS = {"none": abi.SA_VIS_NONE, "cosine": abi.SA_VIS_COSINE, "euclidean": abi.SA_VIS_EUCLIDEAN}
POS = {"iou": abi.SA_POS_IOU, "maha": abi.SA_POS_MAHALANOBIS}


class Stub(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("ok_class", "ok_words", "ok_plain", "calls", "eu_mfma", "vote_words", "class_words")]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan")
    (d / "plan.cpp").write_text(SRC)
    so = d / "libplan.so"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", str(CSRC), "-o", str(so), str(d / "plan.cpp")], check=True)
    f = C.CDLL(str(so)).plan
    f.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(Stub),
                  C.POINTER(C.c_int)]
    return f


def plan(lib, vis="cosine", K=1, flags=0, N=1000, T=1000, feats=True, backing_off=False, pos="iou", min_votes=1, eu_ok=True,
         ok=(True, True, True), stub=None):
    """The plan of one frame; the engine's capability bits as sa_create sets them.  ok = the stub's answers (class words, cell words, other)."""
    bf = (flags & abi.SA_FLAG_BESTFIT_TILE) != 0
    caps = ((vis == "cosine" and K == 1 and min_votes <= 1 and not bf) * 1 | (vis == "euclidean" and K == 1 and min_votes <= 1 and not bf) * 2 |
            bf * 4 | (vis == "euclidean" and eu_ok) * 8)
    stub = stub if stub is not None else Stub()
    stub.ok_class, stub.ok_words, stub.ok_plain = ok
    out = (C.c_int * 9)()
    lib(POS[pos], VIS[vis], flags, K, caps, N, T, int(feats), int(backing_off), C.byref(stub), out)
    return dict(zip(FIELDS, out))


def test_tail_boundaries(lib):
    for (n, t), tail in {(1024, 1024): SMALL, (1, 1): SMALL, (0, 0): SMALL, (1025, 1024): SMALL2, (1024, 1025): SMALL_TC2,
                         (1024, 2048): SMALL_TC2, (2048, 2048): SMALL2, (2049, 2048): GENERAL, (2048, 2049): GENERAL, (1025, 2049): GENERAL,
                         (1024, 2049): SMALL2_1X4, (1024, 4096): SMALL2_1X4, (1024, 4097): GENERAL, (2049, 10): GENERAL}.items():
        for vis in ("none", "cosine"):
            assert plan(lib, vis, N=n, T=t)["tail"] == tail, (vis, n, t)
    assert plan(lib, "none", N=10, T=10, flags=abi.SA_FLAG_GENERAL_TAIL)["tail"] == GENERAL
    # tile words (10-bit index) only on frames the one-column tail takes: wider frames resolve, and keep the wider one-workgroup tails
    sep = abi.SA_FLAG_SEPARATE_FRAME
    assert [plan(lib, K=3, flags=sep, N=1024, T=1024)[k] for k in ("vote", "tail")] == [TILE, SMALL]
    assert [plan(lib, K=3, flags=sep, N=1025, T=1024)[k] for k in ("vote", "tail")] == [RESOLVE, SMALL2]
    assert [plan(lib, K=3, flags=sep, N=1024, T=1025)[k] for k in ("vote", "tail")] == [RESOLVE, SMALL_TC2]
    assert [plan(lib, K=3, flags=sep, N=1024, T=2049)[k] for k in ("vote", "tail")] == [RESOLVE, SMALL2_1X4]
    assert [plan(lib, K=3, flags=sep | abi.SA_FLAG_GENERAL_TAIL, N=10, T=10)[k] for k in ("vote", "tail")] == [RESOLVE, GENERAL]


def test_vote_forms(lib):
    p = plan(lib)   # cosine, one observation per track
    assert (p["vote"], p["partials"], p["eu_mfma"]) == (CELL, 1, 0)
    assert (plan(lib, N=3000, T=3000)["vote"], plan(lib, flags=abi.SA_FLAG_GENERAL_TAIL)["vote"]) == (CELL, CELL)   # any frame size
    assert plan(lib, min_votes=2)["vote"] == TILE and plan(lib, min_votes=2, N=1025)["vote"] == RESOLVE
    # euclidean: the matrix-core expansion votes itself; the vector-pipe kernel reduces into the words too, without partials
    assert [plan(lib, "euclidean")[k] for k in ("vote", "partials", "eu_mfma")] == [CELL, 1, 1]
    assert [plan(lib, "euclidean", flags=abi.SA_FLAG_EUCLID_VALU)[k] for k in ("vote", "partials", "eu_mfma")] == [CELL, 0, 0]
    assert [plan(lib, "euclidean", backing_off=True)[k] for k in ("vote", "partials", "eu_mfma")] == [CELL, 0, 0]
    assert plan(lib, "euclidean", backing_off=True, flags=abi.SA_FLAG_EUCLID_MFMA)["eu_mfma"] == 1
    assert plan(lib, "euclidean", eu_ok=False)["eu_mfma"] == 0
    assert plan(lib, "euclidean", flags=abi.SA_FLAG_BESTFIT_TILE)["vote"] == TILE
    # deeper banks: class words wherever the fused first phase takes them, else tile words on small frames
    assert [plan(lib, K=3)[k] for k in ("vote", "partials", "fused")] == [CLASS, 0, 1]
    assert [plan(lib, K=3, N=1025, T=3000)[k] for k in ("vote", "tail", "fused")] == [CLASS, GENERAL, 1]
    assert plan(lib, "euclidean", K=3)["vote"] == CLASS and plan(lib, K=8)["vote"] == CLASS
    assert plan(lib, K=9)["vote"] == TILE
    assert plan(lib, K=3, flags=abi.SA_FLAG_SEPARATE_FRAME)["vote"] == TILE
    assert plan(lib, K=3, flags=abi.SA_FLAG_BESTFIT_TILE)["vote"] == TILE
    assert plan(lib, K=3, feats=False)["vote"] == TILE
    assert plan(lib, K=3, ok=(False, True, True))["vote"] == TILE
    assert plan(lib, K=3, ok=(False, True, True), N=1025)["vote"] == RESOLVE
    # no vote words at all
    for kw in (dict(), dict(K=3), dict(vis="euclidean")):
        p = plan(lib, flags=abi.SA_FLAG_SEPARATE_RESOLVE, **{"vis": "cosine", **kw})
        assert p["vote"] == RESOLVE and p["prep"] == ALL, kw
    assert plan(lib, flags=abi.SA_FLAG_SEPARATE_RESOLVE)["partials"] == 1
    assert plan(lib, "none")["vote"] == RESOLVE and plan(lib, "none")["partials"] == 0


def test_preparation_blocks(lib):
    lean = abi.SA_FLAG_NEVER_LEAN
    assert plan(lib)["prep"] == NONE and plan(lib, N=1025)["prep"] == NONE and plan(lib, T=4000)["prep"] == NONE
    assert plan(lib, flags=abi.SA_FLAG_GENERAL_TAIL)["prep"] == RESET and plan(lib, N=3000, T=3000)["prep"] == RESET
    assert plan(lib, flags=lean)["prep"] == ALL and plan(lib, flags=lean | abi.SA_FLAG_GENERAL_TAIL)["prep"] == ALL
    assert plan(lib, "none")["prep"] == NONE and plan(lib, "none", N=5000)["prep"] == RESET and plan(lib, "none", flags=lean)["prep"] == ALL
    assert plan(lib, K=3)["prep"] == NONE and plan(lib, K=3, N=3000)["prep"] == RESET
    # the stand-alone contraction reads what the preparation blocks write
    assert plan(lib, flags=abi.SA_FLAG_SEPARATE_FRAME)["prep"] == ALL
    assert plan(lib, feats=False)["prep"] == ALL and plan(lib, ok=(True, False, False))["prep"] == ALL
    assert plan(lib, K=3, flags=abi.SA_FLAG_SEPARATE_FRAME)["prep"] == ALL
    assert plan(lib, K=3, flags=abi.SA_FLAG_BESTFIT_TILE)["prep"] == NONE   # tile words on the fused first phase


def test_fused_or_separate(lib):
    s = Stub()
    assert plan(lib, stub=s)["fused"] == 1 and s.calls == 1 and (s.eu_mfma, s.vote_words, s.class_words) == (0, 1, 0)
    s = Stub()
    assert plan(lib, "euclidean", stub=s)["fused"] == 1 and (s.calls, s.eu_mfma, s.vote_words, s.class_words) == (1, 1, 1, 0)
    s = Stub()
    assert plan(lib, "euclidean", flags=abi.SA_FLAG_EUCLID_VALU, ok=(False, False, False), stub=s)["fused"] == 0 and s.eu_mfma == 0
    s = Stub()
    assert plan(lib, K=3, stub=s)["fused"] == 1 and (s.calls, s.eu_mfma, s.vote_words, s.class_words) == (1, 0, 0, 1)
    s = Stub()
    assert plan(lib, K=3, flags=abi.SA_FLAG_BESTFIT_TILE, stub=s)["fused"] == 1 and (s.calls, s.vote_words, s.class_words) == (1, 0, 0)
    s = Stub()
    assert plan(lib, K=3, ok=(False, False, True), stub=s)["fused"] == 1 and s.calls == 2
    s = Stub()
    assert plan(lib, feats=False, stub=s)["fused"] == 0 and s.calls == 0          # a scene without features
    s = Stub()
    assert plan(lib, flags=abi.SA_FLAG_SEPARATE_FRAME, stub=s)["fused"] == 0 and s.calls == 0
    assert plan(lib, ok=(True, False, True))["fused"] == 0                         # the predicate refuses
    s = Stub()
    assert plan(lib, "none", stub=s)["fused"] == 0 and s.calls == 0


def test_lazy_possible_and_reports_left(lib):
    assert [plan(lib)[k] for k in ("lazy_possible", "lazy", "reports_left")] == [1, 0, 1]
    assert [plan(lib, N=1024, T=1024)[k] for k in ("lazy_possible", "reports_left")] == [1, 1]
    for kw in (dict(N=1025), dict(T=1025), dict(flags=abi.SA_FLAG_GENERAL_TAIL), dict(flags=abi.SA_FLAG_SEPARATE_RESOLVE)):
        assert [plan(lib, **kw)[k] for k in ("lazy_possible", "reports_left")] == [0, 0], kw
    # the vote words of other forms report leftover rows, but have no lazy phase
    for kw in (dict(vis="euclidean"), dict(pos="maha"), dict(K=3), dict(K=3, flags=abi.SA_FLAG_SEPARATE_FRAME), dict(min_votes=2)):
        assert [plan(lib, **kw)[k] for k in ("lazy_possible", "reports_left")] == [0, 1], kw
    assert plan(lib, flags=abi.SA_FLAG_SEPARATE_FRAME)["lazy_possible"] == 1     # the separate first phase has a lazy form too
    assert [plan(lib, "none")[k] for k in ("lazy_possible", "reports_left")] == [0, 0]
    assert plan(lib, flags=abi.SA_FLAG_LAZY_POSITIONAL)["lazy"] == 0           # settled at launch time (sa_lazy_positional)
