"""SaFramePlan::one_launch (similari_amd/csrc/sa_plan.h) on its own (host-only): a lazy frame whose first phase is the helped contraction
tiles alone runs its tail in the same launch where the config asks for it (SA_FLAG_ONE_LAUNCH).  The form is opt-in — measured, it is
slightly slower than the two launches at C2's shape, and only a measured gain would make it the default ("One launch") —, so every
case here asks for it except the one that checks that an engine that does not ask keeps two launches.  The plan goes through the real
planner, the launch-time mode through sa_lazy_positional, then sa_one_launch settles the form; sa_frame_visual_ok and
sa_frame_visual_helped (device-side files) are stubs that say yes."""
import ctypes as C
import subprocess

import pytest

from similari_amd import abi

CSRC = __import__("pathlib").Path(__file__).resolve().parent.parent / "similari_amd" / "csrc"

SRC = r'''
#include "sa_plan.h"
static bool visual_ok(const void*, bool, bool, bool) { return true; }
// caps: the engine's capability bits as sa_create sets them; hint: the scenes' leftover rows; returns lazy | one_launch << 1
extern "C" int one_launch(int pos, int vis, unsigned flags, unsigned K, unsigned caps, unsigned N, unsigned T, unsigned hint, int profile,
                          int helped, unsigned blocks, unsigned n_cu) {
  SaPlanInputs in{pos, vis, flags, K, N, T, (caps & 1) != 0, (caps & 2) != 0, (caps & 4) != 0, (caps & 8) != 0, true, false, visual_ok, nullptr};
  in.n_cu = n_cu;
  in.profile = profile != 0;
  SaFramePlan p = sa_frame_plan(in);
  if (p.one_launch) return -1;   // settled at launch time only
  p.lazy = sa_lazy_positional(p.lazy_possible, flags, hint);
  p.one_launch = sa_one_launch(p, in, helped != 0, blocks);
  return (p.lazy ? 1 : 0) | (p.one_launch ? 2 : 0);
}
'''

VIS = {"cosine": abi.SA_VIS_COSINE, "euclidean": abi.SA_VIS_EUCLIDEAN}
N_CU = 256


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("one_launch")
    (d / "plan.cpp").write_text(SRC)
    so = d / "libplan.so"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", str(CSRC), "-o", str(so), str(d / "plan.cpp")], check=True)
    f = C.CDLL(str(so)).one_launch
    f.argtypes = [C.c_int, C.c_int] + [C.c_uint32] * 6 + [C.c_int, C.c_int, C.c_uint32, C.c_uint32]
    return f


def blocks_of(n, t, ns=1):
    """Blocks of the helped launch: the 64 x 64 tiles of the widest scene rounded up to the eight XCD chunks, per scene."""
    tiles = -(-n // 64) * -(-t // 64)
    return 8 * -(-tiles // 8) * ns


def settle(lib, vis="cosine", K=1, flags=0, N=1000, T=1000, hint=0, profile=False, helped=True, ns=1, n_cu=N_CU, ask=True):
    """(lazy, one_launch) of a frame; `ask`: the engine's config asks for the one-launch form (SA_FLAG_ONE_LAUNCH)."""
    flags |= abi.SA_FLAG_ONE_LAUNCH if ask else 0
    caps = (vis == "cosine" and K == 1) * 1 | (vis == "euclidean" and K == 1) * 2 | (vis == "euclidean") * 8
    r = lib(abi.SA_POS_IOU, VIS[vis], flags, K, caps, N, T, hint, int(profile), int(helped), blocks_of(N, T, ns), n_cu)
    assert r >= 0
    return bool(r & 1), bool(r & 2)


def test_c2_runs_in_one_launch(lib):
    """... where the config asks for it."""
    assert settle(lib) == (True, True)                                          # 1000 x 1000 x 512-d cosine + IoU, no leftover rows reported yet
    assert settle(lib, hint=14) == (True, True)
    assert settle(lib, flags=abi.SA_FLAG_LAZY_POSITIONAL, hint=500) == (True, True)
    assert settle(lib, N=1, T=1) == (True, True) and settle(lib, N=1024, T=1024) == (True, True)


def test_what_clears_it(lib):
    assert settle(lib, ask=False) == (True, False)                               # not asked for
    assert settle(lib, flags=abi.SA_FLAG_EAGER_POSITIONAL) == (False, False)     # eager: by the flag, by the hint, by the taps' default
    assert settle(lib, hint=15) == (False, False)
    assert settle(lib, flags=abi.SA_FLAG_TAP) == (False, False)
    assert settle(lib, K=3) == (False, False)                                    # deeper banks
    assert settle(lib, vis="euclidean") == (False, False)
    assert settle(lib, T=1025) == (False, False) and settle(lib, N=1025) == (False, False)   # beyond the one-column-per-thread tail
    assert settle(lib, flags=abi.SA_FLAG_GENERAL_TAIL) == (False, False)
    assert settle(lib, profile=True) == (True, False)                            # lazy still, two launches
    assert settle(lib, flags=abi.SA_FLAG_SEPARATE_TAIL) == (True, False)
    assert settle(lib, flags=abi.SA_FLAG_SEPARATE_FRAME) == (True, False)        # no fused first phase to ride in
    assert settle(lib, helped=False) == (True, False)                            # the first phase is not the helped tiles alone


def test_one_block_per_compute_unit(lib):
    assert blocks_of(1000, 1000) == 256 and blocks_of(1024, 1024) == 256 and blocks_of(130, 190) == 16 and blocks_of(1, 1) == 8
    assert settle(lib, n_cu=256) == (True, True) and settle(lib, n_cu=255) == (True, False)
    assert settle(lib, ns=2) == (True, False)                                    # two scenes of C2's size: 512 blocks
    assert settle(lib, N=600, T=640, ns=2) == (True, True)                       # 104 blocks a scene
    assert settle(lib, N=600, T=640, ns=3) == (True, False)
    assert settle(lib, N=130, T=190, ns=16) == (True, True) and settle(lib, N=130, T=190, ns=17) == (True, False)
