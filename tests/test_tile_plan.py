"""The contraction's tile plans (similari_amd/csrc/sa_tile_plan.h) on their own (host-only): which tile, main loop and k-group count
each entry point launches for every plan number, pinned and not, and what the other callers ask of the table (tile extents, the
64 x 64 family, the 64 x 96 pin, operands in fragment order).  The expected forms are written out below, recorded from the switch
statements the table replaced."""
import ctypes as C
import subprocess

import pytest

CSRC = __import__("pathlib").Path(__file__).resolve().parent.parent / "similari_amd" / "csrc"

SRC = r'''
#include "sa_tile_plan.h"
extern "C" void launched(int use, int plan_override, int staged, unsigned M, unsigned Ncols, unsigned ns, unsigned Dp, int* out) {
  const SaTileForm f = sa_tile_form((SaTileUse)use, sa_tile_resolve((SaTileUse)use, M, Ncols, ns, Dp, plan_override, staged != 0));
  const int o[9] = {f.bm, f.bn, (int)f.loop, f.kg, f.a_frag, f.b_frag, (int)f.threads(), (int)f.loop_lds_floats(), f.min_blocks_per_cu()};
  for (int i = 0; i < 9; ++i) out[i] = o[i];
}
extern "C" void frame(int plan_override, unsigned M, unsigned Ncols, unsigned ns, unsigned Dp, int* out) {
  const int plan = tile_plan(M, Ncols, ns, Dp, plan_override);   // as sa_visual_tile / sa_frame_visual_ok / sa_launch_frame_visual ask
  const SaTileForm f = sa_tile_form(SaTileUse::cosine, plan);
  out[0] = f.bm; out[1] = f.bn; out[2] = sa_plan_is_64x64(plan); out[3] = sa_plan_pins_w96(plan_override);
}
extern "C" int choice(unsigned M, unsigned Ncols, unsigned ns, unsigned Dp) { return tile_plan(M, Ncols, ns, Dp); }
extern "C" int looped(int plan, int plan_override, int staged) { return loop_plan(plan, plan_override, staged != 0); }
'''

STAGED, RING, KSPLIT, DIRECT, KS128 = range(5)   # SaLoop
COSINE, PARTIALS, EUCLID, MATRIX = range(4)                           # SaTileUse

# (BM, BN, loop, k-groups, a_frag, b_frag)
S128 = (128, 128, STAGED, 1, 0, 0)
S64 = (64, 64, STAGED, 1, 0, 0)
S64K2 = (64, 64, STAGED, 2, 0, 0)
S64K4 = (64, 64, STAGED, 4, 0, 0)
S64x128 = (64, 128, STAGED, 1, 0, 0)
S128x64 = (128, 64, STAGED, 1, 0, 0)
R64 = (64, 64, RING, 1, 0, 0)
R128 = (128, 128, RING, 1, 0, 0)
KS = (64, 64, KSPLIT, 1, 0, 0)
KSB = (64, 64, KSPLIT, 1, 0, 1)
KSAB = (64, 64, KSPLIT, 1, 1, 1)
D128 = (128, 128, DIRECT, 1, 0, 1)
D64x128 = (64, 128, DIRECT, 1, 0, 1)
D128x64 = (128, 64, DIRECT, 1, 0, 1)
K128 = (64, 128, KS128, 1, 0, 1)

# plan_override 0 .. 21 at 1000 x 1000 x 512, one scene, for each entry point (pinned: SA_FLAG_STAGED_LOOP changes nothing)
PINNED = {
    COSINE:   [S128, S64, S64K2, S64, S64K4, S64x128, S128x64, R64, R128, KSB, S64, S64, S64, S64, S64, D128, D64x128, S64, K128, KSB, S64, S64],
    PARTIALS: [S128, S64, S64K2, S64, S64K2, S64x128, S128x64, S64, S128, KSB, S64, S64, S64, S64, S64, D128, D64x128, S64, K128, KSB, S64, S64],
    EUCLID:   [S128, S64, S64, S64, S64, S64x128, S128x64, S64, S128, KSB, S64, S64, S64, S64, S64, D128, D64x128, S64, K128, KSB, S64, S64],
    MATRIX:   [S128, S64, S64K2, S64, S64K4, S64x128, S128x64, R64, R128, KS, KSB, S64, S64, KSAB, S64, D128, D64x128, D128x64, K128, KS, S64, S64],
}
# plan_override -1 at that size (tile_plan: 2): (k-split loop, SA_FLAG_STAGED_LOOP)
UNPINNED = {COSINE: (KSB, S64K2), PARTIALS: (KSB, S64K2), EUCLID: (KSB, S64), MATRIX: (S64K2, S64K2)}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_plan")
    (d / "tile_plan.cpp").write_text(SRC)
    so = d / "libtile_plan.so"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", str(CSRC), "-o", str(so), str(d / "tile_plan.cpp")],
                   check=True)
    return C.CDLL(str(so))


def launched(lib, use, plan=-1, staged=False, N=1000, T=1000, ns=1, D=512, full=False):
    out = (C.c_int * 9)()
    lib.launched(use, plan, int(staged), N, T, ns, D, out)
    return tuple(out) if full else tuple(out)[:6]


def frame(lib, plan=-1, N=1000, T=1000, ns=1, D=512):
    out = (C.c_int * 4)()
    lib.frame(plan, N, T, ns, D, out)
    return tuple(out)


def test_every_plan_number_at_every_entry_point(lib):
    for use, forms in PINNED.items():
        assert len(forms) == 22
        for plan, form in enumerate(forms):
            for staged in (False, True):
                assert launched(lib, use, plan, staged) == form, (use, plan, staged)
        for staged in (False, True):
            assert launched(lib, use, -1, staged) == UNPINNED[use][staged], (use, staged)


def test_what_the_form_answers(lib):
    # (threads per block, LDS floats of the main loop, min blocks per CU)
    for plan, tail in {0: (256, 2 * 256 * 32, 1), 2: (512, 4 * 128 * 32, 1), 4: (1024, 8 * 128 * 32, 1), 7: (256, 3 * 128 * 32, 1),
                       8: (256, 3 * 256 * 32, 1), 9: (256, 4 * 4 * 64 * 4 + 4 * 32, 1), 15: (256, 0, 2), 16: (256, 0, 1), 17: (256, 0, 1),
                       18: (256, 8192, 1)}.items():
        assert launched(lib, MATRIX, plan, full=True)[6:] == tail, plan


def test_extents_family_and_pin(lib):
    wide = {0: (128, 128), 8: (128, 128), 15: (128, 128), 5: (64, 128), 16: (64, 128), 18: (64, 128), 6: (128, 64)}
    for plan in range(0, 22):
        bm, bn, is64, w96 = frame(lib, plan)
        assert (bm, bn) == wide.get(plan, (64, 64)), plan       # (17 is the distance matrix's: a frame runs plan 1 for it)
        assert is64 == (plan in (1, 2, 4, 7, 9, 19)), plan      # (19: tile_plan() answers 9)
        assert w96 == (plan == 19), plan
    assert frame(lib, -1) == (64, 64, 1, 0)
    assert frame(lib, -1, N=2000, T=5000) == (64, 128, 0, 0)
    assert frame(lib, -1, ns=8) == (128, 128, 0, 0)
    assert frame(lib, -1, N=20000, T=64) == (128, 64, 0, 0)


def test_unpinned_choices(lib):
    # (N, T, D, scenes): tile_plan(), after loop_plan(), the form with the k-split / direct loops, the form with SA_FLAG_STAGED_LOOP
    for (n, t, d, ns), (plan, loop, form, staged) in {
            (1000, 1000, 512, 1): (2, 9, KSB, S64K2),
            (2000, 5000, 512, 1): (5, 18, K128, S64x128),
            (5000, 2000, 4096, 1): (5, 18, K128, S64x128),     # C5
            (1000, 1000, 512, 8): (0, 15, D128, S128),         # many scenes: 128 x 128 on the direct loop
            (4096, 2048, 512, 1): (0, 15, D128, S128),
            (20000, 64, 512, 1): (6, 6, S128x64, S128x64),     # 128 x 64 stays staged
            (1000, 3000, 512, 1): (1, 9, KSB, S64),            # 752 tiles: two tiles per CU, one k-group
            (1000, 1000, 128, 1): (1, 9, KSB, S64),            # four k-steps: no k-groups
    }.items():
        assert lib.choice(n, t, ns, d) == plan, (n, t, d, ns)
        assert lib.looped(plan, -1, 0) == loop and lib.looped(plan, -1, 1) == plan and lib.looped(plan, plan, 0) == plan, (n, t, d, ns)
        for use in (COSINE, PARTIALS):
            assert launched(lib, use, -1, False, n, t, ns, d) == form, (use, n, t, d, ns)
            assert launched(lib, use, -1, True, n, t, ns, d) == staged, (use, n, t, d, ns)
        # the euclidean expansion: one k-group where the cosine plans take two
        assert launched(lib, EUCLID, -1, False, n, t, ns, d) == form
        assert launched(lib, EUCLID, -1, True, n, t, ns, d) == (S64 if staged == S64K2 else staged)
    # the distance matrix keeps tile_plan()'s staged choice (one scene), with the flag or without
    for staged in (False, True):
        assert launched(lib, MATRIX, -1, staged, 1000, 1000, 1, 512) == S64K2
        assert launched(lib, MATRIX, -1, staged, 2000, 5000, 1, 512) == S64x128
        assert launched(lib, MATRIX, -1, staged, 4096, 2048, 1, 512) == S128
