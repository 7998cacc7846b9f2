"""include/similari_pose_nms.h against its ctypes mirror similari_amd/pose_nms.py: struct sizes and offsets by a compiled driver, every
declared function exported and bound, the defaults, the refusals that need no device, and the build lists.  No GPU needed."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "similari_pose_nms.h"
DRIVER = r"""
#include <cstdio>
#include <cstddef>
#include "similari_pose_nms.h"
int main() {
  std::printf("%zu %zu %zu %zu %zu %zu ", sizeof(sa_pose_nms_options), offsetof(sa_pose_nms_options, min_common), offsetof(sa_pose_nms_options, n_sigmas),
              offsetof(sa_pose_nms_options, sigmas), offsetof(sa_pose_nms_options, nms_threshold), offsetof(sa_pose_nms_options, score_threshold));
  std::printf("%zu %zu %zu %zu %zu %zu %zu ", sizeof(sa_pose_nms_stats), offsetof(sa_pose_nms_stats, poses), offsetof(sa_pose_nms_stats, host_waits),
              offsetof(sa_pose_nms_stats, bytes_h2d), offsetof(sa_pose_nms_stats, bytes_d2h), offsetof(sa_pose_nms_stats, src_bytes),
              offsetof(sa_pose_nms_stats, device_ms));
  std::printf("%u %u %u\n", SA_POSE_NMS_MAX_SCENES, SA_POSE_NMS_MAX, SA_POSE_NMS_TAP_MAX);
  return 0;
}
"""
DECLARED = ["sa_pose_nms", "sa_pose_nms_batch", "sa_pose_nms_last", "sa_pose_nms_matrix", "sa_pose_nms_options_default"]


def field_names(struct):
    body = re.search(r"typedef struct %s \{(.*?)\}" % struct, HEADER.read_text(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [part.replace("*", " ").split()[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]


def test_the_structs_equal_their_mirrors(tmp_path):
    from similari_amd import pose_nms as N

    cxx = shutil.which("g++") or shutil.which("c++")
    (tmp_path / "drv.cpp").write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-I", str(ROOT / "include"), "-o", str(tmp_path / "drv"), str(tmp_path / "drv.cpp")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "drv")], check=True, capture_output=True, text=True).stdout.split()]
    O, S = N.sa_pose_nms_options, N.sa_pose_nms_stats
    assert out[:6] == [32, 8, 12, 16, 24, 28] == [C.sizeof(O), O.min_common.offset, O.n_sigmas.offset, O.sigmas.offset, O.nms_threshold.offset,
                                                   O.score_threshold.offset]
    assert out[6:13] == [56, 8, 16, 24, 32, 40, 48] == [C.sizeof(S), S.poses.offset, S.host_waits.offset, S.bytes_h2d.offset, S.bytes_d2h.offset,
                                                         S.src_bytes.offset, S.device_ms.offset]
    assert out[13:] == [65535, 16384, 2048] == [N.SA_POSE_NMS_MAX_SCENES, N.SA_POSE_NMS_MAX, N.SA_POSE_NMS_TAP_MAX]
    assert field_names("sa_pose_nms_options") == [f for f, _ in O._fields_] and field_names("sa_pose_nms_stats") == [f for f, _ in S._fields_]
    text = HEADER.read_text()
    assert re.search(r"\} sa_pose_nms_options;\s*/\* 32 B \*/", text) and re.search(r"\} sa_pose_nms_stats;\s*/\* 56 B \*/", text)


def test_every_declared_symbol_is_bound_and_exported():
    from similari_amd import build
    from similari_amd import pose_nms as N

    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:int|void)\s+(sa_[a-z0-9_]+)\s*\(", text, flags=re.M)))
    assert declared == DECLARED and set(N.PROTOTYPES) == set(declared)
    lib = C.CDLL(str(build.build_lib()))
    assert not [n for n in declared if not hasattr(lib, n)]
    N.bind(lib)
    assert lib.sa_pose_nms.restype is C.c_int


def test_defaults_and_null_engine_refusals():
    from similari_amd import build
    from similari_amd import pose_nms as N

    lib = N.bind(C.CDLL(str(build.build_lib())))
    o = N.sa_pose_nms_options()
    lib.sa_pose_nms_options_default(C.byref(o))   # needs no device
    lib.sa_pose_nms_options_default(None)
    assert (o.struct_size, o.points, o.min_common, o.n_sigmas, bool(o.sigmas)) == (32, 17, 1, 0, False)
    assert o.nms_threshold == np.float32(0.9) and np.isnan(o.score_threshold)
    keep, sig, o2 = np.full(4, 77, np.uint32), *N.options(lib)
    n = C.c_uint32(77)
    assert (o2.points, o2.n_sigmas) == (17, 17) and len(sig) == 17
    u32p = C.POINTER(C.c_uint32)
    assert lib.sa_pose_nms(None, C.byref(o2), 0, None, None, keep.ctypes.data_as(u32p), C.byref(n)) != 0
    assert lib.sa_pose_nms_batch(None, C.byref(o2), 0, None, None, None, None, None) != 0
    assert lib.sa_pose_nms_matrix(None, C.byref(o2), 0, None, None, None, None, C.byref(n)) != 0
    assert lib.sa_pose_nms_last(None, None) != 0
    assert n.value == 77 and (keep == 77).all()


def test_the_source_and_the_header_are_built():
    from similari_amd import build

    assert "sa_pose_nms.hip" in build.SOURCES and HEADER in build.HEADERS and build.CSRC / "sa_pose_nms.h" in build.HEADERS
    src = (build.CSRC / "sa_pose_nms.hip").read_text()
    assert "k_pose_nms_mask" in src and "k_pose_nms_lay" in src and "sa_launch_nms_sweep" in src and '#include "sa_pose_nms.h"' in src
    assert "sa_launch_nms_sweep" in (build.CSRC / "sa_upkeep.hip").read_text()
    assert "import torch" not in (ROOT / "similari_amd" / "pose_nms.py").read_text()
