"""include/similari_pose_oks.h against its ctypes mirror similari_amd/pose_oks.py: every declared function is exported by the library
and bound, sa_pose_metric is 24 bytes in C and in the mirror, field for field.  No GPU needed.  (The refusals of sa_points_set_metric
need a bank, and a bank needs a device: they are in tests/test_gpu_oks.py.)"""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "similari_pose_oks.h"
DRIVER = r"""
#include <cstdio>
#include <cstddef>
#include "similari_pose_oks.h"
int main() {
  std::printf("%zu %zu %zu %u %u\n", sizeof(sa_pose_metric), offsetof(sa_pose_metric, reserved), offsetof(sa_pose_metric, sigmas),
              SA_POSE_METRIC_MAHALANOBIS, SA_POSE_METRIC_OKS);
  return 0;
}
"""


def test_the_struct_is_24_bytes_and_equals_its_mirror(tmp_path):
    from similari_amd import pose_oks as K

    cxx = shutil.which("g++") or shutil.which("c++")
    (tmp_path / "drv.cpp").write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-I", str(ROOT / "include"), "-o", str(tmp_path / "drv"), str(tmp_path / "drv.cpp")], check=True)
    out = subprocess.run([str(tmp_path / "drv")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [24, 12, 16, K.SA_POSE_METRIC_MAHALANOBIS, K.SA_POSE_METRIC_OKS]
    assert C.sizeof(K.sa_pose_metric) == 24 and K.sa_pose_metric.reserved.offset == 12 and K.sa_pose_metric.sigmas.offset == 16
    fields = re.search(r"typedef struct sa_pose_metric \{(.*?)\}", HEADER.read_text(), flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [part.replace("*", " ").split()[-1] for decl in fields.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f for f, _ in K.sa_pose_metric._fields_]


def test_every_declared_symbol_is_bound_and_exported():
    from similari_amd import build
    from similari_amd import pose_oks as K

    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:int|void)\s+(sa_[a-z0-9_]+)\s*\(", text, flags=re.M)))
    assert declared == ["sa_points_get_metric", "sa_points_set_metric", "sa_pose_metric_default"] and set(K.PROTOTYPES) == set(declared)
    lib = C.CDLL(str(build.build_lib()))
    assert not [n for n in declared if not hasattr(lib, n)]
    K.bind(lib)
    assert lib.sa_points_set_metric.restype is C.c_int
    m = K.sa_pose_metric()
    lib.sa_pose_metric_default(C.byref(m))   # needs no device
    assert (m.struct_size, m.kind, m.n_sigmas, m.reserved, bool(m.sigmas)) == (24, K.SA_POSE_METRIC_MAHALANOBIS, 0, 0, False)
    assert lib.sa_points_set_metric(None, C.byref(m)) != 0 and lib.sa_points_get_metric(None, None, None) != 0


def test_the_python_face():
    from similari_amd import pose_oks as K

    assert len(K.COCO_SIGMAS) == 17 and K.COCO_SIGMAS[0] == .026 and K.COCO_SIGMAS[-1] == .089 and sum(K.COCO_SIGMAS) == sum(
        (.026, .025, .025, .035, .035, .079, .079, .072, .072, .062, .062, .107, .107, .087, .087, .089, .089))
    m = K.OksMetric(K.COCO_SIGMAS)
    assert m.sigmas.dtype == np.float32 and m == K.OksMetric(np.array(K.COCO_SIGMAS, np.float32)) and m != K.OksMetric([1.0] * 17)
    assert K.default_threshold(m, None) == 0.3 and K.default_threshold(None, None) == 1.0 and K.default_threshold(m, 0.5) == 0.5
