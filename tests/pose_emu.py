"""Builds and binds tests/emu_pose/libemu_pose.so: similari_amd/csrc/sa_pose.h, sa_kalman_point.h and sa_dense.h compiled by g++ with the
flags of tests/points_emu.py.  TEST INFRASTRUCTURE, shared by tests/test_pose_emu.py and scripts/bench_pose.py (the same arithmetic on
one host core)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
EMU_DIR = ROOT / "tests" / "emu_pose"
f32 = np.float32
_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    so = EMU_DIR / "libemu_pose.so"
    csrc = ROOT / "similari_amd" / "csrc"
    srcs = [EMU_DIR / "emu_pose.cpp", csrc / "sa_pose.h", csrc / "sa_kalman_point.h", csrc / "sa_dense.h", csrc / "sa_device.h"]
    if not so.exists() or any(s.stat().st_mtime > so.stat().st_mtime for s in srcs):
        subprocess.run(
            ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-o", str(so), str(EMU_DIR / "emu_pose.cpp")],
            check=True,
        )
    L = C.CDLL(str(so))
    fp, bp, u32, fl, i64 = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.c_uint32, C.c_float, C.c_int64
    for name, (res, args) in {
        "emu_pose_factor": (None, [fl, u32, fp, fp, fp, bp]),
        "emu_pose_distance_factored": (None, [u32, fp, bp, fp, fp]),
        "emu_pose_matrix": (None, [fl, u32, u32, u32, fp, bp, bp, fp, fp, u32, fp]),
        "emu_pose_threshold_q": (i64, [fl]),
        "emu_pose_gain": (i64, [fl, i64]),
        "emu_pose_assign": (C.c_int, [u32, u32, fp, fl, C.POINTER(C.c_int32), C.POINTER(i64), C.POINTER(u32)]),
    }.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _b(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def factor(mean, cov, pw):
    """-> (fac [n, 5]: mean x, y, l00, l10, l11; ok [n] bool)"""
    m = np.ascontiguousarray(mean, f32).reshape(-1, 4)
    c = np.ascontiguousarray(cov, f32).reshape(-1, 16)
    fac, ok = np.zeros((len(m), 5), f32), np.zeros(len(m), np.uint8)
    lib().emu_pose_factor(pw, len(m), _f(m), _f(c), _f(fac), _b(ok))
    return fac, ok.astype(bool)


def distance_factored(fac, ok, z):
    fac, z = np.ascontiguousarray(fac, f32), np.ascontiguousarray(z, f32).reshape(-1, 2)
    ok = np.ascontiguousarray(ok, np.uint8)
    out = np.empty(len(fac), f32)
    lib().emu_pose_distance_factored(len(fac), _f(fac), _b(ok), _f(z), _f(out))
    return out


def matrix(poses, present, has, mean, cov, pw, min_common=1):
    """poses [M, P, 2], present [M, P]; has [T, P], mean [T, P, 4], cov [T, P, 4, 4] -> w [M, T], NaN = no pair"""
    poses = np.ascontiguousarray(poses, f32)
    M, P = poses.shape[:2]
    T = len(has)
    present, has = np.ascontiguousarray(present, np.uint8), np.ascontiguousarray(has, np.uint8)
    mean, cov = np.ascontiguousarray(mean, f32), np.ascontiguousarray(cov, f32)
    w = np.empty((M, T), f32)
    lib().emu_pose_matrix(pw, M, T, P, _f(poses), _b(present), _b(has), _f(mean), _f(cov), min_common, _f(w))
    return w


def assign(w, threshold=1.0):
    """The device's route over w [M, T] -> (rmatch [M] column or -1, total gain, search roots)"""
    w = np.ascontiguousarray(w, f32)
    M, T = w.shape
    rm = np.zeros(max(M, 1), np.int32)
    tot, roots = C.c_int64(), C.c_uint32()
    rc = lib().emu_pose_assign(M, T, _f(w), threshold, rm.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(tot), C.byref(roots))
    assert rc == 0, f"pose route: inconsistent matching ({rc})"
    return rm[:M].astype(np.int64), tot.value, roots.value
