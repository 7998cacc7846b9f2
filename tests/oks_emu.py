"""Builds and binds tests/emu_oks/libemu_oks.so: similari_amd/csrc/sa_pose_oks.h over sa_pose_gate.h and sa_pose.h compiled by g++ with
the flags of tests/pose_emu.py.  TEST INFRASTRUCTURE, for tests/test_oks_emu.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
EMU_DIR = ROOT / "tests" / "emu_oks"
f32 = np.float32
_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    so = EMU_DIR / "libemu_oks.so"
    csrc = ROOT / "similari_amd" / "csrc"
    srcs = [EMU_DIR / "emu_oks.cpp", csrc / "sa_pose_oks.h", csrc / "sa_pose_gate.h", csrc / "sa_pose.h", csrc / "sa_device.h"]
    if not so.exists() or any(s.stat().st_mtime > so.stat().st_mtime for s in srcs):
        subprocess.run(
            ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-o", str(so), str(EMU_DIR / "emu_oks.cpp")],
            check=True,
        )
    L = C.CDLL(str(so))
    fp, bp, u32 = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.c_uint32
    for name, (res, args) in {
        "emu_oks_exp": (None, [C.c_uint64, fp, fp]),
        "emu_oks_var2": (None, [u32, fp, fp]),
        "emu_oks_area": (None, [u32, u32, fp, bp, fp]),
        "emu_oks_matrix": (None, [u32, u32, u32, fp, bp, bp, fp, fp, u32, fp]),
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


def exp(e):
    e = np.ascontiguousarray(e, f32).reshape(-1)
    out = np.empty(len(e), f32)
    lib().emu_oks_exp(len(e), _f(e), _f(out))
    return out


def var2(sigmas):
    s = np.ascontiguousarray(sigmas, f32).reshape(-1)
    out = np.empty(len(s), f32)
    lib().emu_oks_var2(len(s), _f(s), _f(out))
    return out


def area(xy, counts):
    xy, counts = np.ascontiguousarray(xy, f32), np.ascontiguousarray(counts, np.uint8)
    n, P = counts.shape
    out = np.empty(n, f32)
    lib().emu_oks_area(n, P, _f(xy), _b(counts), _f(out))
    return out


def matrix(poses, present, has, mean, sigmas, min_common=1):
    """poses [M, P, 2], present [M, P]; has [T, P], mean [T, P, 4]; sigmas [P] -> w [M, T], NaN = no pair"""
    poses = np.ascontiguousarray(poses, f32)
    M, P = poses.shape[:2]
    T = len(has)
    present, has = np.ascontiguousarray(present, np.uint8), np.ascontiguousarray(has, np.uint8)
    mean, v2 = np.ascontiguousarray(mean, f32), var2(sigmas)
    w = np.empty((M, T), f32)
    lib().emu_oks_matrix(M, T, P, _f(poses), _b(present), _b(has), _f(mean), _f(v2), min_common, _f(w))
    return w
