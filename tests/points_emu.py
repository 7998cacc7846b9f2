"""Builds and binds tests/emu_points/libemu_points.so: similari_amd/csrc/sa_kalman_point.h compiled by g++ with the flags of
tests/test_device_logic_emu.py.  TEST INFRASTRUCTURE, shared by tests/test_points_emu.py and scripts/bench_points.py (the same
arithmetic on one host core)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
EMU_DIR = ROOT / "tests" / "emu_points"
f32 = np.float32
_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    so = EMU_DIR / "libemu_points.so"
    csrc = ROOT / "similari_amd" / "csrc"
    srcs = [EMU_DIR / "emu_points.cpp", csrc / "sa_kalman_point.h", csrc / "sa_device.h"]
    if not so.exists() or any(s.stat().st_mtime > so.stat().st_mtime for s in srcs):
        subprocess.run(
            ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-o", str(so), str(EMU_DIR / "emu_points.cpp")],
            check=True,
        )
    L = C.CDLL(str(so))
    fp, bp, u32, fl = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.c_uint32, C.c_float
    for name, args in {
        "emu_pt_initiate": [fl, fl, u32, fp, fp, fp],
        "emu_pt_predict": [fl, fl, u32, fp, fp],
        "emu_pt_update": [fl, u32, fp, fp, fp],
        "emu_pt_distance": [fl, u32, fp, fp, fp, u32, fp],
        "emu_pt_present": [u32, u32, fp, fl, bp, bp],
        "emu_pt_step": [fl, fl, u32, fp, bp, bp, fp, fp, fp],
    }.items():
        fn = getattr(L, name)
        fn.restype = None
        fn.argtypes = args
    _lib = L
    return L


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _b(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))


def _flat(z, k):
    return np.ascontiguousarray(z, f32).reshape(-1, k)


def initiate(z, pw, vw):
    z = _flat(z, 2)
    m, c = np.empty((len(z), 4), f32), np.empty((len(z), 16), f32)
    lib().emu_pt_initiate(pw, vw, len(z), _f(z), _f(m), _f(c))
    return m, c.reshape(-1, 4, 4)


def predict(mean, cov, pw, vw):
    m, c = _flat(mean, 4).copy(), _flat(cov, 16).copy()
    lib().emu_pt_predict(pw, vw, len(m), _f(m), _f(c))
    return m, c.reshape(-1, 4, 4)


def update(mean, cov, z, pw):
    m, c, z = _flat(mean, 4).copy(), _flat(cov, 16).copy(), _flat(z, 2)
    lib().emu_pt_update(pw, len(m), _f(z), _f(m), _f(c))
    return m, c.reshape(-1, 4, 4)


def distance(mean, cov, z, pw, mode=0):
    m, c, z = _flat(mean, 4), _flat(cov, 16), _flat(z, 2)
    out = np.empty(len(m), f32)
    lib().emu_pt_distance(pw, len(m), _f(z), _f(m), _f(c), mode, _f(out))
    return out


def present(pts, min_score=0.0, mask=None):
    pts = np.ascontiguousarray(pts, f32)
    comps = pts.shape[-1]
    pts = pts.reshape(-1, comps)
    mask = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
    out = np.empty(len(pts), np.uint8)
    lib().emu_pt_present(len(pts), comps, _f(pts), min_score, _b(mask), _b(out))
    return out.astype(bool)


def step(has, mean, cov, z, pres, pw, vw):
    """In place on has [n] u8, mean [n][4], cov [n][16] (C-contiguous f32); -> xy [n][2]."""
    z = _flat(z, 2)
    pres = np.ascontiguousarray(pres, np.uint8).reshape(-1)
    xy = np.empty((len(z), 2), f32)
    lib().emu_pt_step(pw, vw, len(z), _f(z), _b(pres), _b(has), _f(mean), _f(cov), _f(xy))
    return xy
