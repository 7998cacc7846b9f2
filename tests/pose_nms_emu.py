"""Builds and binds tests/emu_pose_nms/libemu_pose_nms.so: similari_amd/csrc/sa_pose_nms.h over sa_pose_oks.h compiled by g++ with the
flags of tests/oks_emu.py.  TEST INFRASTRUCTURE, for tests/test_pose_nms_emu.py and scripts/bench_pose_nms.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
EMU_DIR = ROOT / "tests" / "emu_pose_nms"
f32 = np.float32
_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    so = EMU_DIR / "libemu_pose_nms.so"
    csrc = ROOT / "similari_amd" / "csrc"
    srcs = [EMU_DIR / "emu_pose_nms.cpp"] + [csrc / h for h in ("sa_pose_nms.h", "sa_pose_oks.h", "sa_pose_gate.h", "sa_pose.h", "sa_kalman_point.h", "sa_device.h")]
    if not so.exists() or any(s.stat().st_mtime > so.stat().st_mtime for s in srcs):
        subprocess.run(
            ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-o", str(so), str(EMU_DIR / "emu_pose_nms.cpp")],
            check=True,
        )
    L = C.CDLL(str(so))
    fp, bp, up, u32 = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.c_uint32
    L.emu_pose_nms.restype = None
    L.emu_pose_nms.argtypes = [u32, u32, u32, fp, bp, C.c_float, fp, fp, u32, C.c_float, C.c_float, up, up, fp, up, up]
    _lib = L
    return L


def nms(pts, scores, sigmas, nms_threshold=0.9, score_threshold=None, min_common=1, present=None, min_score=None, want_matrix=False):
    """tests/pose_nms_ref.nms by the compiled header -> keep; want_matrix: (keep, order, w)"""
    fp, bp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    pts = np.ascontiguousarray(pts, f32)
    m, P, comps = pts.shape
    sc, sig = np.ascontiguousarray(scores, f32).reshape(-1), np.ascontiguousarray(sigmas, f32).reshape(-1)
    assert len(sc) == m and len(sig) == P
    mask = None if present is None else np.ascontiguousarray(np.asarray(present).reshape(m, P) != 0, np.uint8)
    order, keep = np.zeros(max(m, 1), np.uint32), np.zeros(max(m, 1), np.uint32)
    w = np.zeros((max(m, 1), max(m, 1)), f32) if want_matrix else None
    n_order, n_keep = C.c_uint32(), C.c_uint32()
    lib().emu_pose_nms(m, P, comps, pts.ctypes.data_as(fp), None if mask is None else mask.ctypes.data_as(bp),
                       0.0 if min_score is None else min_score, sc.ctypes.data_as(fp), sig.ctypes.data_as(fp), min_common, nms_threshold,
                       float("nan") if score_threshold is None else score_threshold, order.ctypes.data_as(up), C.byref(n_order),
                       None if w is None else w.ctypes.data_as(fp), keep.ctypes.data_as(up), C.byref(n_keep))
    keep = keep[: n_keep.value].copy()
    if not want_matrix:
        return keep
    k = n_order.value
    return keep, order[:k].copy(), w.reshape(-1)[: k * k].reshape(k, k).copy()
