"""Device memory for in-process tests, without torch: hipMalloc / hipMemcpy / hipFree / hipDeviceSynchronize of the one libamdhip64
image the process has mapped (the engine's), so that it does not matter which context came first."""
import ctypes as C

import numpy as np

from similari_amd import abi

_H2D, _D2H = 1, 2
_hip = None


def hip():
    global _hip
    if _hip is None:
        paths = abi.hip_runtimes_mapped()
        assert len(paths) == 1, "load the engine's library first; exactly one HIP runtime may be mapped: %r" % (paths,)
        _hip = C.CDLL(paths[0])
        _hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _hip.hipFree.argtypes = [C.c_void_p]
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipSetDevice.argtypes = [C.c_int]
        for f in (_hip.hipMalloc, _hip.hipFree, _hip.hipMemcpy, _hip.hipDeviceSynchronize, _hip.hipSetDevice):
            f.restype = C.c_int
    return _hip


def _chk(rc, what):
    assert rc == 0, "%s failed: hipError %d" % (what, rc)


def malloc(nbytes, device=0) -> int:
    _chk(hip().hipSetDevice(device), "hipSetDevice")
    p = C.c_void_p()
    _chk(hip().hipMalloc(C.byref(p), max(int(nbytes), 1)), "hipMalloc")
    return int(p.value)


def free(ptr):
    _chk(hip().hipFree(C.c_void_p(ptr)), "hipFree")


def upload(ptr, array):
    """The bytes of a contiguous numpy array to device address ptr; returns after the copy is done."""
    a = np.ascontiguousarray(array)
    if a.nbytes:
        _chk(hip().hipMemcpy(C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, _H2D), "hipMemcpy")
    _chk(hip().hipDeviceSynchronize(), "hipDeviceSynchronize")


def download(ptr, nbytes) -> np.ndarray:
    out = np.zeros(int(nbytes), np.uint8)
    if nbytes:
        _chk(hip().hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), int(nbytes), _D2H), "hipMemcpy")
    return out
