"""What include/similari_devrows.h says in words, in numpy: widen on bit patterns, the source-row table, the span of a descriptor."""
import numpy as np

NONE = 0xFFFFFFFF
ELEM_F32, ELEM_BF16, ELEM_F16 = 0, 1, 2
ELEM_BYTES = {ELEM_F32: 4, ELEM_BF16: 2, ELEM_F16: 2}


def widen_bf16(bits):
    """bf16 bit patterns (uint16) -> the f32 values they stand for: the pattern is the upper half of the f32's."""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def widen_f16(bits):
    """binary16 bit patterns (uint16) -> f32, exactly: a subnormal is m 2^-24, inf and NaN keep sign and payload (upper mantissa bits)."""
    h = np.asarray(bits, np.uint16).astype(np.uint32)
    sign, ex, m = (h & 0x8000) << 16, (h >> 10) & 31, h & 0x3FF
    sub = (m.astype(np.float32) * np.float32(2.0 ** -24)).view(np.uint32)
    out = np.where(ex == 31, 0x7F800000 | (m << 13), np.where(ex == 0, sub, ((ex + 112) << 23) | (m << 13)))
    return (sign | out).astype(np.uint32).view(np.float32)


def widen(bits_or_f32, elem):
    """The f32 rows a host call must be fed for the source array of a *_dev call (uint16 bit patterns, or f32 as it is)."""
    if elem == ELEM_F32:
        return np.asarray(bits_or_f32, np.float32)
    return widen_bf16(bits_or_f32) if elem == ELEM_BF16 else widen_f16(bits_or_f32)


def row_table(n_obs, index, Kp):
    """[n * Kp] u32: the source row of observation k of track i at i * Kp + k — index[off], or off, with off counting the call's
    observations in order —, NONE for an absent row."""
    n_obs = np.asarray(n_obs, np.uint32).reshape(-1)
    t = np.full(len(n_obs) * Kp, NONE, np.uint32)
    off = 0
    for i, m in enumerate(n_obs):
        for k in range(int(m)):
            t[i * Kp + k] = off if index is None else index[off]
            off += 1
    return t


def span_bytes(n_rows, row_stride, D, elem):
    """Bytes from base that a descriptor's rows may touch: ((n_rows - 1) * row_stride + D) * elem_size."""
    return ((int(n_rows) - 1) * int(row_stride) + int(D)) * ELEM_BYTES[elem]


def wide_bytes(src, dst, D):
    """The width of the one load per lane and step a row takes when its address is a multiple of it (0: no wide route)."""
    if dst != ELEM_F32:
        return 4 if src != ELEM_F32 else 8
    if D % 4:
        return 0
    return 8 if src != ELEM_F32 else 16


def wide_rows(base, row_stride, table, src, dst, D):
    """How many of the table's rows lie at an address that allows the wide load."""
    w = wide_bytes(src, dst, D)
    rows = [int(t) for t in np.asarray(table).reshape(-1) if int(t) != NONE]
    return sum(1 for t in rows if w and (int(base) + t * int(row_stride) * ELEM_BYTES[src]) % w == 0)
