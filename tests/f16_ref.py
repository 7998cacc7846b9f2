"""Host model of include/similari_f16.h.  An f16 store is an f32 store whose every feature value was replaced by f16(x) first, so the
model is one function — round_f16 — and everything else is the existing restatements (topn_ref, gallery_ref, merge_ref, compat_ref,
bestfit_ref) applied to rounded rows, plus the f64 cells both metrics are held against and the flag rule of the euclidean expansion.
Test infrastructure only."""
from __future__ import annotations

import numpy as np

import merge_ref

# The f16 matrix instruction of gfx950 takes subnormal inputs as they are, so the pad kernel keeps them and so does
# the model.
FLUSH_SUBNORMALS = False


def round_f16(x):
    """f16(x) widened back to f32: the IEEE binary16 conversion, round-to-nearest-even, written on the f32 bit pattern.  Overflow
    (|x| >= 65520) goes to +-inf, a NaN stays a NaN, results below 2^-14 are multiples of 2^-24 (subnormals are kept)."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    sign, a = u & 0x80000000, u & 0x7FFFFFFF
    normal = ((a + 0xFFF + ((a >> 13) & 1)) >> 13) << 13                       # 10 mantissa bits kept, ties to even, carries into the exponent
    with np.errstate(invalid="ignore"):
        mag = a.astype(np.uint32).view(np.float32).astype(np.float64)
        small = (np.rint(np.where(np.isfinite(mag), mag, 0.0) * 2.0**24) * 2.0**-24).astype(np.float32)   # rint: half to even; both products exact
    if FLUSH_SUBNORMALS:
        small = np.where(small < np.float32(2.0**-14), np.float32(0), small)
    r = np.where(a < 0x38800000, small.view(np.uint32).astype(np.uint64), normal)   # below 2^-14
    r = np.where(a >= 0x477FF000, 0x7F800000, r)                               # 65520 and beyond, inf
    r = np.where(a > 0x7F800000, 0x7FC00000 | (a & 0x003FE000), r)             # NaN: quiet, the payload's upper bits
    return (r | sign).astype(np.uint32).view(np.float32).reshape(x.shape)


def round_banks(feats):
    """per-track observation arrays -> the same with every row rounded"""
    return [None if f is None else round_f16(f) for f in feats]


def rho(D):
    """the flag threshold of a store of feature length D, as the host computes it in f32: 5e-3 sqrt(Dp)"""
    Dp = -(-int(D) // 32) * 32
    return np.float32(5e-3) * np.sqrt(np.float32(Dp))


def cells_f64(kind, q_feats, s_feats, K):
    """[Q][K][T][K] f64 cells of the rows as given (round them first), NaN where an observation is absent — the cells a search returns
    through the tap.  cosine: dot / sqrt(|a|^2 |b|^2) (NaN with a zero norm); euclidean: sqrt(sum (a - b)^2)."""
    out = np.full((len(q_feats), K, len(s_feats), K), np.nan, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for qi, qf in enumerate(q_feats):
            a = np.asarray(qf, np.float64)
            for ti, sf in enumerate(s_feats):
                b = np.asarray(sf, np.float64)
                if len(a) and len(b):
                    if kind == "cosine":
                        na, nb = (a * a).sum(1), (b * b).sum(1)
                        out[qi, : len(a), ti, : len(b)] = (a @ b.T) / np.sqrt(na[:, None] * nb[None, :])
                    else:
                        out[qi, : len(a), ti, : len(b)] = np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(2))
    return out


def flag_ratio(q_feats, s_feats, K):
    """[Q][K][T][K] f64: d^2 / (|a|^2 + |b|^2) of the rows as given, the quantity the expansion compares with rho (NaN: absent, or
    both rows zero)"""
    out = np.full((len(q_feats), K, len(s_feats), K), np.nan, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for qi, qf in enumerate(q_feats):
            a = np.asarray(qf, np.float64)
            for ti, sf in enumerate(s_feats):
                b = np.asarray(sf, np.float64)
                if len(a) and len(b):
                    s = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :]
                    out[qi, : len(a), ti, : len(b)] = ((a[:, None, :] - b[None, :, :]) ** 2).sum(2) / s
    return out


class Model(merge_ref.Model):
    """merge_ref.Model of an f16 store: every row is rounded on the way in, nothing else differs."""

    def upsert(self, ids, feats):
        super().upsert(ids, round_banks(feats))

    def append(self, ids, feats, quality=None, keep=merge_ref.LATEST, capacity=None):
        super().append(ids, round_banks(feats), quality, keep, capacity)
