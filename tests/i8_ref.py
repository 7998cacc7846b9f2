"""Host model of include/similari_i8.h.  An i8 store is an f32 store whose every row was replaced by codes(x) first, so the model is
one function — codes — plus the cell formula on the exact integer dot products and norms; everything else is the existing
restatements (topn_ref, gallery_ref, merge_ref, compat_ref, bestfit_ref) applied to coded rows.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

import merge_ref

FLOOR = np.float32(2.0**-100)   # a row whose absmax lies below is a ZERO ROW


def codes(x):
    """codes(x) of rows [..][D] as f32 integers in -127 .. 127, every step in f32 as the header words it:
    m = max |x_k|; a ZERO ROW (all codes 0) if m == 0, m is not finite (a NaN or an inf anywhere in the row) or m < 2^-100;
    inv = 127.0f / m; q_k = clamp(rint(x_k * inv), -127, 127), rint rounding half to even."""
    x = np.ascontiguousarray(x, np.float32)
    if x.size == 0:
        return x.copy()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        bits = x.view(np.uint32) & np.uint32(0x7FFFFFFF)          # NaN > inf > finite as unsigned integers
        mb = bits.max(axis=-1, keepdims=True)
        m = mb.view(np.float32)
        zero = (mb == 0) | (mb >= np.uint32(0x7F800000)) | (m < FLOOR)
        inv = np.float32(127.0) / np.where(zero, np.float32(1), m).astype(np.float32)
        q = np.clip(np.rint((np.where(zero, np.float32(0), x) * inv).astype(np.float32)), -127, 127)
    return np.where(zero, np.float32(0), q).astype(np.float32) + np.float32(0)   # (-0.0 -> +0.0: a code is an integer)


def code_banks(feats):
    """per-track observation arrays -> the same with every row replaced by its codes"""
    return [None if f is None else codes(f) for f in feats]


def cells_f32(qa, qb):
    """[A][B] f32 cells of two arrays of CODED rows: f32(dot) / sqrtf(f32(na) * f32(nb)) with dot and the norms exact integers
    (int64 here), each converted once; 0 / 0 = NaN for a zero row."""
    a, b = np.asarray(qa).astype(np.int64), np.asarray(qb).astype(np.int64)
    dot = (a @ b.T).astype(np.float32)
    na, nb = (a * a).sum(1).astype(np.float32), (b * b).sum(1).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return dot / np.sqrt((na[:, None] * nb[None, :]).astype(np.float32)).astype(np.float32)


def cells_f64(qa, qb):
    """the same cells in f64 from the exact integers: what the f32 formula is held against"""
    a, b = np.asarray(qa).astype(np.int64), np.asarray(qb).astype(np.int64)
    na, nb = (a * a).sum(1).astype(np.float64), (b * b).sum(1).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (a @ b.T).astype(np.float64) / np.sqrt(na[:, None] * nb[None, :])


def tap(q_feats, s_feats, K, cell=cells_f32):
    """[Q][K][T][K] cells of banks of rows AS GIVEN (coded here), NaN where an observation is absent — the tap of a search"""
    out = np.full((len(q_feats), K, len(s_feats), K), np.nan, np.float64 if cell is cells_f64 else np.float32)
    qs, ss = code_banks(q_feats), code_banks(s_feats)
    for qi, a in enumerate(qs):
        for ti, b in enumerate(ss):
            if len(a) and len(b):
                out[qi, : len(a), ti, : len(b)] = cell(a, b)
    return out


class Model(merge_ref.Model):
    """merge_ref.Model of an i8 store: every row is coded on the way in, nothing else differs."""

    def upsert(self, ids, feats):
        super().upsert(ids, code_banks(feats))

    def append(self, ids, feats, quality=None, keep=merge_ref.LATEST, capacity=None):
        super().append(ids, code_banks(feats), quality, keep, capacity)
