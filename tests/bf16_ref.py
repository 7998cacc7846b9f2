"""Host model of include/similari_bf16.h.  A bf16 store is an f32 store whose every feature value was replaced by bf16(x) first, so
the model is one function — round_bf16 — and everything else is the existing restatements (topn_ref, gallery_ref, merge_ref,
compat_ref, bestfit_ref) applied to rounded rows.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

import merge_ref


def round_bf16(x):
    """bf16(x) widened back to f32: round-to-nearest-even on the bit pattern, u + 0x7fff + ((u >> 16) & 1), upper 16 bits kept.
    For finite values whose rounding is finite."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(x.shape)


def round_banks(feats):
    """per-track observation arrays -> the same with every row rounded"""
    return [None if f is None else round_bf16(f) for f in feats]


def cosine_f64(q_feats, s_feats, K):
    """[Q][K][T][K] f64: dot / sqrt(|a|^2 |b|^2) of the rows as given (round them first), NaN where an observation is absent or a
    norm is zero — the cells a search returns through the tap."""
    out = np.full((len(q_feats), K, len(s_feats), K), np.nan, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for qi, qf in enumerate(q_feats):
            a = np.asarray(qf, np.float64)
            for ti, sf in enumerate(s_feats):
                b = np.asarray(sf, np.float64)
                if len(a) and len(b):
                    na, nb = (a * a).sum(1), (b * b).sum(1)
                    out[qi, : len(a), ti, : len(b)] = (a @ b.T) / np.sqrt(na[:, None] * nb[None, :])
    return out


class Model(merge_ref.Model):
    """merge_ref.Model of a bf16 store: every row is rounded on the way in, nothing else differs."""

    def upsert(self, ids, feats):
        super().upsert(ids, round_banks(feats))

    def append(self, ids, feats, quality=None, keep=merge_ref.LATEST, capacity=None):
        super().append(ids, round_banks(feats), quality, keep, capacity)
