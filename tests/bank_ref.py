"""A plain numpy model of a track's feature bank under VisualMetric::optimize (visual_sort/metric.rs:297-374) with
optimize_observations (metric.rs:129-154) and feature_can_be_used (metric.rs:227-249), as the device-side upkeep step applies it to
one candidate.  Nothing here calls the library: the header's sa_bank_policy / sa_feature_can_be_used (tests/test_bank_ref.py) and the
kernels behind sa_tracks_apply* (tests/test_gpu_bank_upkeep.py) are held against it.

A bank is K slots in observation order, slot 0 the newest observation.  A slot holds a feature row (present = 1), or the newest
observation that came without a usable feature (present = 0, its quality kept, a zero row), or nothing (present = 0, quality 0, a zero
row)."""
import numpy as np

NEW = "new"      # the slot takes the candidate's observation
EMPTY = None     # the slot holds nothing
f32 = np.float32


def feature_can_be_used(minimal_area, aspect, height, q, min_q, own, min_own):
    """metric.rs:227-249 in f32: the quality gate, the own-area gate (own = None: no share given, the gate is open) and the box area
    (bbox.rs:163-166: w = height * aspect, area = w * height) against minimal_area."""
    quality_ok = f32(q) >= f32(min_q)
    perc_ok = True if own is None else f32(own) >= f32(min_own)
    w = f32(height) * f32(aspect)
    bbox_ok = f32(w * f32(height)) >= f32(minimal_area)
    return bool(bbox_ok and quality_ok and perc_ok)


def policy(K, present, quality):
    """optimize_observations + push + swap(0, len - 1) on the bank's bookkeeping: the source of every slot after a MERGE — an old slot
    index, NEW or EMPTY — and the number of slots in use.
      retain those with a feature; stable sort by quality descending; len >= K: drop the last; push the new one; swap first and last."""
    kept = [k for k in range(K) if present[k]]
    kept.sort(key=lambda k: -float(f32(quality[k])))          # list.sort is stable, as Vec::sort_by is
    if len(kept) >= K:
        kept.pop()
    kept.append(NEW)
    kept[0], kept[-1] = kept[-1], kept[0]
    return kept + [EMPTY] * (K - len(kept)), len(kept)


class Bank:
    """rows [K, D] f32, present [K] u8, quality [K] f32 in slot order; count = slots that hold a feature."""

    def __init__(self, K, D):
        self.K, self.D = K, D
        self.rows = np.zeros((K, D), np.float32)
        self.present = np.zeros(K, np.uint8)
        self.quality = np.zeros(K, np.float32)
        self.src = [EMPTY] * K      # where the last step took every slot from

    @property
    def count(self):
        return int(self.present.sum())

    def copy(self):
        b = Bank(self.K, self.D)
        b.rows, b.present, b.quality, b.src = self.rows.copy(), self.present.copy(), self.quality.copy(), list(self.src)
        return b


def step(bank, merged, feature, quality, aspect, height, own, minimal_area, q_collect, own_collect):
    """One candidate's observation into its destination track's bank.  bank: the track's Bank (ignored for a new track: merged = False);
    feature: the candidate's row [D] or None; quality: its feature quality; aspect, height: its box; own: its own-area share or None.
    A new track keeps its observation as it came; a merge keeps the feature only if it may be collected.  Returns the new Bank, .src
    telling where every slot came from."""
    K, D = bank.K, bank.D
    has = feature is not None
    keep = has
    if merged:
        keep = has and feature_can_be_used(minimal_area, aspect, height, quality, q_collect, own, own_collect)
        src, _ = policy(K, bank.present, bank.quality)
    else:
        src = [NEW] + [EMPTY] * (K - 1)
    out = Bank(K, D)
    out.src = src
    for k, s in enumerate(src):
        if s is EMPTY:
            continue
        if s == NEW:
            out.present[k] = 1 if keep else 0
            out.quality[k] = f32(quality)
            if keep:
                out.rows[k] = np.asarray(feature, np.float32)
        else:
            out.present[k] = 1
            out.quality[k] = bank.quality[s]
            out.rows[k] = bank.rows[s]
    return out
