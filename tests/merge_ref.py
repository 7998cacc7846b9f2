"""Host restatement of include/similari_merge.h: a feature store as an ordered list of ids with, per id, the ORDERED list of its
observations (feature row, quality).  Plain Python on purpose, and the append runs the rule after every single observation, as the
reference does (Track::add_observation calls optimize each time), so that the library's once-per-call is checked against it.

    optimize(bank, keep, C)      the two retention rules
    Model                        upsert / remove / append / merge as the library documents them, with the store's slot order
"""
import math

import numpy as np

LATEST, BEST = "latest", "best"


def optimize(bank, keep, C):
    """bank: list of (row, quality).  latest: reverse, truncate(C), reverse.  best: stable sort by quality descending, truncate(C)."""
    bank = list(bank)
    if keep == LATEST:
        bank.reverse()
        del bank[C:]
        bank.reverse()
        return bank
    assert keep == BEST
    assert not any(math.isnan(q) for _, q in bank), "the reference panics on a NaN quality"
    out = []
    for ob in bank:   # insertion keeps earlier-first among equals: go past everything that is >= (-0.0 == 0.0 in float compare)
        k = len(out)
        while k > 0 and out[k - 1][1] < ob[1]:
            k -= 1
        out.insert(k, ob)
    del out[C:]
    return out


def growth_capacity(merges, initial=4, extension=1.5, most=12):
    """examples/track_merging.rs:288-293: the capacity after `merges` merges."""
    return min(int(np.float32(initial) * np.float32(extension) ** np.float32(merges)), most)


class Model:
    def __init__(self, K, D):
        self.K, self.D = K, D
        self.order = []   # slot -> id
        self.banks = {}   # id -> [(row [D] f32, quality f32), ...]

    def copy(self):
        m = Model(self.K, self.D)
        m.order = list(self.order)
        m.banks = {i: list(b) for i, b in self.banks.items()}
        return m

    def _cap(self, capacity, i, key):
        if capacity is None:
            return self.K
        if isinstance(capacity, dict):
            return capacity.get(key, self.K)
        return int(capacity) if np.ndim(capacity) == 0 else int(capacity[i])

    def upsert(self, ids, feats):
        for i, f in zip(ids, feats):
            i = int(i)
            if i not in self.banks:
                self.order.append(i)
            self.banks[i] = [(np.asarray(r, np.float32), np.float32(0)) for r in np.asarray(f, np.float32).reshape(-1, self.D)]

    def remove(self, ids):
        """the last track moves into the hole; unknown ids are ignored"""
        for i in ids:
            i = int(i)
            if i not in self.banks:
                continue
            k = self.order.index(i)
            self.order[k] = self.order[-1]
            self.order.pop()
            del self.banks[i]

    def append(self, ids, feats, quality=None, keep=LATEST, capacity=None):
        for n, (i, f) in enumerate(zip(ids, feats)):
            i = int(i)
            rows = np.zeros((0, self.D), np.float32) if f is None else np.asarray(f, np.float32).reshape(-1, self.D)
            q = np.zeros(len(rows), np.float32) if quality is None or quality[n] is None else np.asarray(quality[n], np.float32)
            if i not in self.banks:
                self.order.append(i)
                self.banks[i] = []
            for r, x in zip(rows, q):
                self.banks[i] = optimize(self.banks[i] + [(r, np.float32(x))], keep, self._cap(capacity, n, i))

    def merge(self, pairs, keep=LATEST, capacity=None):
        for n, (d, srcs) in enumerate(pairs.items()):
            bank = list(self.banks[int(d)])
            for s in srcs:
                bank += self.banks[int(s)]
            self.banks[int(d)] = optimize(bank, keep, self._cap(capacity, n, int(d)))
        self.remove([s for srcs in pairs.values() for s in srcs])

    def feats(self, i):
        b = self.banks[int(i)]
        return np.stack([r for r, _ in b]) if b else np.zeros((0, self.D), np.float32)

    def quality(self, i):
        return np.array([q for _, q in self.banks[int(i)]], np.float32)
