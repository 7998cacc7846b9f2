"""Host restatement of include/similari_absorb.h: steps 1-4 composed from bestfit_ref (the vote) and merge_ref (the append), and
nothing else.  Test infrastructure only.

    decide(q_ids, res)     step 2: {query: destination} from a BestFit result — only entry 0 acts
    Model                  a merge_ref.Model with attributes; absorb() runs steps 1-4 on it
"""
import math

import numpy as np

import bestfit_ref as B
import merge_ref as M

f32 = np.float32


def cells_of(model, q_feats, kind):
    """The distance cells [Q][K][T][K] of the queries against the model's banks (NaN = absent), f32 arithmetic in plain order: what
    bestfit_ref.restate takes.  euclidean: sqrt(sum (x - y)^2); cosine: the similarity x.y / sqrt(|x|^2 |y|^2), as the reference names it."""
    K, T = model.K, len(model.order)
    out = np.full((len(q_feats), K, T, K), np.nan, f32)
    for qi, qf in enumerate(q_feats):
        for a, x in enumerate(np.asarray(qf, f32).reshape(-1, model.D)):
            for ti, t in enumerate(model.order):
                for b, (y, _) in enumerate(model.banks[t]):
                    if kind == "euclidean":
                        out[qi, a, ti, b] = np.sqrt(((x - y) ** 2).sum(dtype=f32))
                    else:
                        out[qi, a, ti, b] = (x * y).sum(dtype=f32) / np.sqrt((x * x).sum(dtype=f32) * (y * y).sum(dtype=f32))
    return out


def decide(q_ids, res):
    """Step 2.  res: {query: [(winner, weight, track), ...]} of the BestFit call.  A query is matched iff it has an entry and entry
    0's winner is not the query itself."""
    dest = {}
    for q in q_ids:
        q = int(q)
        lst = res.get(q, [])
        dest[q] = int(lst[0][0]) if lst and int(lst[0][0]) != q else q
    return dest


class Model(M.Model):
    def __init__(self, K, D, kind="euclidean"):
        super().__init__(K, D)
        self.kind = kind
        self.attrs = {}   # id -> (key, start, end)

    def absorb(self, q_ids, q_feats, topn, max_distance, min_votes=1, keep_below=math.inf, quality=None, capacity=None, rule=None, q_attrs=None):
        """-> (res cut at topn, {query: destination}).  rule: a compat_ref rule or None; q_attrs: [(key, start, end)] with a rule."""
        q_ids = [int(q) for q in q_ids]
        assert not set(q_ids) & set(self.order), "a query id that the store holds is refused"
        cells = cells_of(self, q_feats, self.kind)
        if rule is None:
            res, _, _ = B.restate(q_ids, self.order, cells, max_distance, min_votes, keep_below) if self.order else ({}, 0, 0)
        else:
            s_attrs = [self.attrs.get(t, (0, 0, 0)) for t in self.order]
            res, _, _ = B.restate_compat(q_ids, self.order, cells, rule, q_attrs, s_attrs, max_distance, min_votes, keep_below) if self.order else ({}, 0, 0)
        dest = decide(q_ids, res)
        held = set(self.order)
        cap = capacity
        if isinstance(capacity, dict):   # per query -> per destination, as the one append sees it
            cap = [capacity.get(q, self.K) for q in q_ids]
        self.append([dest[q] for q in q_ids], q_feats, quality, M.LATEST, cap)
        if rule is not None:
            for q, a in zip(q_ids, q_attrs):
                d = dest[q]
                if d in held:
                    k, s, e = self.attrs.get(d, (0, 0, 0))
                    self.attrs[d] = (k, min(s, a[1]), max(e, a[2]))
                else:
                    self.attrs[d] = tuple(a)
        return B.cut(res, topn), dest
