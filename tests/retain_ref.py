"""Host restatement of include/similari_retain.h: absorb_ref.Model whose absorb takes the retention rule and hands it to
merge_ref.Model.append, and nothing else; and ranks(), the numpy statement of the rank k_absorb_move_best gives an observation.
Test infrastructure only."""
import math

import numpy as np

import absorb_ref as A
import bestfit_ref as B
import merge_ref as M

f32 = np.float32


def ranks(q):
    """q: the qualities of a combined bank in bank order (no NaN).  rank[i] = #{j: q[j] > q[i]} + #{j < i: q[j] == q[i]}, in float
    compares (-0.0 == 0.0): the place a stable sort by quality descending gives observation i."""
    q = np.asarray(q, f32)
    i = np.arange(len(q))
    above = q[None, :] > q[:, None]
    tied_before = (q[None, :] == q[:, None]) & (i[None, :] < i[:, None])
    return (above | tied_before).sum(axis=1)


class Model(A.Model):
    def absorb(self, q_ids, q_feats, topn, max_distance, min_votes=1, keep_below=math.inf, quality=None, capacity=None, rule=None, q_attrs=None,
               keep=M.BEST):
        """absorb_ref.Model.absorb with step 3 under `keep`."""
        q_ids = [int(q) for q in q_ids]
        assert not set(q_ids) & set(self.order), "a query id that the store holds is refused"
        cells = A.cells_of(self, q_feats, self.kind)
        if rule is None:
            res, _, _ = B.restate(q_ids, self.order, cells, max_distance, min_votes, keep_below) if self.order else ({}, 0, 0)
        else:
            s_attrs = [self.attrs.get(t, (0, 0, 0)) for t in self.order]
            res, _, _ = B.restate_compat(q_ids, self.order, cells, rule, q_attrs, s_attrs, max_distance, min_votes, keep_below) if self.order else ({}, 0, 0)
        dest = A.decide(q_ids, res)
        held = set(self.order)
        cap = [capacity.get(q, self.K) for q in q_ids] if isinstance(capacity, dict) else capacity
        self.append([dest[q] for q in q_ids], q_feats, quality, keep, cap)
        if rule is not None:
            for q, a in zip(q_ids, q_attrs):
                d = dest[q]
                if d in held:
                    k, s, e = self.attrs.get(d, (0, 0, 0))
                    self.attrs[d] = (k, min(s, a[1]), max(e, a[2]))
                else:
                    self.attrs[d] = tuple(a)
        return B.cut(res, topn), dest
