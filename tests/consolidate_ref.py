"""Host restatement of steps 2 and 3 of include/similari_consolidate.h, on top of tests/merge_ref.py.  Nothing here calls the library.

    winner_of(ids, out_n, out_winner)   w(a): entry 0's winner, or a itself
    pairs(ids, out_n, out_winner)       the mutual pairs [(destination id, source id), ...] in the order of `ids`, and out_dest
    consolidate(model, ...)             the pairs merged in a merge_ref.Model: banks, qualities, attributes, order after removal
"""
import numpy as np


def winner_of(ids, out_n, out_winner):
    """{a: w(a)}: out_winner[a][0] if out_n[a] >= 1, else a's own id."""
    win = np.asarray(out_winner).reshape(len(ids), -1) if len(ids) else np.zeros((0, 1), np.uint64)
    return {int(a): int(win[i, 0]) if out_n[i] >= 1 else int(a) for i, a in enumerate(ids)}


def pairs(ids, out_n, out_winner):
    """-> ([(dst, src), ...] with dst < src, destinations in the order of ids; out_dest [T])."""
    w = winner_of(ids, out_n, out_winner)
    found, dest = [], [int(a) for a in ids]
    at = {int(a): i for i, a in enumerate(ids)}
    for a in (int(x) for x in ids):
        b = w[a]
        if b != a and b in w and w[b] == a and a < b:
            found.append((a, b))
            dest[at[b]] = a
    return found, np.array(dest, np.uint64)


def union(dst, src):
    """Track::merge on (key, start, end): the destination keeps its key and spans both."""
    return (dst[0], min(dst[1], src[1]), max(dst[2], src[2]))


def consolidate(model, attrs, ids, out_n, out_winner, keep, capacity=None, ruled=False):
    """model: a merge_ref.Model holding the banks with their qualities, attrs: {id: (key, start, end)}.  The mutual pairs of the join
    outputs merge (bank = dst ++ src, the rule always runs, the sources leave in pair order).  -> (pairs, out_dest, model after,
    attrs after); the order after removal is the model's."""
    found, dest = pairs(ids, out_n, out_winner)
    after = model.copy()
    new_attrs = dict(attrs)
    if found:
        after.merge({d: [s] for d, s in found}, keep, capacity)
    for d, s in found:
        if ruled:
            new_attrs[d] = union(new_attrs[d], new_attrs[s])
        del new_attrs[s]
    return found, dest, after, new_attrs
