"""Host restatement of include/similari_attrs.h, composed from topn_ref / gallery_ref / merge_ref.  Test infrastructure only.

Attributes are (key, start, end) tuples of Python ints; a rule is (flags, ready_at).  A dead pair is the reference's
Err(IncompatibleAttributes) that TrackStore drops (src/track.rs:609, src/track/store.rs:217-219), or a stored track the only_baked
gate passes over (store.rs:222-238): it yields no distance.  In topn_ref NaN is "absent" — it neither raises M nor is kept — which
is exactly that, so every form here sets the cells of dead pairs to NaN and hands over to the plain restatement."""
from __future__ import annotations

import math

import numpy as np

import gallery_ref as G
import merge_ref
import topn_ref as R

f32 = np.float32
SAME_KEY, DISJOINT, QUERY_FIRST, ONLY_READY = 1, 2, 4, 8
INT64_MIN, INT64_MAX = -(2**63), 2**63 - 1
NO_RULE = (0, INT64_MAX)
ZERO = (0, 0, 0)


def live(flags, ready_at, q, t):
    """q: the query's (key, start, end) — self in self.compatible(other) — t: the stored track's."""
    ok = True
    if flags & SAME_KEY:
        ok = ok and q[0] == t[0]
    if flags & DISJOINT:
        ok = ok and (q[1] >= t[2] or q[2] <= t[1])
    if flags & QUERY_FIRST:
        ok = ok and q[2] <= t[1]
    if flags & ONLY_READY:
        ok = ok and t[2] <= ready_at
    return ok


def live_matrix(rule, q_attrs, s_attrs):
    """[Q][T] bool"""
    out = np.zeros((len(q_attrs), len(s_attrs)), bool)
    for i, q in enumerate(q_attrs):
        for j, t in enumerate(s_attrs):
            out[i, j] = live(rule[0], rule[1], q, t)
    return out


def mask_dead(cells, rule, q_attrs, s_attrs):
    """A copy of the cell matrix [Q][K][T][K] with the cells of dead pairs absent."""
    cells = np.array(cells, f32, copy=True)
    dead = ~live_matrix(rule, q_attrs, s_attrs)
    cells[np.broadcast_to(dead[:, None, :, None], cells.shape)] = np.nan
    return cells


def pairs(q_ids, s_ids, cells, rule, q_attrs, s_attrs, keep_below=math.inf):
    """The distances the reference's foreign_track_distances returns: (query, stored, d) triples."""
    return R.pair_metrics(q_ids, s_ids, mask_dead(cells, rule, q_attrs, s_attrs), keep_below)


def restate(q_ids, s_ids, cells, rule, q_attrs, s_attrs, topn, max_distance, min_votes=1, keep_below=math.inf):
    """sa_store_search_topn_compat on that call's own tap cells -> ({query: [(winner, weight), ...]}, M)"""
    return R.restate(q_ids, s_ids, mask_dead(cells, rule, q_attrs, s_attrs), topn, max_distance, min_votes, keep_below)


def attrs_of(s_ids, s_attrs, ids):
    """The stored attributes of `ids`; an id the store does not hold is a query without observations, its attributes {0, 0, 0}."""
    at = {int(i): a for i, a in zip(s_ids, s_attrs)}
    return [at.get(int(i), ZERO) for i in ids]


def search_stored(s_ids, cells, ids, rule, s_attrs, topn, max_distance, min_votes=1, keep_below=math.inf, withdraw=False):
    """sa_store_search_stored_compat: cells [n][K][T][K] of the call; the queries carry their stored attributes."""
    masked = mask_dead(cells, rule, attrs_of(s_ids, s_attrs, ids), s_attrs)
    return G.search_stored(s_ids, masked, ids, topn, max_distance, min_votes, keep_below, withdraw)


def join(s_ids, cells, rule, s_attrs, topn, max_distance, min_votes=1, keep_below=math.inf):
    """sa_store_join_topn_compat: cells [T][K][T][K]; each direction of a pair under its own live(query, stored)."""
    return search_stored(s_ids, cells, s_ids, rule, s_attrs, topn, max_distance, min_votes, keep_below)


def surviving_pairs(s_ids, cells, rule, s_attrs, max_distance, min_votes=1, keep_below=math.inf):
    """The unordered pairs of stored ids with at least one live surviving direction (sa_join_stats.blocks counts them)."""
    res, _ = join(s_ids, cells, rule, s_attrs, G.ALL, max_distance, min_votes, keep_below)
    return {frozenset((q, w)) for q, lst in res.items() for w, _ in lst}


TILE = {"cosine": (64, 64), "euclidean": (32, 128)}   # rows x columns of a launch-1 tile, in observation slots


def dead_tiles(kind, Kp, rule, q_attrs, s_attrs, join=False):
    """-> (tiles launch 1 runs, tiles among them without a live group).  A group is one (query track, stored track) pair of Kp x Kp
    slots; only the rule decides (a self pair or a withdrawn column is an ordinary group here, as in the kernels).  join: q_attrs is
    s_attrs, the tiles are those on or above the diagonal (n0 + BN > m0), a tile owns the groups with q < t and a group is live when
    either direction is."""
    bm, bn = TILE[kind]
    gr, gc = bm // Kp, bn // Kp
    lv = live_matrix(rule, q_attrs, s_attrs)
    if join:
        lv = np.triu(lv | lv.T, 1)
    Q, T = lv.shape
    tiles = dead = 0
    for i in range(-(-Q * Kp // bm)):
        for j in range(-(-T * Kp // bn)):
            if join and not (j + 1) * bn > i * bm:
                continue
            tiles += 1
            dead += not lv[i * gr: (i + 1) * gr, j * gc: (j + 1) * gc].any()
    return tiles, dead


class Incompatible(Exception):
    pass


def merged_attrs(rule, dst, srcs):
    """Track::merge's attribute part for one destination: the sources in order against the destination as merged so far; with rule
    bits set an incompatible source raises (CamTrackingAttributes::merge), without it is the union (TimeAttrs::merge)."""
    run = tuple(dst)
    for s in srcs:
        if rule[0] and not live(rule[0], rule[1], run, s):
            raise Incompatible((run, tuple(s)))
        run = (run[0], min(run[1], s[1]), max(run[2], s[2]))
    return run


class Model(merge_ref.Model):
    """merge_ref.Model whose tracks carry attributes: {0, 0, 0} at birth, kept by a replaced bank, dropped with the track."""

    def __init__(self, K, D):
        super().__init__(K, D)
        self.attrs = {}

    def copy(self):
        m = Model(self.K, self.D)
        m.order, m.banks, m.attrs = list(self.order), {i: list(b) for i, b in self.banks.items()}, dict(self.attrs)
        return m

    def _born(self):
        for i in self.order:
            self.attrs.setdefault(i, ZERO)

    def upsert(self, ids, feats):
        super().upsert(ids, feats)
        self._born()

    def append(self, *a, **kw):
        super().append(*a, **kw)
        self._born()

    def remove(self, ids):
        super().remove(ids)
        for i in ids:
            self.attrs.pop(int(i), None)

    def set_attrs(self, ids, attrs):
        for i, a in zip(ids, attrs):
            self.attrs[int(i)] = tuple(int(x) for x in a)

    def merge(self, pairs, keep=merge_ref.LATEST, capacity=None, rule=None):
        """rule None: plain sa_store_merge (the destination's attributes stay).  Raises Incompatible before anything changes."""
        if rule is not None:
            new = {int(d): merged_attrs(rule, self.attrs[int(d)], [self.attrs[int(s)] for s in srcs]) for d, srcs in pairs.items()}
            self.attrs.update(new)
        super().merge(pairs, keep, capacity)

    def attrs_in_order(self):
        return [self.attrs[i] for i in self.order]
