"""Host restatement of include/similari_bestfit.h: steps 1-7 as topn_ref / gallery_ref / compat_ref state them — every weight here
is one of theirs, so the two votes cannot drift — then steps 8b-10b (BestFitVoting::winners, src/track/voting/best.rs:52-128).  Test
infrastructure only.

Every form returns (res, groups, claimed): res = {query: [(winner, weight, track), ...]} with each query's FULL list (cut() takes
the first topn), groups = ordered surviving groups of the call, claimed = stored tracks with a claimant."""
from __future__ import annotations

import math

import compat_ref as X
import gallery_ref as G
import topn_ref as R

ALL = G.ALL


def claim(lists):
    """Steps 8b-10b on {query: [(track, weight), ...]} (every surviving group of the call, each query's in TopN order): one list
    ranked by weight descending, query id ascending, stored id ascending; a stored track belongs to the first group that names it;
    every later group that names it has its winner replaced by the query's own id (best.rs:112-119)."""
    ranked = sorted((-w, q, t) for q, lst in lists.items() for t, w in lst)
    holder = {}
    for _, q, t in ranked:
        holder.setdefault(t, q)
    res = {q: [(t if holder[t] == q else q, w, t) for t, w in lst] for q, lst in lists.items() if lst}
    return res, len(ranked), len(holder)


def cut(res, topn):
    return {q: lst[: int(topn)] for q, lst in res.items()}


def from_triples(metrics, max_distance, min_votes=1):
    """BestFitVoting::winners over (query, winner, distance | None) triples, as topn_ref.winners takes them."""
    return claim(R.winners(metrics, ALL, max_distance, min_votes)[0])


def restate(q_ids, s_ids, cells, max_distance, min_votes=1, keep_below=math.inf):
    """sa_store_search_bestfit without a rule on that call's own tap cells [Q][K][T][K]."""
    return claim(R.restate(q_ids, s_ids, cells, ALL, max_distance, min_votes, keep_below)[0])


def restate_compat(q_ids, s_ids, cells, rule, q_attrs, s_attrs, max_distance, min_votes=1, keep_below=math.inf):
    return claim(X.restate(q_ids, s_ids, cells, rule, q_attrs, s_attrs, ALL, max_distance, min_votes, keep_below)[0])


def search_stored(s_ids, cells, ids, max_distance, min_votes=1, keep_below=math.inf, withdraw=False, rule=None, s_attrs=None):
    """sa_store_search_stored_bestfit: cells [n][K][T][K] of the call; with a rule the queries carry their stored attributes."""
    if rule is None:
        return claim(G.search_stored(s_ids, cells, ids, ALL, max_distance, min_votes, keep_below, withdraw)[0])
    return claim(X.search_stored(s_ids, cells, ids, rule, s_attrs, ALL, max_distance, min_votes, keep_below, withdraw)[0])


def join(s_ids, cells, max_distance, min_votes=1, keep_below=math.inf, rule=None, s_attrs=None):
    """sa_store_join_bestfit: cells [T][K][T][K]; each direction of a pair is a group of its own, with its own weight and claim."""
    return search_stored(s_ids, cells, s_ids, max_distance, min_votes, keep_below, False, rule, s_attrs)


def topn_view(res, topn):
    """What the TopN call returns when the BestFit call returns `res`: {query: [(track, weight), ...]}"""
    return {q: [(t, w) for _, w, t in lst[: int(topn)]] for q, lst in res.items()}
