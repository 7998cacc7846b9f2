"""Host restatement of the two gallery calls (include/similari_gallery.h), composed from topn_ref.restate.  Test infrastructure only.

search_stored(): TrackStore::owned_track_distances + TopNVoting::winners (src/track/store.rs:471-486) when withdraw is set, and the
same queries left in the store when it is not.  join(): every stored track searched against every other one."""
from __future__ import annotations

import math

import numpy as np

import topn_ref as R

f32 = np.float32
ALL = 1 << 30


def rows_of(s_ids, full_cells, ids):
    """The cells [n][K][T][K] of a search with the stored tracks `ids`, cut from the store's own matrix [T][K][T][K]; an id the store
    does not hold is a query without observations (a NaN row)."""
    s_ids = [int(i) for i in np.asarray(s_ids, np.uint64).reshape(-1)]
    full = np.asarray(full_cells, f32)
    slot = {i: k for k, i in enumerate(s_ids)}
    out = np.full((len(ids),) + full.shape[1:], np.nan, f32)
    for k, i in enumerate(ids):
        if int(i) in slot:
            out[k] = full[slot[int(i)]]
    return out


def search_stored(s_ids, cells, ids, topn, max_distance, min_votes=1, keep_below=math.inf, withdraw=False):
    """cells: [n][K][T][K] of the call (rows: the queried ids, columns: the store).  withdraw: the queried tracks' columns are out of
    the store before steps 3-4, so a pair of two queried tracks forms no group and does not raise M.  -> ({id: [(winner, weight)]}, M)"""
    s_ids = np.asarray(s_ids, np.uint64).reshape(-1)
    ids = np.asarray(ids, np.uint64).reshape(-1)
    cells = np.array(cells, f32, copy=True)
    if withdraw:
        cells[:, :, np.isin(s_ids, ids), :] = np.nan
    return R.restate(ids, s_ids, cells, topn, max_distance, min_votes, keep_below)


def join(s_ids, cells, topn, max_distance, min_votes=1, keep_below=math.inf):
    """cells: [T][K][T][K], rows and columns in store order."""
    return search_stored(s_ids, cells, s_ids, topn, max_distance, min_votes, keep_below)


def surviving_pairs(s_ids, cells, max_distance, min_votes=1, keep_below=math.inf):
    """The unordered pairs of stored ids that form a group in a join (each direction forms it or neither does)."""
    res, _ = join(s_ids, cells, ALL, max_distance, min_votes, keep_below)
    return {frozenset((q, w)) for q, lst in res.items() for w, _ in lst}
