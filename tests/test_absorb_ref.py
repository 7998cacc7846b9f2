"""tests/absorb_ref.py, the model the GPU tests of sa_store_absorb lean on, held to what the reference's incremental loop does
(examples/incremental_track_build.rs) and to the two corners of step 2 of include/similari_absorb.h."""
import numpy as np

import absorb_ref as A
import bestfit_ref as B

f32 = np.float32


def test_two_drifting_identities_build_two_tracks_of_five():
    """incremental_track_build.rs, seeded: FeatGen2 walks from (0, 0) and (1, 1) with drift 0.01, every frame brings one new track
    per identity under a fresh id, MAX_DIST 0.1 cuts below (`< MAX_DIST`) and votes, the metric keeps the last five observations.
    Ten frames leave two tracks — the ids of the first frame — of five observations each: the identities' last five, in order."""
    rng = np.random.default_rng(7)
    m = A.Model(5, 2, "euclidean")
    pos = [np.array([0.0, 0.0], f32), np.array([1.0, 1.0], f32)]
    seen = [[], []]
    next_id = 100
    for frame in range(10):
        ids, feats, qual = [], [], []
        for k in range(2):
            pos[k] = (pos[k] + rng.uniform(-0.01, 0.01, 2).astype(f32)).astype(f32)
            seen[k].append(pos[k].copy())
            ids.append(next_id)
            next_id += 1
            feats.append(pos[k].reshape(1, 2))
            qual.append([f32(0.7 + rng.uniform(-0.01, 0.01))])
        res, dest = m.absorb(ids, feats, 1, 0.1, keep_below=0.1, quality=qual, capacity=5)
        if frame == 0:
            assert res == {} and dest == {100: 100, 101: 101}
        else:
            assert dest == {ids[0]: 100, ids[1]: 101}
            assert [res[q][0][0] for q in ids] == [100, 101]
    assert m.order == [100, 101]
    for k, t in enumerate(m.order):
        assert len(m.banks[t]) == 5
        assert np.array_equal(m.feats(t), np.stack(seen[k][-5:]))


def test_two_queries_on_one_stored_track_the_loser_is_created():
    m = A.Model(2, 2, "euclidean")
    m.upsert([1, 2], [np.array([[0.0, 0.0]], f32), np.array([[10.0, 10.0]], f32)])
    q = [np.array([[0.0, 0.5]], f32), np.array([[0.0, 0.25]], f32)]   # both name track 1 and nothing else below the cut; 7 is nearer
    res, dest = m.absorb([8, 7], q, 2, 1.0)
    assert dest == {7: 1, 8: 8}                                        # the loser keeps its own id and becomes a track
    assert res[7][0][0] == 1 and res[8][0][0] == 8 and res[8][0][2] == 1
    assert m.order == [1, 2, 8]
    assert np.array_equal(m.feats(1), np.array([[0.0, 0.0], [0.0, 0.25]], f32))
    assert np.array_equal(m.feats(8), np.array([[0.0, 0.5]], f32))


def test_entry_zero_lost_while_entry_one_holds_a_claim_still_creates():
    """Query 8's best track is 1, which query 7 claims with a better weight; 8's second entry names track 2 and holds that claim.
    Only entry 0 acts: 8 is created, track 2 stays as it is."""
    m = A.Model(2, 2, "euclidean")
    m.upsert([1, 2], [np.array([[0.0, 0.0]], f32), np.array([[1.0, 0.0]], f32)])
    q7, q8 = np.array([[0.0, 0.125]], f32), np.array([[0.25, 0.0]], f32)
    cells = A.cells_of(m, [q7, q8], "euclidean")
    full, _, _ = B.restate([7, 8], m.order, cells, 2.0)
    assert [e[0] for e in full[8]] == [8, 2] and [e[2] for e in full[8]] == [1, 2]   # lost entry 0, holds entry 1
    res, dest = m.absorb([7, 8], [q7, q8], 2, 2.0)
    assert A.decide([7, 8], full) == dest == {7: 1, 8: 8}
    assert m.order == [1, 2, 8] and len(m.banks[2]) == 1 and len(m.banks[1]) == 2


def test_a_matched_query_without_rows_and_capacity_per_query():
    m = A.Model(3, 2, "euclidean")
    m.upsert([1], [np.array([[0.0, 0.0], [0.0, 0.5], [0.0, 1.0]], f32)])
    res, dest = m.absorb([5], [np.array([[0.0, 1.25]], f32)], 1, 1.0, capacity={5: 2})
    assert dest == {5: 1}
    assert np.array_equal(m.feats(1), np.array([[0.0, 1.0], [0.0, 1.25]], f32))   # 2 < n0: the bank shrinks
    res, dest = m.absorb([6], [np.zeros((0, 2), f32)], 1, 1.0)
    assert res == {} and dest == {6: 6} and m.order == [1, 6] and len(m.banks[6]) == 0
