"""tests/absorb_ref.py, the model the GPU tests of sa_store_absorb lean on, held to what the reference's incremental loop does
(examples/incremental_track_build.rs) and to the two corners of step 2 of include/similari_absorb.h; and tests/absorb_cases.py, the
frames of tests/test_gpu_absorb.py, held to the premise their expected destinations rest on."""
import numpy as np
import pytest

import absorb_cases as AC
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


# ---- tests/absorb_cases.py ------------------------------------------------------------------------------------------------------
def test_expected_dest_is_the_named_track_once_and_only_with_a_row():
    rng = np.random.default_rng(1)
    banks = {4: rng.uniform(-1, 1, (2, 33)).astype(f32), 9: rng.uniform(-1, 1, (1, 33)).astype(f32), 6: np.zeros((0, 33), f32)}
    on, n_obs, q_ids = [4, None, 9, 4, 9, 6, None], [2, 1, 0, 1, 1, 1, 0], np.arange(100, 107)
    feats, dest = AC.frame(rng, banks, on, n_obs, "euclidean", q_ids=q_ids)
    assert [int(d) for d in dest] == [4, 101, 102, 103, 9, 105, 106]   # 102 brings no row, 103 names track 4 again, track 6 holds no row
    assert [f.shape for f in feats] == [(m, 33) for m in n_obs]
    assert np.abs(feats[0] - banks[4][0]).max() < 0.01 and np.abs(feats[4] - banks[9][0]).max() < 0.01
    neg, _ = AC.frame(rng, banks, [4], [1], "cosine")
    assert np.abs(neg[0] + banks[4][0]).max() < 0.01


def below_and_above(case):
    """The premise of expected_dest for one case: in the store's measure, on the rows as the store rounds them."""
    built, other = AC.premise(case)
    cut = AC.CUT[case["kind"]]
    print("%s D = %d Q = %d: built rows within %.4g of their row, every other pairing beyond %.4g (cut %g)"
          % (case["kind"], case["D"], len(case["q_ids"]), built, other, cut))
    assert built <= cut < other
    # nearer than half the cut, farther than twice it (a similarity: the same margins towards -1 and 0): no rounding decides a vote
    if case["kind"] == "euclidean":
        assert built <= cut / 2 and other >= 2 * cut
    else:
        assert built <= -0.95 and other >= -0.8


@pytest.mark.parametrize("Q,last", AC.WAVE_QS)
def test_a_long_frames_queries_lie_where_expected_dest_needs_them(Q, last):
    """The exact generator and seeds of test_a_frame_past_one_wave_and_one_scan_chunk.  Measured at Q = 2100: built rows within 0.008
    of their row, every other pairing beyond 2 (D = 33, uniform(-1, 1) rows, noise 1e-3)."""
    case = AC.wave_case(Q, last)
    below_and_above(case)
    q_ids, dest = case["q_ids"], case["expected_dest"]
    matched = dest != q_ids
    assert len(set(dest.tolist())) == Q                      # no stored track is named twice
    assert 0 < matched.sum() < Q and (np.array(case["n_obs"]) == 0).any() == (Q >= 64)
    if last is not None:
        assert bool(matched[-1]) == last
    if Q == 2100:   # what the GPU test asserts again on the engine's own dest: every scan chunk, every slot range
        for lo, hi in AC.SCAN_CHUNKS:
            assert matched[lo:hi].any() and not matched[lo:hi].all()
        slots = dest[matched].astype(np.int64) - 1
        for lo, hi in AC.SLOT_RANGES:
            assert ((slots >= lo) & (slots < hi)).any()
        assert set(case["capacity"].tolist()) == {1, 2}


@pytest.mark.parametrize("elem,kind,D", AC.WIDE_FORMS)
def test_a_wide_frames_queries_lie_where_expected_dest_needs_them(elem, kind, D):
    case = AC.wide_case(elem, kind, D)
    below_and_above(case)
    assert [int(d) for d in case["expected_dest"]] == [1, 2, 3, 503, 504, 505, 506, 4, 5, 7]
    before, after = case["model"], case["after"]
    assert [len(before.banks[t]) for t in (1, 2, 3, 4, 5, 7, 8)] == [5, 5, 2, 4, 1, 5, 3]
    assert [len(after.banks[t]) for t in (1, 2, 3, 4, 5, 7, 8, 503, 504, 505, 506)] == [5, 2, 3, 5, 1, 3, 3, 0, 0, 1, 5]
    assert after.order == list(range(1, 13)) + [503, 504, 505, 506]
    assert np.array_equal(after.feats(1)[:3], before.feats(1)[2:])   # drop = 2: the bank's rows 2, 3, 4 lead
    assert np.array_equal(after.feats(7)[:2], before.feats(7)[3:])   # drop = 3
    n_obs, feats, qual = AC.held(after, after.order)
    assert list(n_obs[:3]) == [5, 2, 3] and not feats[1, 2:].any() and np.array_equal(qual[0, 3:], np.asarray(case["quality"][0], f32))
