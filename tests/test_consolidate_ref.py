"""The host model of a consolidation (tests/consolidate_ref.py) against what include/similari_consolidate.h says of steps 2 and 3:
pairs are disjoint, the lower id is the destination, a third track that names a paired one stays, and the sources leave as
tests/merge_ref.py's merge removes them."""
import numpy as np

import consolidate_ref as CR
import merge_ref as MR

u32, u64, f32 = np.uint32, np.uint64, np.float32


def join_outputs(ids, names, topn=2):
    """out_n / out_winner of a join in which track a's entry 0 is names[a] (absent: no entry)."""
    out_n = np.array([1 if int(a) in names else 0 for a in ids], u32)
    win = np.zeros((len(ids), topn), u64)
    for i, a in enumerate(ids):
        win[i, 0] = names.get(int(a), 0)
    return out_n, win


def test_pairs_are_disjoint_and_the_lower_id_is_the_destination():
    rng = np.random.default_rng(3)
    for _ in range(50):
        ids = rng.permutation(np.arange(1, 31, dtype=u64))
        names = {int(a): int(rng.choice(ids)) for a in ids if rng.random() < 0.8}   # own id among them: no partner
        out_n, win = join_outputs(ids, names)
        found, dest = CR.pairs(ids, out_n, win)
        flat = [x for p in found for x in p]
        assert len(flat) == len(set(flat))
        at = {int(a): i for i, a in enumerate(ids)}
        for d, s in found:
            assert d < s and names[d] == s and names[s] == d
            assert dest[at[s]] == d and dest[at[d]] == d
        assert [at[d] for d, _ in found] == sorted(at[d] for d, _ in found)   # destinations in the order of ids
        sources = {s for _, s in found}
        assert all(dest[i] == a for i, a in enumerate(ids) if int(a) not in sources)
        # every mutual pair is found
        want = {(a, b) for a, b in names.items() if a < b and names.get(b) == a}
        assert set(found) == want


def test_an_entry_beyond_out_n_does_not_act():
    ids = np.array([5, 9], u64)
    win = np.array([[9, 0], [5, 0]], u64)
    assert CR.pairs(ids, np.array([1, 0], u32), win)[0] == []
    assert CR.pairs(ids, np.array([1, 1], u32), win)[0] == [(5, 9)]


def test_a_third_track_naming_a_paired_one_stays():
    ids = np.array([7, 3, 11], u64)   # A = 7, B = 3, C = 11 names B
    out_n, win = join_outputs(ids, {7: 3, 3: 7, 11: 3})
    found, dest = CR.pairs(ids, out_n, win)
    assert found == [(3, 7)] and dest.tolist() == [3, 3, 11]


def test_the_merge_and_the_removal_are_merge_refs():
    rng = np.random.default_rng(5)
    K, D = 3, 4
    ids = np.array([4, 9, 2, 7, 5, 1], u64)
    m = MR.Model(K, D)
    banks = [rng.uniform(0, 1, (int(n), D)).astype(f32) for n in (1, 3, 2, 3, 1, 2)]
    m.append(ids, banks, [rng.uniform(0, 1, len(b)).astype(f32) for b in banks], MR.BEST)
    attrs = {int(a): (int(a) % 2, 10 * i, 10 * i + 5) for i, a in enumerate(ids)}
    out_n, win = join_outputs(ids, {4: 9, 9: 4, 2: 1, 1: 2, 7: 9})
    for keep in (MR.LATEST, MR.BEST):
        for cap in (None, 2):
            found, dest, after, new_attrs = CR.consolidate(m, attrs, ids, out_n, win, keep, cap, ruled=True)
            assert found == [(4, 9), (1, 2)]
            want = m.copy()
            want.merge({4: [9], 1: [2]}, keep, cap)
            assert after.order == want.order == [4, 1, 5, 7]   # 9 leaves: 1 moves in; 2 leaves: 5 moves in
            for i in after.order:
                assert np.array_equal(after.feats(i), want.feats(i)) and np.array_equal(after.quality(i), want.quality(i))
            assert len(after.banks[4]) == min(K + 1, cap or K) and len(after.banks[1]) == min(2 + 2, cap or K)   # the rule ran on both
            assert new_attrs[4] == (0, 0, 15) and new_attrs[1] == (1, 20, 55) and sorted(new_attrs) == [1, 4, 5, 7]
    # without a rule no attribute is touched, and without a pair nothing changes
    assert CR.consolidate(m, attrs, ids, out_n, win, MR.LATEST)[3][4] == attrs[4]
    none = CR.consolidate(m, attrs, ids, *join_outputs(ids, {4: 9, 9: 2}), MR.LATEST)
    assert none[0] == [] and none[2].order == m.order and none[3] == attrs and none[1].tolist() == ids.tolist()
