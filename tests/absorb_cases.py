"""The data of tests/test_gpu_absorb.py and what makes it decidable on the host: seeded banks, frames whose queries are either built on
a stored row or far from every stored row, and the destination every query must therefore take.  tests/test_absorb_ref.py asserts
the premise — every built row below the cut, every other pairing above it — for the exact cases the GPU tests run, so that
`expected_dest` is a statement about the data and not about the engine.  numpy only; test infrastructure only.

    banks(rng, T, K, D)                 ids 1..T and their ragged banks (what test_gpu_absorb.twin upserts)
    frame(rng, banks, on, n_obs, kind)  the query rows of one frame and, with q_ids, expected_dest
    wave_case(Q, last)                  D = 33, K = 2, T = 700: a frame past one wave and past one scan chunk of k_absorb_rank
    wide_case(elem, kind, D)            K = 5, T = 12, Q = 10: every shape of bank shift at rows wider than one pass of a wave
    held(model, ids)                    what fetch_raw must return for a merge_ref.Model
    premise(case)                       the extremes test_absorb_ref.py holds against CUT
"""
import numpy as np

import bf16_ref
import f16_ref
import merge_ref

u32, u64, f32 = np.uint32, np.uint64, np.float32
ELEM_F32, ELEM_BF16, ELEM_F16 = 0, 1, 2   # SA_ELEM_*
# A query built on a stored row lies below the cut, random rows lie far above it.  "cosine" is the similarity, as the reference names
# it, and the vote keeps d <= max_distance: the best match of a row is its negation (-1), and random rows stay above -0.9.
CUT = {"cosine": -0.9, "euclidean": 0.25}
# k_absorb_rank walks the queries in chunks of 1024; k_absorb_match finds a slot by lane u of 4 x 64 per turn of 256
SCAN_CHUNKS = [(0, 1024), (1024, 2048), (2048, 2100)]
SLOT_RANGES = [(0, 64), (64, 256), (256, 512), (512, 700)]
WAVE_QS = [(64, None), (65, False), (65, True), (1024, None), (1025, False), (1025, True), (2100, None)]   # (Q, the last query is matched)
WIDE_FORMS = [(ELEM_F32, "euclidean", 260), (ELEM_F32, "cosine", 1024), (ELEM_F16, "euclidean", 1024), (ELEM_BF16, "cosine", 520)]


def banks(rng, T, K, D):
    """ids 1..T; every count 1..K among the first tracks, no stored track is empty, so each can be a winner"""
    ids = np.arange(1, T + 1, dtype=u64)
    n_obs = rng.integers(1, K + 1, T)
    n_obs[: min(T, K)] = np.arange(1, min(T, K) + 1)
    return ids, [rng.uniform(-1, 1, (int(m), D)).astype(f32) for m in n_obs]


def frame(rng, banks, on, n_obs, kind, noise=1e-3, q_ids=None, D=None):
    """One query per entry of `on`: a stored id — its rows are that track's first row (a cosine store: its negation) plus a little
    noise, so the track is its winner — or None: random rows, far from everything.  banks: {id: rows [n][D]}, the host's copy of
    what the store holds (of a 16-bit store: the rounded rows).  -> (feats, expected_dest); expected_dest[i] is the named stored id
    where on[i] is a stored id with a row, n_obs[i] > 0 and no earlier query names it, else q_ids[i] (None without q_ids).
    Which of two queries on one stored track holds the claim is the vote's to say, not this rule's: the cases below name a stored
    track once."""
    if D is None:
        D = next(iter(banks.values())).shape[1]
    sign = f32(-1) if kind == "cosine" else f32(1)
    feats, dest, named = [], [], set()
    for i, (t, m) in enumerate(zip(on, n_obs)):
        bank = None if t is None or m == 0 else banks[int(t)]
        if bank is None or len(bank) == 0:   # (a stored track without a row cannot be a winner either)
            feats.append(rng.uniform(-1, 1, (int(m), D)).astype(f32))
            dest.append(None)
        else:
            feats.append((sign * bank[0][None, :] + rng.normal(0, noise, (int(m), D))).astype(f32))
            dest.append(None if int(t) in named else int(t))
            named.add(int(t))
    if q_ids is None:
        return feats, None
    return feats, np.array([int(q) if d is None else d for q, d in zip(q_ids, dest)], u64)


def finish(rng, case, on, n_obs, q_ids, capacity):
    host = {int(i): case["model"].feats(i) for i in case["ids"]}   # as the store holds them: rounded, in a 16-bit store
    feats, dest = frame(rng, host, on, n_obs, case["kind"], q_ids=q_ids)
    quality = [rng.uniform(0, 1, int(m)).astype(f32) for m in n_obs]
    after = type(case["model"])(case["K"], case["D"])   # (merge_ref.Model.copy would drop a 16-bit model's rounding)
    after.order, after.banks = list(case["model"].order), {i: list(b) for i, b in case["model"].banks.items()}
    after.append(dest, feats, quality, merge_ref.LATEST, capacity)
    case.update(rng=rng, on=on, n_obs=[int(m) for m in n_obs], q_ids=q_ids, feats=feats, quality=quality,
                capacity=np.asarray(capacity, u32), expected_dest=dest, after=after)
    return case


def start(rng, elem, kind, D, K, ids, bk):
    ref = {ELEM_F32: merge_ref, ELEM_F16: f16_ref, ELEM_BF16: bf16_ref}[elem]
    model = ref.Model(K, D)
    model.upsert(ids, bk)
    return dict(elem=elem, kind=kind, D=D, K=K, ids=ids, banks=bk, model=model)


def wave_case(Q, last=None):
    """An f32 euclidean store of 700 ragged banks of up to two rows at D = 33 and one frame of Q queries.  About three queries in
    ten are built on a stored track, dealt from a permutation of the slots, so matched and created queries alternate irregularly
    inside every wave of the scan and the matched slots lie all over [0, 700); some stored tracks are left when the last scan chunk
    begins.  A query in twenty-five brings no row (it is created, whatever it names).  last: the last query is matched (True) or
    created (False) — a frame of 65 or 1025 ends with one query alone in its wave and its chunk."""
    D, K, T = 33, 2, 700
    rng = np.random.default_rng(7000 + 2 * Q + (last is True))
    ids, bk = banks(rng, T, K, D)
    case = start(rng, ELEM_F32, "euclidean", D, K, ids, bk)
    perm = rng.permutation(T)
    named = rng.random(Q) < 0.3
    n_obs = rng.integers(1, K + 1, Q)
    n_obs[rng.random(Q) < 0.04] = 0
    if last is not None:
        named[-1], n_obs[-1] = last, max(int(n_obs[-1]), 1)
    on, used = [], 0
    for i in range(Q):
        on.append(int(ids[perm[used]]) if named[i] and used < T else None)
        used += on[-1] is not None
    q_ids = np.arange(10000, 10000 + Q, dtype=u64)
    return finish(rng, case, on, n_obs, q_ids, rng.integers(1, K + 1, Q).astype(u32))


def wide_case(elem, kind, D):
    """K = 5 (Kp = 8), twelve stored banks of 5 5 2 4 1 4 5 3 rows and four more, ten queries:
        0  on a full bank, 2 rows at capacity 5: drop = 2, the bank shifts onto itself;
        1  on a full bank, K rows at capacity 2: drop >= n0, nothing of the bank stays and its tail is zeroed;
        2  on a bank of 2, 1 row at capacity 5: drop = 0, the rows stay;
        3  names a stored track and brings no row: no vote, so it becomes a track without rows and the named bank stays;
        4  far from everything, no row; 5 one row; 6 K rows: created tracks;
        7  on a bank of 4, 3 rows at capacity 5: the shifted bank is two of its own rows and three of the query's;
        8  on a bank of 1, 2 rows at capacity 1: the bank's only row leaves;
        9  on a full bank, 1 row at capacity 3: two rows move down, one arrives, two are zeroed."""
    K, T = 5, 12
    rng = np.random.default_rng(8000 + 10 * D + elem)
    ids = np.arange(1, T + 1, dtype=u64)
    bk = [rng.uniform(-1, 1, (m, D)).astype(f32) for m in (5, 5, 2, 4, 1, 4, 5, 3, 2, 5, 1, 3)]
    case = start(rng, elem, kind, D, K, ids, bk)
    on = [1, 2, 3, 8, None, None, None, 4, 5, 7]
    n_obs = [2, K, 1, 0, 0, 1, K, 3, 2, 1]
    q_ids = np.arange(500, 510, dtype=u64)
    return finish(rng, case, on, n_obs, q_ids, [5, 2, 5, 5, 1, 5, 5, 5, 1, 3])


def held(model, ids):
    """(n_obs [n], feats [n][K][D], quality [n][K]) as fetch_raw returns them for a store that holds what the model holds"""
    n = len(ids)
    n_obs, feats, qual = np.zeros(n, u32), np.zeros((n, model.K, model.D), f32), np.zeros((n, model.K), f32)
    for k, i in enumerate(ids):
        m = len(model.banks[int(i)])
        n_obs[k] = m
        if m:
            feats[k, :m], qual[k, :m] = model.feats(i), model.quality(i)
    return n_obs, feats, qual


def probes(case, tracks):
    """One query of one row per track: a row the track holds after the frame (a cosine store: its negation), under a fresh id."""
    sign = f32(-1) if case["kind"] == "cosine" else f32(1)
    return np.arange(900001, 900001 + len(tracks), dtype=u64), [sign * case["after"].feats(t)[:1] for t in tracks]


def distances(kind, a, b):
    """[len(a)][len(b)] in f64: the euclidean distance, or the cosine similarity"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    dot, na, nb = a @ b.T, (a * a).sum(1), (b * b).sum(1)
    if kind == "cosine":
        return dot / np.sqrt(na[:, None] * nb[None, :])
    return np.sqrt(np.maximum(na[:, None] + nb[None, :] - 2.0 * dot, 0.0))


def premise(case):
    """-> (the farthest a built row lies from the row it was built on, the nearest any query row comes to a stored row it was not
    built on), both in the store's measure and on the rows as the store rounds them.  Rows of the named track other than the first
    are left out of the second: they vote for the same track."""
    rnd = {ELEM_F32: lambda x: np.asarray(x, f32), ELEM_F16: f16_ref.round_f16, ELEM_BF16: bf16_ref.round_bf16}[case["elem"]]
    model, kind = case["model"], case["kind"]
    owner = np.concatenate([np.full(len(model.banks[int(i)]), int(i)) for i in case["ids"]])
    first = np.concatenate([np.arange(len(model.banks[int(i)])) == 0 for i in case["ids"]])
    stored = np.concatenate([model.feats(i) for i in case["ids"]])
    built, other = [], []
    for q, t, f in zip(case["q_ids"], case["expected_dest"], case["feats"]):
        if not len(f):
            continue
        d = distances(kind, rnd(f), stored)
        mine = (owner == int(t)) if t != q else np.zeros(len(owner), bool)
        if mine.any():
            built.append(d[:, mine & first].max())
        if (~mine).any():
            other.append(d[:, ~mine].min())
    return max(built), min(other)
