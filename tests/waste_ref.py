"""The host sequence include/similari_waste.h names as the meaning of sa_tracks_waste and sa_tracks_waste_absorb, through the calls
that were there before it — sa_tracks_get_state per id, the compaction of the present slots in numpy, sa_store_append or
sa_store_absorb_keep, sa_tracks_remove_many — and the engine tables the twin tests run both routes on.  Test infrastructure only.

    fill(engine, scene, ids, present, feats, quality, rng)   a scene's table: sa_tracks_upsert with feat_present, then a full state and
                                                              the qualities through sa_tracks_set_state (an upsert writes no quality)
    read(engine, scene, id)                                   sa_tracks_get_state: (mean10, cov100, quality [K], present [K], feats [K][D])
    compact(state)                                            rows(id) and their qualities: the slots with present == 1, in slot order
    leaving_rows(engine, leaving)                             ids, rows, qualities of {scene: ids} in call order, read BEFORE a call
    remove_many(engine, leaving)                              sa_tracks_remove_many
    snapshot(engine, scenes)                                  sa_tracks_order and sa_tracks_get_state of every track, as bytes
"""
import ctypes as C

import numpy as np

from similari_amd import abi

u8, u32, u64, f32 = np.uint8, np.uint32, np.uint64, np.float32
P = C.POINTER


def patterns(K):
    """The presence patterns of the issue that exist at depth K, by name."""
    out = {"all": np.ones(K, u8), "none": np.zeros(K, u8)}
    if K >= 2:
        out["slot 0 absent"] = np.array([0] + [1] * (K - 1), u8)
        out["only the last"] = np.array([0] * (K - 1) + [1], u8)
    if K >= 3:
        hole = np.ones(K, u8)
        hole[K // 2] = 0
        out["a hole in the middle"] = hole
    return out


def table(rng, n, K, D, first_id=1):
    """n tracks whose presence patterns cycle through patterns(K), then random ones; rows random where present, zero elsewhere (as the
    upsert's pad kernel leaves an absent slot); a quality for every slot, the absent ones included (the newest observation without a
    usable feature keeps its quality)."""
    pats = list(patterns(K).values())
    present = np.stack([pats[i] if i < len(pats) else rng.integers(0, 2, K).astype(u8) for i in range(n)])
    feats = rng.uniform(-1, 1, (n, K, D)).astype(f32) * present[:, :, None]
    quality = rng.uniform(0.05, 1, (n, K)).astype(f32)
    return np.arange(first_id, first_id + n, dtype=u64), present, feats, quality


def fill(engine, scene, ids, present, feats, quality, rng):
    n = len(ids)
    boxes = abi.make_boxes(100.0 + 150.0 * (np.arange(n) % 40), 100.0 + 150.0 * (np.arange(n) // 40), np.full(n, 0.5), np.full(n, 80.0))
    engine.upsert(scene, abi.make_tracks(ids, boxes, np.full(n, 1, u64), feats=feats, feat_present=present))
    fp = P(C.c_float)
    for i, t in enumerate(ids):
        mean, cov = rng.uniform(-1, 1, 10).astype(f32), rng.uniform(-1, 1, 100).astype(f32)
        q = np.ascontiguousarray(quality[i], f32)
        engine._chk(engine.lib.sa_tracks_set_state(engine.h, scene, int(t), mean.ctypes.data_as(fp), cov.ctypes.data_as(fp), q.ctypes.data_as(fp)))


def read(engine, scene, tid, K, D):
    mean, cov, q, pres, feats = np.zeros(10, f32), np.zeros(100, f32), np.zeros(K, f32), np.zeros(K, u8), np.zeros((K, D), f32)
    fp = P(C.c_float)
    engine._chk(engine.lib.sa_tracks_get_state(engine.h, scene, int(tid), mean.ctypes.data_as(fp), cov.ctypes.data_as(fp), q.ctypes.data_as(fp),
                                               pres.ctypes.data_as(P(C.c_uint8)), feats.ctypes.data_as(fp)))
    return mean, cov, q, pres, feats


def compact(state):
    _, _, q, pres, feats = state
    keep = pres != 0
    return feats[keep].copy(), q[keep].copy()


def items(leaving):
    return list(leaving.items()) if isinstance(leaving, dict) else list(leaving)


def leaving_rows(engine, leaving, K, D):
    ids, rows, quality = [], [], []
    for scene, lst in items(leaving):
        for t in lst:
            r, q = compact(read(engine, scene, t, K, D))
            ids.append(int(t)), rows.append(r), quality.append(q)
    return np.array(ids, u64), rows, quality


def remove_many(engine, leaving):
    its = items(leaving)
    lists = [np.ascontiguousarray(x, u64).reshape(-1) for _, x in its]
    scene_ids = np.array([s for s, _ in its], u64)
    counts = np.array([len(x) for x in lists], u32)
    ptrs = (P(C.c_uint64) * max(len(its), 1))(*[x.ctypes.data_as(P(C.c_uint64)) for x in lists])
    engine._chk(engine.lib.sa_tracks_remove_many(engine.h, len(its), scene_ids.ctypes.data_as(P(C.c_uint64)), counts.ctypes.data_as(P(C.c_uint32)), ptrs))


def snapshot(engine, scenes, K, D):
    out = []
    for s in scenes:
        order = engine.order(s)
        out.append((s, order.tobytes(), [tuple(x.tobytes() for x in read(engine, s, t, K, D)) for t in order]))
    return out
