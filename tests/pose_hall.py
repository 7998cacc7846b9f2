"""The packed halls of tests/pose_ref.hall as scenes the keypoint tests can share.  TEST INFRASTRUCTURE: tests/test_pose_hall_ref.py shows
on the CPU, from the model alone, that every (hall, threshold, min_common) listed here is what tests/test_gpu_pose_hall.py takes it
for; the GPU file runs the same list.  A Hall has the attributes of tests/test_gpu_pose.Scene that check_vote and
tests/test_gpu_pose_batch.fill read; its model, its vote and the host emulation's answer are computed once per process.

No filter produced these tracks: fill()'s one step (every point present) creates them, settle() then writes every state."""
import functools

import numpy as np

import points_ref as R
import pose_emu as PE
import pose_ref as PR

f32, u64 = np.float32, np.uint64
NT = 256   # a thread of the dense search owns the columns t, t + NT, ...: strip c holds the columns [c * NT, (c + 1) * NT)


class Hall:
    def __init__(self, M, T, P, corner=None, seed=1):
        self.m, self.T, self.P, self.corner, self.seed = M, T, P, corner, seed
        self.ids = np.arange(T, dtype=u64) * 3 + 5
        self.poses, self.pres, has, mean, cov = PR.hall(seed, M, T, P, corner=corner)
        self.model = R.Bank((T, P))
        self.model.has = has
        self.model.mean[has], self.model.cov[has] = mean[has], cov[has]
        self.rounds = [(mean[..., :2].copy(), np.ones((T, P), bool))]
        self.seeded = (0, int(np.argmax(has[0])))   # (what fill() writes itself; settle() writes them all)
        for a in (self.poses, self.pres, has):
            a.setflags(write=False)

    def __repr__(self):
        return "hall%dx%dx%d" % (self.m, self.T, self.P) + ("c%g" % self.corner if self.corner else "") + ("s%d" % self.seed if self.seed != 1 else "")

    @functools.lru_cache(maxsize=None)
    def weights(self, min_common=1):
        w = PR.weights(self.poses, self.pres, self.model.has, self.model.mean, self.model.cov, R.PW, min_common)
        w.setflags(write=False)
        return w

    @functools.lru_cache(maxsize=None)
    def vote(self, min_common=1, threshold=1.0):
        return PR.vote(self.weights(min_common), threshold)

    @functools.lru_cache(maxsize=None)
    def emu(self, min_common=1, threshold=1.0):
        """the host build of the device's route -> (rmatch [M], total gain, roots)"""
        return PE.assign(self.weights(min_common), threshold)

    @functools.lru_cache(maxsize=None)
    def facts(self, min_common=1, threshold=1.0):
        """What the model alone says of the search this scene asks for."""
        total, ref, wq, thr_q = self.vote(min_common, threshold)
        w = self.weights(min_common)
        M = self.m
        gain = wq[:, M:] - thr_q
        bid = np.where(gain.max(1) > 0, np.argmax(gain, 1), -1)   # the first of the maxima
        won = np.zeros(M, bool)
        taken = set()
        for i in np.flatnonzero(bid >= 0):
            if int(bid[i]) not in taken:
                taken.add(int(bid[i]))
                won[i] = True
        cols = ref[ref >= 0]
        finite = ~np.isnan(w)
        l_cov = self.model.cov[..., 0, 1]
        coupled = (self.model.has & (l_cov != 0)).any(1)   # tracks with a point whose x and y are correlated
        return dict(
            roots=PR.greedy_roots(wq, thr_q),
            moved=int(((ref >= 0) & (bid >= 0) & (ref != bid)).sum()),     # matched, but not to the column the row bid for
            dropped=int(((bid >= 0) & (ref < 0)).sum()),                     # has a usable pair, unmatched in the optimum
            winners_dropped=int((won & (ref < 0)).sum()),                    # ... although the greedy start had matched it
            matched=int((ref >= 0).sum()),
            top=int(cols.max()) if len(cols) else -1,
            strips=np.bincount(cols // NT, minlength=8)[:8].tolist(),
            usable=float((gain > 0).sum()) / max(gain.size, 1),
            coupled_weights=int(finite[:, coupled].sum()),
        )

    def settle(self, bank, ids):
        """every track's state as the model has it"""
        b = self.model
        for j, t in enumerate(ids):
            h = b.has[j]
            bank.set_state(t, h, np.where(h[:, None], b.mean[j], 0), np.where(h[:, None, None], b.cov[j], 0))


@functools.lru_cache(maxsize=None)
def hall(M, T, P, corner=None, seed=1):
    return Hall(M, T, P, corner, seed)


# (M, T, P, corner) and the thresholds of the single call
VOTE = [
    ((300, 300, 2, None), (1.0, 99.0, 99.5)),
    ((320, 257, 3, 50.0), (1.0, 99.5)),      # one column in strip 1; more poses than tracks, in a corner: rows are dropped
    ((300, 40, 2, None), (1.0, 99.5)),       # few columns: nearly every row is a root
    ((96, 96, 65, None), (1.0, 99.5)),       # the 64-point chunk crossed
    ((256, 2048, 2, 20.0), (1.0, 99.5)),     # strips 0 .. 7
    ((512, 2048, 2, 30.0), (1.0, 99.5)),
]
MATRIX = [(17, 70, 17, None), (96, 96, 129, None)]   # the second crosses three 64-point chunks
# the batch and the frame loop: threshold 99.5, min_common 2
BATCH = [(300, 300, 2, None), (320, 257, 2, 50.0, 2), (300, 40, 2, None)]   # (seed 2: the first whose optimum takes column 256)
TRACK = [(300, 300, 3, None), (200, 257, 3, 50.0), (150, 40, 3, None)]
THRESHOLD, MIN_COMMON = 99.5, 2
BIG = 256   # from this many poses and tracks on, the floors the halls were made for hold


def uses():
    """every (hall, min_common, threshold) of tests/test_gpu_pose_hall.py's votes"""
    out = [(hall(*k), 1, thr) for k, thrs in VOTE for thr in thrs]
    return out + [(hall(*k), MIN_COMMON, THRESHOLD) for k in BATCH + TRACK]
