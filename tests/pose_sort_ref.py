"""The keypoint tracker of include/similari_pose_sort.h as a numpy f32 model.  TEST INFRASTRUCTURE: what similari_amd/csrc/sa_pose_gate.h,
sa_pose_sort_plan.h, the gated kernels of sa_pose.hip and KeypointSort are compared with.

Two parts.  The gate: the circle around a set of points, dist_in_2r, the limit of a track and the mask of refused pairs, applied to
tests/pose_ref.py's weight matrix.  The life cycle: RefSort keeps what the header says the tracker keeps — per scene an epoch and the
list of its tracks, per track its record, the id counter, the bank's order under sa_points_remove's rule — and steps the states with
tests/points_ref.py.  Its vote is pose_ref's kuhn_munkres on the gated matrix, or columns handed in (the plan test feeds the same
columns to the header and to the model)."""
import numpy as np

import points_ref as R

f32 = np.float32
EPS = f32(0.00001)
INF = f32(np.inf)


# ---- the gate ----------------------------------------------------------------------------------------------------------------------
def circle(xy, counts):
    """xy [..., P, 2] f32, counts [..., P] bool -> (c [..., 3] f32: xc, yc, r; valid [...] bool).  The walk of sa_pose_rect_add: the first
    point that counts seeds the rectangle, every later one is compared with < and >."""
    xy, counts = np.asarray(xy, f32), np.asarray(counts, bool)
    lead = counts.shape[:-1]
    lo, hi = np.zeros(lead + (2,), f32), np.zeros(lead + (2,), f32)
    n = np.zeros(lead, np.int64)
    with np.errstate(invalid="ignore"):
        for p in range(counts.shape[-1]):
            z, c = xy[..., p, :], counts[..., p]
            first = (c & (n == 0))[..., None]
            later = (c & (n > 0))[..., None]
            lo = np.where(first, z, np.where(later & (z < lo), z, lo)).astype(f32)
            hi = np.where(first, z, np.where(later & (z > hi), z, hi)).astype(f32)
            n += c
        centre = (f32(0.5) * (lo + hi)).astype(f32)
        half = (f32(0.5) * (hi - lo)).astype(f32)
        r = np.sqrt((half[..., 0] * half[..., 0] + half[..., 1] * half[..., 1]).astype(f32)).astype(f32)
    out = np.concatenate([centre, r[..., None]], -1).astype(f32)
    valid = n > 0
    return np.where(valid[..., None], out, f32(0)).astype(f32), valid


def dist_in_2r(a, b):
    """sa_dist_in_2r on circles [..., 3]: every operation an f32 one, none fused"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    with np.errstate(all="ignore"):
        radial = (a[..., 2] + b[..., 2]).astype(f32)
        x, y = (a[..., 0] - b[..., 0]).astype(f32), (a[..., 1] - b[..., 1]).astype(f32)
        num = np.sqrt(((x * x).astype(f32) + (y * y).astype(f32)).astype(f32)).astype(f32)
        den = np.sqrt(((radial * radial).astype(f32) + EPS).astype(f32)).astype(f32)
        return (num / den).astype(f32)


def constraints(cons):
    """add_constraints: a stable sort by delta, of equal deltas the first stays"""
    out = []
    for d, x in sorted(((int(d), f32(x)) for d, x in cons), key=lambda c: c[0]):
        if not out or out[-1][0] != d:
            out.append((d, x))
    return out


def limit(cons, delta):
    """validate()'s choice for an epoch delta: the max_dist of the first constraint whose delta is >= it, +inf: none.  cons: sorted."""
    for d, x in cons:
        if d >= delta:
            return f32(x)
    return INF


def refused(pose_c, pose_ok, track_c, track_ok, limits):
    """-> [M, T] bool: the pairs the rule refuses"""
    limits = np.asarray(limits, f32)
    d = dist_in_2r(np.asarray(pose_c, f32)[:, None, :], np.asarray(track_c, f32)[None, :, :])
    with np.errstate(invalid="ignore"):
        return np.isfinite(limits)[None, :] & np.asarray(pose_ok, bool)[:, None] & np.asarray(track_ok, bool)[None, :] & ~(d <= limits[None, :])


def gate(w, poses, present, has, mean, limits):
    """pose_ref.weights' matrix under the gate: a refused pair has no weight -> (w gated, refused [M, T])"""
    pc, pok = circle(np.where(np.asarray(present, bool)[..., None], poses, f32(0)), present)
    tc, tok = circle(np.asarray(mean, f32)[..., :2], has)
    no = refused(pc, pok, tc, tok, limits)
    return np.where(no, f32(np.nan), np.asarray(w, f32)).astype(f32), no


# ---- the life cycle ----------------------------------------------------------------------------------------------------------------
class RefSort:
    def __init__(self, P, max_idle_epochs=5, cons=(), min_common=1, threshold=1.0, coast=True, pw=R.PW, vw=R.VW):
        self.P, self.max_idle, self.cons = P, int(max_idle_epochs), constraints(cons)
        self.min_common, self.threshold, self.coast, self.pw, self.vw = min_common, threshold, coast, f32(pw), f32(vw)
        self.epochs, self.lists, self.rec = {}, {}, {}     # scene -> epoch; scene -> [track ids]; id -> dict(scene, first, last, length)
        self.order, self.state = [], {}                    # the bank's order; id -> [has [P], mean [P, 4], cov [P, 4, 4]]
        self.next_id, self.wasted = 1, []

    # -- what the next frame over these scenes would do; nothing changes --
    def plan(self, scene_ids):
        assert len(set(scene_ids)) == len(scene_ids), "a scene named twice"
        epoch = [self.epochs.get(s, 0) + 1 for s in scene_ids]
        expired, tracks, limits = [], [], []
        for s, e in zip(scene_ids, epoch):
            mine = self.lists.get(s, [])
            gone = [t for t in mine if e - self.rec[t]["last"] > self.max_idle]
            expired += gone
            tracks.append([t for t in mine if t not in gone])
            limits.append(np.array([limit(self.cons, e - self.rec[t]["last"]) for t in tracks[-1]], f32))
        return dict(epoch=epoch, expired=expired, tracks=tracks, limits=limits)

    def remove_from_order(self, ids):
        """sa_points_remove: the last track moves into each hole in turn, in call order"""
        for t in ids:
            at = self.order.index(t)
            self.order[at] = self.order[-1]
            self.order.pop()

    def states_of(self, ids):
        if not len(ids):
            return np.zeros((0, self.P), bool), np.zeros((0, self.P, 4), f32), np.zeros((0, self.P, 4, 4), f32)
        return tuple(np.stack([self.state[t][k] for t in ids]) for k in range(3))

    def weights(self, pl, k, poses, present):
        """the gated weight matrix of named scene k -> (w [m, T], refused [m, T], ungated w)"""
        import pose_ref as PR

        has, mean, cov = self.states_of(pl["tracks"][k])
        m = len(poses)
        if m == 0 or len(has) == 0:
            z = np.full((m, len(has)), np.nan, f32)
            return z, np.zeros((m, len(has)), bool), z
        w = PR.weights(poses, present, has, mean, cov, self.pw, self.min_common)
        g, no = gate(w, poses, present, has, mean, pl["limits"][k])
        return g, no, w

    def vote(self, pl, k, poses, present):
        import pose_ref as PR

        w = self.weights(pl, k, poses, present)[0]
        if w.shape[0] == 0 or w.shape[1] == 0:
            return np.full(w.shape[0], -1, np.int64)
        return PR.vote(w, self.threshold)[1]

    # -- the life cycle alone: cols [scene][pose] the column the vote gave, -1 none --
    def apply(self, scene_ids, pl, cols):
        """-> (records per scene: (id, scene, epoch, length, created) per pose; matched ids; created ids; coasting ids)"""
        for s, e in zip(scene_ids, pl["epoch"]):
            self.epochs[s] = e
            self.lists.setdefault(s, [])
        for t in pl["expired"]:
            self.lists[self.rec[t]["scene"]].remove(t)
            self.wasted.append(dict(id=t, state=self.state.pop(t, None), **self.rec.pop(t)))
        self.remove_from_order(pl["expired"])
        out, matched, created, listed = [], [], [], []
        for s, e, tracks, c in zip(scene_ids, pl["epoch"], pl["tracks"], cols):
            recs = []
            listed += tracks
            for col in c:
                if 0 <= col < len(tracks):
                    t = tracks[int(col)]
                    self.rec[t]["last"], self.rec[t]["length"] = e, self.rec[t]["length"] + 1
                    matched.append(t)
                    recs.append((t, s, e, self.rec[t]["length"], 0))
                else:
                    t = self.next_id + len(created)
                    created.append(t)
                    self.rec[t] = dict(scene=s, first=e, last=e, length=1)
                    self.lists[s].append(t)
                    self.order.append(t)
                    recs.append((t, s, e, 1, 1))
            out.append(recs)
        self.next_id += len(created)
        coasting = [t for t in listed if t not in set(matched)] if self.coast else []
        return out, matched, created, coasting

    # -- a whole frame: frame = [(scene, poses [m, P, 2], present [m, P]), ...] --
    def predict(self, frame, cols=None):
        scene_ids = [f[0] for f in frame]
        pl = self.plan(scene_ids)
        if cols is None:
            cols = [self.vote(pl, k, f[1], f[2]) for k, f in enumerate(frame)]
        out, matched, created, coasting = self.apply(scene_ids, pl, cols)
        ids = [r[0] for recs in out for r in recs]
        if ids:   # ONE step over every pose's track
            z = np.concatenate([np.asarray(f[1], f32).reshape(-1, self.P, 2) for f in frame])
            pres = np.concatenate([np.asarray(f[2], bool).reshape(-1, self.P) for f in frame]) & np.isfinite(z).all(-1)
            b = R.Bank((len(ids), self.P), self.pw, self.vw)
            for r, t in enumerate(ids):
                if t in self.state:
                    b.has[r], b.mean[r], b.cov[r] = self.state[t]
            b.step(np.where(pres[..., None], z, f32(0)), pres)
            for r, t in enumerate(ids):
                self.state[t] = [b.has[r].copy(), b.mean[r].copy(), b.cov[r].copy()]
        if coasting:
            b = R.Bank((len(coasting), self.P), self.pw, self.vw)
            for r, t in enumerate(coasting):
                b.has[r], b.mean[r], b.cov[r] = self.state[t]
            b.predict()
            for r, t in enumerate(coasting):
                self.state[t] = [b.has[r].copy(), b.mean[r].copy(), b.cov[r].copy()]
        return out

    def skip_epochs(self, scene, n):
        self.epochs[scene] = self.epochs.get(scene, 0) + n
        self.lists.setdefault(scene, [])


# ---- scenes: cameras whose tracks have been idle 1, 2 and 4 epochs, and the frame that is then shown -------------------------------
IDLE = np.array([1, 2, 4])
WARM = 5   # warm-up epochs; the frame in question is epoch WARM + 1


def warmup(seed, shapes, P, never=0.15):
    """shapes: (m, T) per scene; scene k is camera k + 1.  T people per camera stand apart (pose_ref.people), person j is shown in every
    epoch up to WARM + 1 - IDLE[j % 3] with all points but those it never shows (`never`: their share; nobody loses all), so that in
    epoch WARM + 1 track j has been idle IDLE[j % 3] epochs.  -> (frames [WARM] of [(scene, poses, present)], centres per scene)"""
    import pose_ref as PR

    rng = np.random.default_rng(seed)
    centres, shows = [], []
    for k, (m, T) in enumerate(shapes):
        centres.append(PR.people(rng, max(T, 1), P, False)[:T] + 400.0 * k)
        nev = rng.random((T, P)) < never
        nev[nev.all(1), 0] = False
        shows.append(~nev)
    frames = []
    for e in range(1, WARM + 1):
        fr = []
        for k, (m, T) in enumerate(shapes):
            shown = np.flatnonzero(WARM + 1 - IDLE[np.arange(T) % 3] >= e)
            z = (centres[k][shown] + rng.normal(0, 0.03, (len(shown), P, 2))).astype(f32)
            fr.append((k + 1, z, shows[k][shown]))
        frames.append(fr)
    return frames, centres


def shown_frame(seed, shapes, P, centres, absent=0.4, off=1.5):
    """The frame of epoch WARM + 1: pose i of a scene continues person perm[i] (while there are people) or shows somebody new.  Of
    the continuing poses every third is where its track is with `absent` of its points missing; every third is where its track is but
    shows one or two points only — inside the chi-square gate, yet its circle is small and off the track's centre —; every third is
    moved by up to `off`.  Pose 1 of a scene has no present point, pose 2 has a NaN coordinate under a set mask bit.
    -> [(scene, poses, present)]"""
    rng = np.random.default_rng(seed + 1000)
    fr = []
    for k, (m, T) in enumerate(shapes):
        z = np.empty((m, P, 2))
        pres = rng.random((m, P)) >= absent
        src = rng.permutation(T) if T else np.zeros(0, np.int64)
        for i in range(m):
            if i < T and rng.random() >= 0.15:
                z[i] = centres[k][src[i]] + rng.normal(0, 0.05, (P, 2))
                if i % 3 == 1:
                    pres[i] = False
                    pres[i, rng.permutation(P)[: 1 + i % 2]] = True
                elif i % 3 == 2:
                    z[i] += rng.uniform(-off, off, (1, 2))
            else:
                z[i] = 5000.0 + 10.0 * i + 400.0 * k + rng.uniform(-3, 3, (P, 2))
        if m > 1:
            pres[1] = False
        if m > 2:
            z[2, 0, 0] = np.nan
            pres[2, 0] = True
        fr.append((k + 1, z.astype(f32), pres))
    return fr


def present_of(fr):
    """the presence rule on a frame: the mask and finite coordinates"""
    return [(s, z, p & np.isfinite(z).all(-1)) for s, z, p in fr]


# ---- the gated scenes of the vote test: found on the CPU, from the model alone -----------------------------------------------------
GATED_SHAPES = [(8, 9), (17, 70), (70, 17)]   # (three poses are too few for a sparse one that continues a track)
GATED_CONS = [(1, 0.3), (3, 0.6)]
_gated = {}


def gated_scenes(P=17):
    """The first seed whose warmed-up tracker (GATED_CONS) and shown frame give, in EVERY scene: a pair inside the chi-square gate that
    the limit refuses, a row whose match differs from the ungated vote, and a gated optimum in which every row is forced (forbidding
    its cell lowers kuhn_munkres's total: pose_ref's definition of unique).
    -> dict(seed, frames, frame, model: the RefSort before the frame, plan, votes: per scene (gated match, ungated match, refused inside))"""
    import pose_ref as PR

    if P in _gated:
        return _gated[P]
    for seed in range(40, 70):
        mdl = RefSort(P, WARM, GATED_CONS)
        frames, centres = warmup(seed, GATED_SHAPES, P)
        for fr in frames:
            mdl.predict(fr)
        fr = present_of(shown_frame(seed, GATED_SHAPES, P, centres))
        pl = mdl.plan([f[0] for f in fr])
        votes = []
        for k, f in enumerate(fr):
            w, no, raw = mdl.weights(pl, k, f[1], f[2])
            total, match, wq, thr_q = PR.vote(w, mdl.threshold)
            plain = PR.vote(raw, mdl.threshold)[1]
            inside = int((no & (raw > 0)).sum())
            if not (inside >= 1 and (match != plain).any() and PR.forced_rows(wq, total, match.copy()).all()):
                break
            votes.append((match, plain, inside))
        if len(votes) == len(fr):
            _gated[P] = dict(seed=seed, frames=frames, frame=fr, model=mdl, plan=pl, votes=votes)
            return _gated[P]
    raise AssertionError("no seed gives three gated scenes whose optimum is unique")


_crowd = {}


def crowd(P=2, n=150, seed=31):
    """One camera of n people in clusters tighter than the gate (pose_ref.people, crowd), every one a track after the first epoch, all of
    them shown again, in another order, under [(1, 1.0)] -> dict(frames, frame, model, plan, w, refused, match, wq, thr_q): the model's gated vote."""
    import pose_ref as PR

    if (P, n, seed) in _crowd:
        return _crowd[(P, n, seed)]
    rng = np.random.default_rng(seed)
    centres = PR.people(rng, n, P, True)
    every = np.ones((n, P), bool)
    mdl = RefSort(P, WARM, [(1, 1.0)])
    frames = [[(1, (centres + rng.normal(0, 0.03, centres.shape)).astype(f32), every)]]   # nobody has a track yet: everybody is born
    mdl.predict(frames[0])
    fr = [(1, (centres[rng.permutation(n)] + rng.normal(0, 0.04, centres.shape)).astype(f32), every)]
    pl = mdl.plan([1])
    w, no, raw = mdl.weights(pl, 0, fr[0][1], fr[0][2])
    total, match, wq, thr_q = PR.vote(w, mdl.threshold)
    _crowd[(P, n, seed)] = dict(frames=frames, frame=fr, model=mdl, plan=pl, w=w, refused=no, match=match, wq=wq, thr_q=thr_q, total=total)
    return _crowd[(P, n, seed)]
