"""From the model alone (tests/oks_ref.py, no GPU): the scenes that tests/test_gpu_oks.py compares the device's OKS vote with are what
they claim to be.  EVERY row of every optimum is forced — forbidding its cell lowers kuhn_munkres's total —, so the GPU comparison
leaves out no row: the cap on excused rows is 0, and it is met here, on the CPU.  The OKS vote is another vote than the Mahalanobis
one, the crowd's greedy start leaves rows without their bid, and the gated tracker frames refuse pairs that OKS alone would take."""
import numpy as np
import pytest

import oks_ref as OR
import pose_ref as PR
import pose_sort_ref as SR


@pytest.mark.parametrize("P", [2, 17])
def test_every_row_of_the_vote_scenes_is_forced_and_oks_is_another_vote(P):
    excused = differs = 0
    for m, T in OR.VOTE_SHAPES:
        sc = OR.scene(m, T, P, crowd=True)
        total, match, wq, thr_q = sc.vote()
        excused += int((~PR.forced_rows(wq, total, match.copy())).sum())
        assert (match >= 0).sum() >= 2, (m, T)
        differs += int((match != PR.vote(sc.mahalanobis(), 1.0)[1]).any())
        w = sc.weights()
        real = w[~np.isnan(w)]
        assert ((real >= 0) & (real <= 1)).all() and (real > OR.THRESHOLD).any()
    assert excused == 0
    assert differs >= 1   # at least one scene where the OKS vote is not the Mahalanobis vote


def test_the_crowd_has_roots_and_a_unique_optimum():
    m, T, P = OR.CROWD
    sc = OR.scene(m, T, P, crowd=True)
    total, match, wq, thr_q = sc.vote()
    assert PR.greedy_roots(wq, thr_q) >= 1 and (match >= 0).sum() >= 50
    assert PR.forced_rows(wq, total, match.copy()).all()


@pytest.mark.parametrize("gated", [False, True])
def test_the_tracker_frames_expire_refuse_and_have_unique_optima(gated):
    mdl = OR.sort_model(gated)
    excused = refused_above = expired = changed = voted = 0
    for fr in OR.sort_frames():
        fr = SR.present_of(fr)
        pl = mdl.plan([f[0] for f in fr])
        expired += len(pl["expired"])
        for k, f in enumerate(fr):
            w, no, raw = mdl.weights(pl, k, f[1], f[2])
            if w.size == 0:
                continue
            total, match, wq, thr_q = PR.vote(w, mdl.threshold)
            excused += int((~PR.forced_rows(wq, total, match.copy())).sum())
            with np.errstate(invalid="ignore"):
                refused_above += int((no & (raw > np.float32(mdl.threshold))).sum())
            changed += int((match != PR.vote(raw, mdl.threshold)[1]).any())
            voted += 1
        mdl.predict(fr)
    assert excused == 0 and voted == 2 * (OR.SORT_FRAMES - 1)
    assert expired >= 2 and len(mdl.wasted) == expired
    if gated:
        assert refused_above >= 1 and changed >= 1   # pairs OKS alone would take; a frame whose vote the gate changes
    else:
        assert refused_above == 0
