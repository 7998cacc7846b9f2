"""From the model alone (tests/pose_sort_ref.py, no GPU): the gated scenes that tests/test_gpu_pose_sort.py compares the device's vote
with are what they claim to be.  In each of them at least one pair inside the chi-square gate is refused by the limit, the match of at
least one row differs from the ungated vote, and EVERY row of the gated optimum is forced — forbidding its cell lowers kuhn_munkres's
total —, so the GPU comparison leaves out no row: the cap on excused rows is 0, and it is met here, on the CPU."""
import numpy as np

import pose_ref as PR
import pose_sort_ref as SR


def test_the_gated_scenes_are_gated_and_their_optimum_is_unique():
    g = SR.gated_scenes(17)
    mdl, pl = g["model"], g["plan"]
    assert [len(t) for t in pl["tracks"]] == [T for _, T in SR.GATED_SHAPES] and pl["expired"] == []
    idle = {float(x) for ls in pl["limits"] for x in ls}
    assert idle == {float(np.float32(0.3)), float(np.float32(0.6)), float("inf")}   # tracks idle 1, 2 and 4 epochs
    excused = 0
    for k, f in enumerate(g["frame"]):
        w, no, raw = mdl.weights(pl, k, f[1], f[2])
        assert np.isnan(w[no]).all() and ((no & (raw > 0)).sum()) >= 1, k                    # a pair inside the gate is refused
        total, match, wq, thr_q = PR.vote(w, mdl.threshold)
        plain = PR.vote(raw, mdl.threshold)[1]
        assert (match != plain).any(), k                                                     # and the vote is another one for it
        assert (match == g["votes"][k][0]).all()
        excused += int((~PR.forced_rows(wq, total, match.copy())).sum())
        assert (match >= 0).sum() >= 3 and (match < 0).sum() >= 1, k
    assert excused == 0


def test_the_crowd_has_roots_and_refusals():
    """150 x 150 under [(1, 1.0)]: the greedy start leaves rows without their bid (the dense search runs) and the limit refuses pairs."""
    c = SR.crowd()
    assert PR.greedy_roots(c["wq"], c["thr_q"]) >= 1 and c["refused"].any() and (c["match"] >= 0).sum() >= 50
