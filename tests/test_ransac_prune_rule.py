"""The pruning rule of the RANSAC scoring flow as a numpy model, against the sequential oracle.

The device scores every hypothesis on a probe of the first min(n, 256) points, takes h* = the first solved hypothesis with
the largest probe count, L = the full count of h*, and scores the remaining points only for the hypotheses with
probe + (n - probe points) >= L.  Two properties make the result what it was:
  1. no hypothesis whose full count reaches the best one is dropped (ties included: one of them may be the first maximum);
  2. the first maximum over the survivors' exact counts is the oracle's best_iter (and a dropped hypothesis, left with its
     probe count, stays strictly below it).
No GPU: hypotheses from oracle.hypothesis_once, per-point decisions from oracle.score_points."""
import numpy as np
import pytest

import oracle
import synth

PROBE_POINTS = 256  # kProbeSets * 64 in csrc/ransac.hip
THR = synth.THR_5DEG


def _okw(pr):
    return dict(cam=pr["cam"], cam_off=pr["cam_off"], cam_rot=pr["cam_rot"]) if pr["cam"] is not None else {}


def _inlier_matrix(pr, max_iter, seed):
    """-> (solved [H] bool, inl [H, n] bool) by the oracle's own hypothesis generator and score."""
    n = pr["f"].shape[0]
    solved = np.zeros(max_iter, bool)
    inl = np.zeros((max_iter, n), bool)
    for it in range(max_iter):
        ok, T, _ = oracle.hypothesis_once(pr["f"], pr["p"], seed, it, **_okw(pr))
        solved[it] = ok
        if ok and n:
            inl[it] = oracle.score_points(pr["f"], pr["p"], T, **_okw(pr)) < THR
    return solved, inl


def prune_model(solved, inl, probe_points=PROBE_POINTS):
    """-> dict(alive [H] bool, counts [H] what the select step sees (-1: not solved), best_iter, L, hstar)."""
    H, n = inl.shape
    pn = min(n, probe_points)
    probe = np.where(solved, inl[:, :pn].sum(axis=1), -1)
    if not solved.any():
        return dict(alive=np.zeros(H, bool), counts=probe, best_iter=-1, L=None, hstar=-1)
    hstar = int(np.argmax(probe))  # first maximum; unsolved ones sit at -1
    L = int(inl[hstar].sum())
    alive = solved & (probe + (n - pn) >= L)
    counts = np.where(alive, inl.sum(axis=1), probe)
    return dict(alive=alive, counts=counts, best_iter=int(np.argmax(counts)), L=L, hstar=hstar)


def _check(pr, max_iter, seed):
    want = oracle.ransac_abs_pose(pr["f"], pr["p"], THR, max_iter, seed=seed, want_counts=True, **_okw(pr))
    solved, inl = _inlier_matrix(pr, max_iter, seed)
    full = np.where(solved, inl.sum(axis=1), -1)
    assert np.array_equal(full, want["counts"]), "the model's inlier matrix is not the oracle's"
    m = prune_model(solved, inl)
    if not solved.any():
        assert want["status"] == 1 and want["best_iter"] == -1 and m["best_iter"] == -1
        return want, m, full
    best = full.max()
    assert m["L"] <= best
    # 1. nothing that reaches the best count is dropped
    assert m["alive"][full >= best].all()
    # 2. the first maximum over the survivors' exact counts is the oracle's winner ...
    surv = np.where(m["alive"], full, -1)
    assert int(np.argmax(surv)) == want["best_iter"]
    # ... and what the select step sees (dropped ones keep their probe count) has the same first maximum
    assert m["best_iter"] == want["best_iter"]
    assert (m["counts"][~m["alive"] & solved] < m["L"]).all()
    return want, m, full


@pytest.mark.parametrize("n,frac,noise,noncentral,n_top", [
    (1285, 0.9, 0.3, True, None),    # the bench's size: a straddling set, good and junk hypotheses
    (700, 0.35, 0.2, True, 100),
    (600, 0.5, 0.1, False, None),
    (2048, 0.6, 0.2, True, 2047),
])
def test_rule_on_synthetic_problems(n, frac, noise, noncentral, n_top):
    rng = np.random.default_rng(n)
    pr = synth.make_abs_pose_problem(rng, n, inlier_frac=frac, noise_deg=noise, noncentral=noncentral, n_top=n_top)
    _, m, _ = _check(pr, 150, seed=21)
    assert not m["alive"].all(), "nothing pruned: the case does not exercise the rule"


def test_all_hypotheses_junk():
    rng = np.random.default_rng(5)
    pr = synth.make_abs_pose_problem(rng, 900, inlier_frac=0.0, noise_deg=0.0, noncentral=True)
    want, m, full = _check(pr, 120, seed=3)
    assert full.max() < 0.1 * 900  # junk indeed


def test_ties_at_the_maximum_and_L_equals_n():
    # noise-free, all inliers: every solved hypothesis counts all n points -- L == n, everything solved survives, and the
    # earliest of the tied ones wins
    rng = np.random.default_rng(6)
    pr = synth.make_abs_pose_problem(rng, 640, inlier_frac=1.0, noise_deg=0.0, noncentral=True)
    want, m, full = _check(pr, 60, seed=8)
    assert m["L"] == 640 and (full == 640).sum() >= 2
    assert want["best_iter"] == int(np.nonzero(full == 640)[0][0])
    assert m["alive"][full == 640].all()


def test_two_tied_below_n():
    # noise-free inliers among outliers: the all-inlier samples recover the same pose and tie at a count below n
    rng = np.random.default_rng(7)
    pr = synth.make_abs_pose_problem(rng, 800, inlier_frac=0.6, noise_deg=0.0, noncentral=True)
    want, m, full = _check(pr, 200, seed=4)
    best = full.max()
    tied = np.nonzero(full == best)[0]
    assert best < 800 and len(tied) >= 2, "the case needs a tie at the maximum"
    assert want["best_iter"] == tied[0] and m["alive"][tied].all()
    assert not m["alive"].all()


@pytest.mark.parametrize("n", [100, 255, 256, 257])
def test_n_below_at_and_just_above_the_probe(n):
    rng = np.random.default_rng(n)
    pr = synth.make_abs_pose_problem(rng, n, inlier_frac=0.5, noise_deg=0.2, noncentral=True)
    _, m, full = _check(pr, 120, seed=11)
    if n <= PROBE_POINTS:  # the probe is the whole problem: only the hypotheses tied with h* are left, nothing to rescore
        assert np.array_equal(m["counts"], full)


def test_no_solved_hypothesis():
    rng = np.random.default_rng(9)
    coll = synth.make_abs_pose_problem(rng, 600, inlier_frac=1.0, noise_deg=0.0, noncentral=False)
    coll["p"][:] = np.outer(np.linspace(1, 2, 600), [100.0, 200.0, 300.0])  # collinear world points: P3P has no solution
    want, m, _ = _check(coll, 40, seed=2)
    assert want["status"] == 1 and not m["alive"].any()
    few = synth.make_abs_pose_problem(rng, 3, inlier_frac=1.0, noise_deg=0.0, noncentral=False)
    _check(few, 20, seed=2)


def test_best_hypothesis_is_the_last_one():
    rng = np.random.default_rng(10)
    pr = synth.make_abs_pose_problem(rng, 1000, inlier_frac=0.5, noise_deg=0.3, noncentral=True)
    long_run = oracle.ransac_abs_pose(pr["f"], pr["p"], THR, 200, seed=13, want_counts=True, **_okw(pr))
    last = long_run["best_iter"]
    assert last > 10
    want, m, _ = _check(pr, last + 1, seed=13)  # hypotheses depend on (seed, iteration) only: the same ones, cut short
    assert want["best_iter"] == last and m["alive"][last]


def test_probe_winner_is_not_the_overall_winner():
    # the rule must not assume h* wins: here the best probe count and the best full count belong to different hypotheses
    rng = np.random.default_rng(12)
    found = False
    for seed in range(40):
        pr = synth.make_abs_pose_problem(rng, 900, inlier_frac=0.5, noise_deg=0.4, noncentral=True)
        want, m, _ = _check(pr, 80, seed=seed)
        if m["hstar"] != want["best_iter"]:
            found = True
            break
    assert found, "no such problem among the seeds tried"
