"""The staged pruning rule of the RANSAC scoring flow as a numpy model, against the sequential oracle.

The device walks the problem's E = ceil(n / 64) point sets in a worst-first order (set_at: the ends of the two views'
lists in turn, bottom first) and prunes after every stage of the plan: with the positions [0, k) scored, h* = the first
alive hypothesis with the largest partial count, L = max(L of the stage before, full count of h*), and h stays alive iff
partial[h] + (n - done) >= L, done = the points behind the first k positions.  The last launch scores the remaining
positions for the final survivors.  What the select step then sees must have the oracle's first maximum, whatever the
order (it is a heuristic: `split` is a free parameter here) and whatever the plan.
No GPU: hypotheses from oracle.hypothesis_once, per-point decisions from oracle.score_points."""
import numpy as np
import pytest

import oracle
import synth

THR = synth.THR_5DEG
PLAN = (4, 14)             # kStagePlan in csrc/ransac.hip: a prune after the positions [0, 4) and [4, 14)
PLANS = (PLAN, (4, 8, 12, 16), (4, 8, 16), (4, 16), (4,), (1, 2, 3, 5, 7, 11))


def set_at(n, split, k):
    """The set of 64 rows behind position k of the worst-first order (score_set_at in csrc/ransac.hip); arrays broadcast."""
    n, split, k = np.asarray(n), np.asarray(split), np.asarray(k)
    E = (n + 63) // 64
    tb = split // 64
    nbot, ntop = E - 1 - tb, tb + 1      # the bottom list E-1 .. tb+1, the top list tb .. 0
    m = np.minimum(nbot, ntop)
    turn = np.where(k % 2 == 0, E - 1 - k // 2, tb - k // 2)
    tail = np.where(nbot > ntop, E - 1 - (k - m), tb - (k - m))
    return np.where((split <= 0) | (split >= n), E - 1 - k, np.where(k < 2 * m, turn, tail))


def done_points(n, k):
    """Valid points behind the first k >= 1 positions: position 0 is the one partial set."""
    E = (n + 63) // 64
    return 64 * min(k, E) - (64 * E - n)


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


def stage_model(solved, inl, split, plan=PLAN, set_at=set_at):
    """-> dict(alive [H] bool after the last prune, counts [H] what the select step sees (-1: not solved), best_iter, L,
    hstars (one per stage), scored: the (hypothesis, set) evaluations done, alive_after: survivors of each stage).
    set_at: another order with the partial set at position 0 (scripts/score_stage_model.py compares some)."""
    H, n = inl.shape
    E = (n + 63) // 64
    full = inl.sum(axis=1)
    partial = np.zeros(H, np.int64)
    alive = solved.copy()
    L, hstars, scored, alive_after = 0, [], 0, []

    def score(k0, k1):
        nonlocal scored
        for k in range(k0, min(k1, E)):
            s = int(set_at(n, split, k))
            partial[alive] += inl[alive, 64 * s: 64 * s + 64].sum(axis=1)
            scored += int(alive.sum())

    k0 = 0
    for k1 in plan:
        score(k0, k1)
        k0 = k1
        if not alive.any():
            hstars.append(-1)
            alive_after.append(0)
            continue
        hstar = int(np.argmax(np.where(alive, partial, -1)))  # first alive maximum
        hstars.append(hstar)
        L = max(L, int(full[hstar]))
        rest = n - done_points(n, k1)
        assert rest == n - sum(min(64, n - 64 * int(set_at(n, split, k))) for k in range(min(k1, E)))
        alive &= partial + rest >= L
        alive_after.append(int(alive.sum()))
    score(k0, E)
    counts = np.where(solved, partial, -1)
    return dict(alive=alive, counts=counts, best_iter=int(np.argmax(counts)) if solved.any() else -1, L=L, hstars=hstars,
                scored=scored, alive_after=alive_after)


def _check(pr, max_iter, seed, splits, plans=(PLAN,), mat=None):
    want = oracle.ransac_abs_pose(pr["f"], pr["p"], THR, max_iter, seed=seed, want_counts=True, **_okw(pr))
    solved, inl = mat if mat is not None else _inlier_matrix(pr, max_iter, seed)
    full = np.where(solved, inl.sum(axis=1), -1)
    assert np.array_equal(full, want["counts"]), "the model's inlier matrix is not the oracle's"
    out = []
    for plan in plans:
        for split in splits:
            m = stage_model(solved, inl, split, plan)
            out.append(m)
            assert int((m["counts"] >= 0).sum()) == int((want["counts"] >= 0).sum()), "number of solved hypotheses"
            if not solved.any():
                assert want["status"] == 1 and want["best_iter"] == -1 and m["best_iter"] == -1
                continue
            best = full.max()
            assert m["L"] <= best
            assert m["alive"][full >= best].all(), "a hypothesis that reaches the best count was dropped"
            assert m["best_iter"] == want["best_iter"], "best iteration, plan %r split %r" % (plan, split)
            assert m["counts"][m["best_iter"]] == want["n_inliers"] == best
            assert np.array_equal(m["counts"][m["alive"]], full[m["alive"]]), "a survivor's count is not complete"
            assert (m["counts"][~m["alive"] & solved] < m["L"]).all()
    return want, out, full


def _splits(n):
    E = (n + 63) // 64
    return sorted({0, 1, 63, 64, 65, n - 1, n, 64 * (E - 1) + max(1, (n - 64 * (E - 1)) // 2), 30} & set(range(n + 1)))


@pytest.mark.parametrize("n,E", [(40, 1), (150, 3), (256, 4), (300, 5), (512, 8), (513, 9), (768, 12), (790, 13),
                                 (896, 14), (897, 15), (1024, 16), (1030, 17), (1440, 23)])
def test_rule_for_set_counts_on_both_sides_of_every_stage(n, E):
    assert (n + 63) // 64 == E
    rng = np.random.default_rng(n)
    pr = synth.make_abs_pose_problem(rng, n, inlier_frac=0.6, noise_deg=0.25, noncentral=True, n_top=n // 2 + 7 if n > 64 else None)
    split = int(np.argmax(pr["cam"] != pr["cam"][0])) or n
    _, ms, _ = _check(pr, 100, seed=21, splits=[split, 0], plans=PLANS)
    if E > 4:
        assert not ms[0]["alive"].all(), "nothing pruned: the case does not exercise the rule"


@pytest.mark.parametrize("n", [1100, 1088])
def test_every_split(n):
    rng = np.random.default_rng(n + 1)
    pr = synth.make_abs_pose_problem(rng, n, inlier_frac=0.7, noise_deg=0.3, noncentral=True)
    splits = _splits(n)
    assert len(splits) >= 8
    _, ms, _ = _check(pr, 120, seed=5, splits=splits)
    assert not all(m["alive"].all() for m in ms)


def test_all_hypotheses_junk():
    rng = np.random.default_rng(5)
    pr = synth.make_abs_pose_problem(rng, 1100, inlier_frac=0.0, noise_deg=0.0, noncentral=True)
    want, _, full = _check(pr, 120, seed=3, splits=[550, 0])
    assert full.max() < 0.1 * 1100  # junk indeed


def test_nothing_solved():
    rng = np.random.default_rng(9)
    coll = synth.make_abs_pose_problem(rng, 1200, inlier_frac=1.0, noise_deg=0.0, noncentral=False)
    coll["p"][:] = np.outer(np.linspace(1, 2, 1200), [100.0, 200.0, 300.0])  # collinear world points: P3P has no solution
    want, ms, _ = _check(coll, 40, seed=2, splits=[1200, 600])
    assert want["status"] == 1 and not ms[0]["alive"].any() and ms[0]["hstars"] == [-1] * len(PLAN)
    few = synth.make_abs_pose_problem(rng, 3, inlier_frac=1.0, noise_deg=0.0, noncentral=False)
    _check(few, 20, seed=2, splits=[3])


def test_ties_at_the_maximum_and_L_equals_n():
    # noise-free, all inliers: every solved hypothesis counts all n points -- L == n, everything solved survives every
    # stage, and the earliest of the tied ones wins
    rng = np.random.default_rng(6)
    pr = synth.make_abs_pose_problem(rng, 1090, inlier_frac=1.0, noise_deg=0.0, noncentral=True)
    want, ms, full = _check(pr, 60, seed=8, splits=[545, 0])
    assert ms[0]["L"] == 1090 and (full == 1090).sum() >= 2
    assert want["best_iter"] == int(np.nonzero(full == 1090)[0][0])
    assert ms[0]["alive"][full == 1090].all()


def test_two_tied_below_n():
    rng = np.random.default_rng(7)
    pr = synth.make_abs_pose_problem(rng, 1200, inlier_frac=0.6, noise_deg=0.0, noncentral=True)
    want, ms, full = _check(pr, 200, seed=4, splits=[600, 0, 1200], plans=PLANS)
    best = full.max()
    tied = np.nonzero(full == best)[0]
    assert best < 1200 and len(tied) >= 2, "the case needs a tie at the maximum"
    assert want["best_iter"] == tied[0]
    for m in ms:
        assert m["alive"][tied].all() and not m["alive"].all()


def test_best_hypothesis_is_the_last_one():
    rng = np.random.default_rng(10)
    pr = synth.make_abs_pose_problem(rng, 1100, inlier_frac=0.5, noise_deg=0.3, noncentral=True)
    long_run = oracle.ransac_abs_pose(pr["f"], pr["p"], THR, 200, seed=13, want_counts=True, **_okw(pr))
    last = long_run["best_iter"]
    assert last > 10
    want, ms, _ = _check(pr, last + 1, seed=13, splits=[550, 0])  # hypotheses depend on (seed, iteration) only
    assert want["best_iter"] == last and ms[0]["alive"][last]


def test_a_stage_best_is_not_the_winner():
    # the rule must not assume that a stage's h* wins, nor that h* stays the same from stage to stage
    rng = np.random.default_rng(12)
    found = changed = False
    for seed in range(40):
        pr = synth.make_abs_pose_problem(rng, 1100, inlier_frac=0.5, noise_deg=0.4, noncentral=True)
        want, ms, _ = _check(pr, 80, seed=seed, splits=[550])
        hs = ms[0]["hstars"]
        found |= any(h != want["best_iter"] for h in hs)
        changed |= len(set(hs)) > 1
        if found and changed:
            break
    assert found and changed, "no such problem among the seeds tried"


def test_rows_in_random_order():
    # the order is a heuristic: rows in any order give the oracle's result for those rows, only less pruning
    rng = np.random.default_rng(14)
    pr = synth.make_abs_pose_problem(rng, 1285, inlier_frac=0.9, noise_deg=0.3, noncentral=True)
    # misses at the end of each view's list, as the sorted matches of the pipeline have them
    for lo, hi in ((0, 642), (642, 1285)):
        o = lo + np.argsort(~pr["is_inlier"][lo:hi], kind="stable")
        for k in ("f", "p"):
            pr[k][lo:hi] = pr[k][o]
    _, sorted_ms, _ = _check(pr, 120, seed=17, splits=[642, 0])
    perm = rng.permutation(1285)
    sh = dict(pr, f=np.ascontiguousarray(pr["f"][perm]), p=np.ascontiguousarray(pr["p"][perm]), cam=pr["cam"][perm])
    split = int(np.argmax(sh["cam"] != sh["cam"][0]))
    _, shuffled_ms, _ = _check(sh, 120, seed=17, splits=[split, 642])
    assert sorted_ms[0]["scored"] < shuffled_ms[0]["scored"], "the worst-first order is meant to prune more on sorted rows"
    assert sorted_ms[0]["scored"] < sorted_ms[1]["scored"]


def test_order_is_a_permutation_and_done_counts_the_points():
    for n in range(1, 2049):
        E = (n + 63) // 64
        split = np.arange(n + 1)[:, None]
        order = set_at(n, split, np.arange(E)[None, :])              # [split, position]
        assert np.array_equal(np.sort(order, axis=1), np.broadcast_to(np.arange(E), order.shape)), "n = %d" % n
        pts = np.cumsum(np.minimum(64, n - 64 * order), axis=1)     # valid points behind the first k + 1 positions
        want = np.array([done_points(n, k) for k in range(1, E + 1)])
        assert np.array_equal(pts, np.broadcast_to(want, pts.shape)), "n = %d" % n
    assert done_points(100, 7) == 100 and done_points(1285, 4) == 3 * 64 + 5
    assert [int(set_at(1380, 713, k)) for k in range(22)] == [21, 11, 20, 10, 19, 9, 18, 8, 17, 7, 16, 6, 15, 5, 14, 4, 13,
                                                                3, 12, 2, 1, 0]
    assert [int(set_at(300, 64, k)) for k in range(5)] == [4, 1, 3, 0, 2]
