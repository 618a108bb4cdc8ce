"""GPU: the staged scoring flow of sosvo_ransac_abs_pose gives what scoring everything gives.

From a capacity of 1024 points (16 sets of 64) a call without `hyp_counts` (fixed iteration count, identity camera
rotations, threshold below 0.5, at least 64 problems) scores the sets worst first in the stages of PLAN with a prune
after each; a call WITH counts scores everything in one launch.  Both are compared with the sequential oracle and with
each other: pose, mask, index list, inlier count and info are equal bit for bit.  The cases are those of
tests/test_ransac_stage_rule.py in batches of 64 to 70 problems (problem b samples with seed + b, so the copies of a case
draw different hypotheses)."""
import numpy as np
import pytest
import torch

import oracle
import synth

pytestmark = pytest.mark.gpu

THR = synth.THR_5DEG
KEYS = ("T", "mask", "idx", "n_inliers", "info")
PLAN = (4, 14)          # kStagePlan in csrc/ransac.hip: a boundary below the capacity's sets is a stage
STAGE_MIN_POINTS = 1024  # 64 * kStageMinSets
MIN_PROBLEMS = 64        # kPruneMinProblems


def _call(ctx, probs, S, max_iter, seed, noncentral=True, want_counts=False, seeds=None, gp3p=False):
    P = len(probs)
    f = np.zeros((P, S, 3))
    p = np.zeros((P, S, 3))
    cam = np.zeros((P, S), dtype=np.int32)
    n = np.zeros(P, dtype=np.int32)
    for b, pr in enumerate(probs):
        k = pr["f"].shape[0]
        n[b] = k
        f[b, :k], p[b, :k] = pr["f"], pr["p"]
        if noncentral:
            cam[b, :k] = pr["cam"]
    dev = ctx.device
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kw = {}
    if noncentral:
        kw = dict(cam=to(cam), cam_off=to(probs[0]["cam_off"]), cam_rot=to(probs[0]["cam_rot"]), cam_rot_identity=True)
    out = ctx.ransac_abs_pose(to(f), to(p), to(n), THR, max_iter, seed=seed, want_counts=want_counts, seeds=seeds, gp3p=gp3p,
                              **kw)
    ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(ctx, probs, S, max_iter, seed, noncentral=True, seeds=None, gp3p=False, total=MIN_PROBLEMS):
    """staged call == call with counts == oracle; the cases repeated up to `total` problems -> (records, oracle results)"""
    reps = -(-total // len(probs))
    probs = (list(probs) * reps)[:max(total, len(probs))]
    assert MIN_PROBLEMS <= len(probs) <= 70
    if seeds is not None:
        seeds = [s + 1000 * k for k in range(reps) for s in seeds][:len(probs)]
    got = _call(ctx, probs, S, max_iter, seed, noncentral, False, seeds, gp3p)
    ref = _call(ctx, probs, S, max_iter, seed, noncentral, True, seeds, gp3p)
    for k in KEYS:
        assert np.array_equal(got[k], ref[k]), "%s differs between the call without counts and the one with" % k
    wants = []
    for b, pr in enumerate(probs):
        okw = dict(cam=pr["cam"], cam_off=pr["cam_off"], cam_rot=pr["cam_rot"]) if noncentral else {}
        sb = seed + b if seeds is None else seeds[b]
        want = oracle.ransac_abs_pose(pr["f"], pr["p"], THR, max_iter, seed=sb, want_counts=True, gp3p=gp3p, **okw)
        wants.append(want)
        k = pr["f"].shape[0]
        assert np.array_equal(ref["counts"][b], want["counts"]), "hypothesis counts, problem %d" % b
        assert got["info"][b, 0] == want["best_iter"], "winning iteration, problem %d" % b
        assert got["info"][b, 1] == want["iters_used"] and got["info"][b, 2] == want["status"]
        assert got["info"][b, 3] == (want["counts"] >= 0).sum(), "solved hypotheses, problem %d" % b
        assert np.array_equal(got["mask"][b, :k].astype(bool), want["mask"]), "inlier mask, problem %d" % b
        assert got["n_inliers"][b] == want["n_inliers"]
        assert np.array_equal(got["idx"][b, : want["n_inliers"]], np.nonzero(want["mask"])[0])
        assert np.array_equal(got["T"][b], want["T"]), "RANSAC pose bits, problem %d" % b
    return got, wants


def _sorted_views(pr, n_top):
    """The rows of either view with the misses last, as the pipeline's sorted matches have them."""
    n = pr["f"].shape[0]
    for lo, hi in ((0, n_top), (n_top, n)):
        o = lo + np.argsort(~pr["is_inlier"][lo:hi], kind="stable")
        for k in ("f", "p"):
            pr[k][lo:hi] = pr[k][o]
    return pr


@pytest.mark.parametrize("S", [1024, 2048])
def test_ragged_batch_on_both_sides_of_every_stage_boundary(ctx, S):
    rng = np.random.default_rng(41)
    ns = [1, S]
    for k in PLAN + (S // 64,):
        if 64 * k <= S:
            ns += [64 * k - 65, 64 * k - 64, 64 * k - 63, 64 * k - 1, 64 * k]   # E = k - 1 (full, and one over), k
        if 64 * k + 65 <= S:
            ns += [64 * k + 1, 64 * k + 65]                                     # E = k + 1, k + 2
    ns = sorted(set(ns))
    probs = [_sorted_views(synth.make_abs_pose_problem(rng, n, inlier_frac=0.8, noise_deg=0.3, n_top=int(n * fr)), int(n * fr))
             for n, fr in zip(ns, np.linspace(0.35, 0.65, len(ns)))]
    _check(ctx, probs, S, 100, seed=5)


@pytest.mark.parametrize("S,n", [(1100, 1100), (2048, 1285)])
def test_every_split(ctx, S, n):
    rng = np.random.default_rng(42)
    E = (n + 63) // 64
    splits = [0, 1, 63, 64, 65, n - 1, n, 64 * (E - 1) + (n - 64 * (E - 1) + 1) // 2, 30]
    # (n_top = 0: every row is the bottom view's, the leading run is the whole problem)
    probs = [_sorted_views(synth.make_abs_pose_problem(rng, n, inlier_frac=0.7, noise_deg=0.3, n_top=s), s) for s in splits]
    _check(ctx, probs, S, 80, seed=11, total=66)


def test_central_and_per_problem_seeds(ctx):
    rng = np.random.default_rng(43)
    probs = [synth.make_abs_pose_problem(rng, n, inlier_frac=0.5, noise_deg=0.2, noncentral=False) for n in (1200, 300, 1025)]
    _check(ctx, probs, 1200, 130, seed=9, noncentral=False)       # cam == NULL
    _check(ctx, probs, 1200, 130, seed=0, noncentral=False, seeds=[2 ** 63 + 5, 17, 123456789])
    both = [synth.make_abs_pose_problem(rng, n, inlier_frac=0.6, noise_deg=0.2) for n in (1285, 700, 1030)]
    _check(ctx, both, 1285, 40, seed=0, seeds=[3, 2 ** 40, 99], total=65)


def test_gp3p(ctx):
    rng = np.random.default_rng(44)
    probs = [_sorted_views(synth.make_abs_pose_problem(rng, n, inlier_frac=0.7, noise_deg=0.2, n_top=t), t)
             for n, t in ((1285, 640), (1024, 100), (500, 250), (1100, 1099))]
    _check(ctx, probs, 1285, 60, seed=7, gp3p=True)


def _collinear(rng, n):
    pr = synth.make_abs_pose_problem(rng, n, inlier_frac=1.0, noise_deg=0.0, noncentral=True)
    pr["p"][:] = np.outer(np.linspace(1, 2, n), [100.0, 200.0, 300.0])  # no P3P solution
    return pr


def test_hard_cases_in_one_batch(ctx):
    rng = np.random.default_rng(45)
    mk = synth.make_abs_pose_problem
    shuffled = mk(rng, 1285, inlier_frac=0.9, noise_deg=0.3)
    perm = rng.permutation(1285)
    shuffled = dict(shuffled, f=np.ascontiguousarray(shuffled["f"][perm]), p=np.ascontiguousarray(shuffled["p"][perm]),
                    cam=np.ascontiguousarray(shuffled["cam"][perm]))
    probs = [
        mk(rng, 1100, inlier_frac=0.0, noise_deg=0.0),                # all junk
        mk(rng, 1090, inlier_frac=1.0, noise_deg=0.0),                # L == n, every solved hypothesis tied
        mk(rng, 1200, inlier_frac=0.6, noise_deg=0.0),                # ties at the maximum below n
        _collinear(rng, 1150),                                        # no solved hypothesis
        mk(rng, 3, inlier_frac=1.0, noise_deg=0.0, n_top=3),          # too few points to sample
        dict(f=np.zeros((0, 3)), p=np.zeros((0, 3)), cam=np.zeros(0, np.int32), cam_off=None, cam_rot=None),
        shuffled,                                                     # rows in random order: both cameras everywhere
        _sorted_views(mk(rng, 1285, inlier_frac=0.9, noise_deg=0.3, n_top=642), 642),   # the bench's shape
        mk(rng, 1100, inlier_frac=0.5, noise_deg=0.4),                # a stage's best is often not the winner
    ]
    probs[5]["cam_off"], probs[5]["cam_rot"] = probs[0]["cam_off"], probs[0]["cam_rot"]
    got, wants = _check(ctx, probs, 1285, 160, seed=40, total=66)
    full = wants[2]["counts"]
    assert (full == full.max()).sum() >= 2 and full.max() < 1200, "problem 2 is meant to have a tie at the maximum"
    assert wants[1]["n_inliers"] == 1090 and wants[3]["status"] == 1 and wants[4]["status"] == 1 and wants[5]["status"] == 1


def test_best_hypothesis_is_the_last_one(ctx):
    rng = np.random.default_rng(11)
    pr = synth.make_abs_pose_problem(rng, 1100, inlier_frac=0.5, noise_deg=0.3)
    last = oracle.ransac_abs_pose(pr["f"], pr["p"], THR, 160, seed=13, cam=pr["cam"], cam_off=pr["cam_off"],
                                  cam_rot=pr["cam_rot"])["best_iter"]
    assert last >= 40
    got, _ = _check(ctx, [pr], 1100, last + 1, seed=13)
    assert got["info"][0, 0] == last


def test_capacity_threshold_both_sides(ctx):
    # a capacity of 1023 points keeps the probe / rest flow, 1024 runs the stages: the same problems through both
    rng = np.random.default_rng(46)
    probs = [_sorted_views(synth.make_abs_pose_problem(rng, n, inlier_frac=0.7, noise_deg=0.25), n // 2)
             for n in (1023, 1000, 961, 600, 257, 40)]
    a, _ = _check(ctx, probs, STAGE_MIN_POINTS - 1, 120, seed=3)
    b, _ = _check(ctx, probs, STAGE_MIN_POINTS, 120, seed=3)
    for k in ("T", "n_inliers", "info"):
        assert np.array_equal(a[k], b[k])
    assert np.array_equal(a["mask"], b["mask"][:, :STAGE_MIN_POINTS - 1])


def test_launches_are_the_plans(ctx):
    # the per-launch profile names the kernels of a call: their number depends on the capacity alone
    rng = np.random.default_rng(47)
    probs = [synth.make_abs_pose_problem(rng, 300, inlier_frac=0.5, noise_deg=0.2)] * MIN_PROBLEMS

    def launches(S, **kw):
        ctx.profile_enable(True)
        try:
            _call(ctx, probs, S, 40, 1, **kw)
            labels = [name for name, _ in ctx.profile_read()]
        finally:
            ctx.profile_enable(False)
        return sum("ransac_score_kernel" in name for name in labels), labels.count("ransac_prune_kernel")

    for S in (1024, 1025, 1285, 2048, 4096):
        stages = sum(k < -(-S // 64) for k in PLAN)
        assert launches(S) == (stages + 1, stages), "capacity %d" % S
    assert launches(1024) == (3, 2) and launches(2048) == (3, 2)
    assert launches(512) == (2, 1) and launches(1023) == (2, 1)
    assert launches(511) == (1, 0)
    assert launches(1024, want_counts=True) == (1, 0)
