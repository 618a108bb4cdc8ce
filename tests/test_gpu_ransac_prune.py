"""GPU: the pruned scoring flow of sosvo_ransac_abs_pose gives what scoring everything gives.

A call without `hyp_counts` (fixed iteration count, identity camera rotations, threshold below 0.5, a capacity of at
least 512 points, at least 64 problems) scores a probe of 256 points, prunes, and scores the rest for the survivors; a
call WITH counts scores everything in one launch as before.  Both are compared with the sequential oracle and with each other: pose, mask,
index list, inlier count and info are equal bit for bit.  The cases are those of tests/test_ransac_prune_rule.py plus
ragged batches, n from 1 to 2048, both cameras, and the calls that must keep the old path.  Every batch is the list of
cases repeated up to 64 problems (problem b samples with seed + b, so the copies draw different hypotheses)."""
import numpy as np
import pytest
import torch

import oracle
import synth

pytestmark = pytest.mark.gpu

THR = synth.THR_5DEG
KEYS = ("T", "mask", "idx", "n_inliers", "info")
MIN_PROBLEMS = 64  # kPruneMinProblems in csrc/ransac.hip: smaller batches keep the single launch


def _collinear(rng, n):
    pr = synth.make_abs_pose_problem(rng, n, inlier_frac=1.0, noise_deg=0.0, noncentral=True)
    pr["p"][:] = np.outer(np.linspace(1, 2, n), [100.0, 200.0, 300.0])  # no P3P solution
    return pr


def _call(ctx, probs, S, max_iter, seed, noncentral=True, want_counts=False, adaptive=False, seeds=None, thr=THR):
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
    out = ctx.ransac_abs_pose(to(f), to(p), to(n), thr, max_iter, seed=seed, adaptive=adaptive, want_counts=want_counts,
                              seeds=seeds, **kw)
    ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(ctx, probs, S, max_iter, seed, noncentral=True, adaptive=False, seeds=None, thr=THR, tile=True):
    """pruned call == call with counts == oracle; -> (records of the call without counts, oracle results)"""
    if tile:
        reps = -(-MIN_PROBLEMS // len(probs))
        probs = list(probs) * reps
        seeds = None if seeds is None else [s + 1000 * k for k in range(reps) for s in seeds]
    got = _call(ctx, probs, S, max_iter, seed, noncentral, False, adaptive, seeds, thr)
    ref = _call(ctx, probs, S, max_iter, seed, noncentral, True, adaptive, seeds, thr)
    for k in KEYS:
        assert np.array_equal(got[k], ref[k]), "%s differs between the call without counts and the one with" % k
    wants = []
    for b, pr in enumerate(probs):
        okw = dict(cam=pr["cam"], cam_off=pr["cam_off"], cam_rot=pr["cam_rot"]) if noncentral else {}
        sb = seed + b if seeds is None else seeds[b]
        want = oracle.ransac_abs_pose(pr["f"], pr["p"], thr, max_iter, seed=sb, adaptive=adaptive, want_counts=True, **okw)
        wants.append(want)
        k = pr["f"].shape[0]
        used = want["iters_used"]
        assert np.array_equal(ref["counts"][b, :used], want["counts"][:used]), "hypothesis counts, problem %d" % b
        assert got["info"][b, 0] == want["best_iter"], "winning iteration, problem %d" % b
        assert got["info"][b, 1] == used and got["info"][b, 2] == want["status"]
        if not adaptive:  # (with the adaptive stop the device still solves all max_iter samples and reports those)
            assert got["info"][b, 3] == (want["counts"] >= 0).sum(), "solved hypotheses, problem %d" % b
        assert np.array_equal(got["mask"][b, :k].astype(bool), want["mask"]), "inlier mask, problem %d" % b
        assert got["n_inliers"][b] == want["n_inliers"]
        assert np.array_equal(got["idx"][b, : want["n_inliers"]], np.nonzero(want["mask"])[0])
        assert np.array_equal(got["T"][b], want["T"]), "RANSAC pose bits, problem %d" % b
    return got, wants


def test_hard_cases_in_one_ragged_batch(ctx):
    rng = np.random.default_rng(31)
    mk = synth.make_abs_pose_problem
    probs = [
        mk(rng, 900, inlier_frac=0.0, noise_deg=0.0),                 # all junk
        mk(rng, 640, inlier_frac=1.0, noise_deg=0.0),                 # L == n, every solved hypothesis tied
        mk(rng, 800, inlier_frac=0.6, noise_deg=0.0),                 # ties at the maximum below n
        mk(rng, 100, inlier_frac=0.5, noise_deg=0.2),                 # below the probe
        mk(rng, 255, inlier_frac=0.5, noise_deg=0.2),
        mk(rng, 256, inlier_frac=0.5, noise_deg=0.2),                 # exactly the probe
        mk(rng, 257, inlier_frac=0.5, noise_deg=0.2),                 # one point left for the rest pass
        _collinear(rng, 600),                                         # no solved hypothesis
        mk(rng, 3, inlier_frac=1.0, noise_deg=0.0, n_top=3),          # too few points to sample
        dict(f=np.zeros((0, 3)), p=np.zeros((0, 3)), cam=np.zeros(0, np.int32), cam_off=None, cam_rot=None),
        mk(rng, 1285, inlier_frac=0.9, noise_deg=0.3),                # the bench's size: 21 sets, two point blocks
        mk(rng, 1024, inlier_frac=0.35, noise_deg=0.2, n_top=0),      # bottom camera only
        mk(rng, 1023, inlier_frac=0.35, noise_deg=0.2, n_top=1023),   # top camera only
    ]
    probs[9]["cam_off"], probs[9]["cam_rot"] = probs[0]["cam_off"], probs[0]["cam_rot"]
    got, wants = _check(ctx, probs, 1285, 200, seed=40)
    full = wants[2]["counts"]
    assert (full == full.max()).sum() >= 2 and full.max() < 800, "problem 2 is meant to have a tie at the maximum"
    assert wants[1]["n_inliers"] == 640 and wants[7]["status"] == 1 and wants[8]["status"] == 1 and wants[9]["status"] == 1


def test_n_from_1_to_2048(ctx):
    rng = np.random.default_rng(32)
    ns = [1, 2, 4, 63, 64, 65, 192, 320, 511, 512, 513, 1087, 1088, 1089, 1280, 2047, 2048]
    probs = [synth.make_abs_pose_problem(rng, n, inlier_frac=0.45, noise_deg=0.25, n_top=int(n * fr))
             for n, fr in zip(ns, np.linspace(0.0, 1.0, len(ns)))]
    _check(ctx, probs, 2048, 140, seed=5)


def test_central_and_per_problem_seeds(ctx):
    rng = np.random.default_rng(33)
    probs = [synth.make_abs_pose_problem(rng, n, inlier_frac=0.5, noise_deg=0.2, noncentral=False) for n in (600, 300, 777)]
    _check(ctx, probs, 777, 130, seed=9, noncentral=False)
    _check(ctx, probs, 777, 130, seed=0, noncentral=False, seeds=[2 ** 63 + 5, 17, 123456789])


def test_best_hypothesis_is_the_last_one(ctx):
    rng = np.random.default_rng(10)
    pr = synth.make_abs_pose_problem(rng, 1000, inlier_frac=0.5, noise_deg=0.3)
    last = oracle.ransac_abs_pose(pr["f"], pr["p"], THR, 200, seed=13, cam=pr["cam"], cam_off=pr["cam_off"],
                                  cam_rot=pr["cam_rot"])["best_iter"]
    assert last > 10
    got, _ = _check(ctx, [pr], 1000, last + 1, seed=13)
    assert got["info"][0, 0] == last


def test_capacity_and_batch_thresholds_both_sides(ctx):
    # a capacity below 512 points keeps the single launch, 512 takes the pruned flow: the same problems through both
    rng = np.random.default_rng(34)
    probs = [synth.make_abs_pose_problem(rng, n, inlier_frac=0.5, noise_deg=0.2) for n in (500, 511, 257, 40)]
    a, _ = _check(ctx, probs, 511, 120, seed=3)
    b, _ = _check(ctx, probs, 512, 120, seed=3)
    for k in ("T", "n_inliers", "info"):
        assert np.array_equal(a[k], b[k])
    # ... and so does a batch of fewer than 64 problems
    c, _ = _check(ctx, (probs * 16)[:63], 512, 120, seed=3, tile=False)
    for k in ("T", "n_inliers", "info"):
        assert np.array_equal(b[k][:63], c[k])


def test_adaptive_and_fp64_only_keep_the_old_path(ctx):
    # adaptive stop: the replay reads every count up to the stop, so nothing may be pruned -- the records are those of the
    # call with counts and of the oracle's sequential loop (an early stop included)
    rng = np.random.default_rng(35)
    probs = [synth.make_abs_pose_problem(rng, n, inlier_frac=fr, noise_deg=0.2) for n, fr in ((1285, 0.9), (900, 0.4), (600, 0.0))]
    got, wants = _check(ctx, probs, 1285, 160, seed=6, adaptive=True)
    assert wants[0]["iters_used"] < 160, "the case is meant to stop early"
    fixed, _ = _check(ctx, probs, 1285, 160, seed=6)
    ctx.set_hint_score_fp64_only(True)
    try:
        slow, _ = _check(ctx, probs, 1285, 160, seed=6)
    finally:
        ctx.set_hint_score_fp64_only(False)
    for k in KEYS:
        assert np.array_equal(fixed[k], slow[k])
    # a threshold of 0.5 and above has no single-precision tier and no pruning
    _check(ctx, probs[:2], 1285, 60, seed=6, thr=0.6)


def test_which_calls_take_the_pruned_flow(ctx):
    # the per-launch profile names the kernels of a call: ransac_prune_kernel runs exactly where the rule may be used
    rng = np.random.default_rng(36)
    probs = [synth.make_abs_pose_problem(rng, 300, inlier_frac=0.5, noise_deg=0.2)] * MIN_PROBLEMS

    def pruned(probs=probs, S=512, **kw):
        ctx.profile_enable(True)
        try:
            _call(ctx, probs, S, 40, 1, **kw)
            labels = [name for name, _ in ctx.profile_read()]
        finally:
            ctx.profile_enable(False)
        assert sum("ransac_score_kernel" in name for name in labels) == (2 if "ransac_prune_kernel" in labels else 1)
        return "ransac_prune_kernel" in labels

    assert pruned()
    assert not pruned(want_counts=True)
    assert not pruned(adaptive=True)
    assert not pruned(probs=probs[:-1])
    assert not pruned(S=511)
    assert not pruned(thr=0.6)
    ctx.set_hint_score_fp64_only(True)
    try:
        assert not pruned()
    finally:
        ctx.set_hint_score_fp64_only(False)
