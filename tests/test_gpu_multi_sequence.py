"""GPU: several sequences ("lanes") through one engine -- the per-problem seeds of the RANSAC, the ..._front_end_slots /
..._track_seeds / ..._copy_slots entry points, pipeline.MultiSequenceEngine / RGBDMultiSequenceEngine against the
single-sequence engines, and run_VO_many / the demos against solo runs.

Everything is compared bit for bit or byte for byte: a frame record is a function of its image only and a tracking record
of (reference record, current record, seed) only, so the launch that computes a record cannot change it.

Seeds of the synthetic sequences (synthetic.write_sos_sequence / write_rgbd_sequence, steps |t| <= 40 mm, <= 2 degrees):
SOS 77, 5 and 61, RGB-D 41 and 43 -- the seeds tests/test_gpu_sequence.py tracks over their whole length."""
import os

import numpy as np
import pytest
import torch

import matching_scenes as scenes
import oracle
import synth
from matching_scenes import drive as _drive, rig as _rig, sos_kwargs as _sos_kwargs
from vo_single_camera_sos_amd import synthetic
from vo_single_camera_sos_amd.device import SosvoError
from vo_single_camera_sos_amd.frontend import DeviceImageModel
from vo_single_camera_sos_amd.pipeline import (MultiSequenceEngine, RGBDCamConfig, RGBDMultiSequenceEngine, RGBDSequenceEngine,
                                               RigConfig, SequenceEngine)

pytestmark = pytest.mark.gpu

FILES = ("estimated_frame_poses_TUM.txt", "gt_associated_frame_poses_TUM.txt", "keyframe_ids.txt")
SOS_SEEDS, SOS_FRAMES = (77, 5, 61), (26, 17, 21)
RGBD_SEEDS, RGBD_FRAMES = (41, 43), (14, 10)
LIVE_THRESHOLDS = (0.05, 0.50, np.deg2rad(5.0), np.deg2rad(60.0))      # run_VO_live's


def _to(dev, *arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


# ---- 1. per-problem seeds, stage level -----------------------------------------------------------------------------
SEEDS = [7, 2 ** 40 + 3, 7, 0, 2 ** 63 + 11, 5]      # non-monotonic, repeated, beyond 2^32 and 2^63


def _pack(problems, S, noncentral):
    P = len(problems)
    f, p = np.zeros((P, S, 3)), np.zeros((P, S, 3))
    cam, n = np.zeros((P, S), dtype=np.int32), np.zeros(P, dtype=np.int32)
    for b, pr in enumerate(problems):
        k = pr["f"].shape[0]
        n[b] = k
        f[b, :k], p[b, :k] = pr["f"], pr["p"]
        if noncentral:
            cam[b, :k] = pr["cam"]
    return f, p, cam, n


@pytest.mark.parametrize("solver", ["p3p_one_mirror", "gp3p_noncentral", "gp3p_central", "epnp", "twopt"])
@pytest.mark.parametrize("adaptive", [False, True])
def test_per_problem_seeds_equal_the_oracle_problem_by_problem(ctx, solver, adaptive):
    """Problem b of sosvo_ransac_abs_pose_seeds == oracle.ransac_abs_pose on problem b alone with seed = seeds[b]: pose,
    inlier mask, inlier list, count, info and every hypothesis count, bit for bit; and seeds[b] = seed + b reproduces the
    scalar entry."""
    noncentral = solver in ("p3p_one_mirror", "gp3p_noncentral")
    flags = dict(epnp=solver == "epnp", gp3p=solver.startswith("gp3p"), twopt=solver == "twopt")
    rng = np.random.default_rng(17)
    sizes = [(300, 0.5), (64, 0.9), (257, 0.4), (500, 0.7), (33, 1.0), (120, 0.6)]
    probs = [synth.make_abs_pose_problem(rng, n, inlier_frac=fr, noise_deg=0.2, noncentral=noncentral) for n, fr in sizes]
    S, max_iter, thr = 512, 120, synth.THR_5DEG
    f, p, cam, n = _pack(probs, S, noncentral)
    tf, tp, tcam, tn = _to(ctx.device, f, p, cam, n)
    kw = dict(adaptive=adaptive, want_counts=True, **flags)
    if noncentral:
        off, rot = _to(ctx.device, probs[0]["cam_off"], probs[0]["cam_rot"])
        kw.update(cam=tcam, cam_off=off, cam_rot=rot, cam_rot_identity=True)
    out = ctx.ransac_abs_pose_seeds(tf, tp, tn, thr, max_iter, SEEDS, **kw)
    ctx.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for b, pr in enumerate(probs):
        okw = dict(cam=pr["cam"], cam_off=pr["cam_off"], cam_rot=pr["cam_rot"]) if noncentral else {}
        want = oracle.ransac_abs_pose(pr["f"], pr["p"], thr, max_iter, seed=SEEDS[b], adaptive=adaptive, want_counts=True,
                                      **flags, **okw)
        k, used = n[b], want["iters_used"]
        assert got["info"][b, 1] == used and got["info"][b, 0] == want["best_iter"] and got["info"][b, 2] == want["status"], b
        assert np.array_equal(got["counts"][b, :used], want["counts"][:used]), "hypothesis counts, problem %d" % b
        assert np.array_equal(got["mask"][b, :k].astype(bool), want["mask"]), "inlier mask, problem %d" % b
        assert got["n_inliers"][b] == want["n_inliers"]
        assert np.array_equal(got["idx"][b, : want["n_inliers"]], np.nonzero(want["mask"])[0])
        assert np.array_equal(got["T"][b], want["T"]), "RANSAC pose bits, problem %d" % b
    # problems 0 and 2 carry the same seed but different data; the seeds really differ between problems
    assert not np.array_equal(got["counts"][0], got["counts"][2])
    # seeds[b] = seed + b is the scalar entry, exactly -- as a device tensor this time
    base = 2 ** 33 + 9
    seeds_t = torch.from_numpy(np.array([base + b for b in range(len(probs))], dtype=np.uint64).view(np.int64)).to(ctx.device)
    a = ctx.ransac_abs_pose(tf, tp, tn, thr, max_iter, seed=base, **kw)
    b_ = ctx.ransac_abs_pose_seeds(tf, tp, tn, thr, max_iter, seeds_t, **kw)
    ctx.synchronize()
    for key in ("T", "mask", "idx", "n_inliers", "info", "counts"):
        assert torch.equal(a[key], b_[key]), key


# ---- 2. the engines against the single-sequence engines ---------------------------------------------------------------
def _lanes_against_solo(multi, solo_of, sequences, window):
    """sequences through the lanes of `multi` (one thread each) against each through solo_of() alone."""
    S = len(sequences)
    got = scenes.drive_lanes(multi, sequences, window)
    for s in range(S):
        want = _drive(solo_of(), sequences[s], window)
        assert len(got[s]) == len(want) == len(sequences[s])
        scenes.assert_same_drive(got[s], want)
        assert max(g[0] for g in got[s]) > 50
    rounds = max(-(-len(q) // window) for q in sequences)
    c = multi.counters
    assert c["front_end_launches"] == c["rounds"] == rounds, (c, rounds)        # one per round, not per lane
    assert c["speculative_track_launches"] <= 2 * rounds
    # the lanes' serial calls of one moment shared a launch: fewer launches than calls, and one held every lane
    calls = sum(len(q) - 1 for q in sequences)
    assert c["serial_track_launches"] == max(len(q) for q in sequences) - 1 < calls and c["max_serial_pairs"] == S
    assert c["copy_launches"] == 1      # every lane's frame 0, promoted, copied when the first serial call read the slot


def test_multi_sequence_engine_equals_the_single_sequence_engine(ctx):
    gs, rig_kw = _rig()
    sequences = []
    for n, seed in ((7, 61), (4, 62), (9, 63)):     # different lengths: ragged last windows, lanes end in different rounds
        room = synthetic.Room(seed=seed)
        rng = np.random.default_rng(seed + 1)
        sequences.append(np.stack([synthetic.render_omni(gs, room, R, t, 2.0, rng)
                                   for R, t in synthetic.trajectory(n, seed, max_t=40.0, max_deg=2.0)]))
    model = DeviceImageModel(ctx, gs, (480, 640))
    kw = dict(num_of_features=300, kp_cap=320, frame_cap=1024, max_iter=210, adaptive=True, ransac_solver="GP3P")
    for window in (1, 3, 4):
        multi = MultiSequenceEngine(ctx, model, RigConfig(**rig_kw), lanes=3, window=window, **kw)
        assert multi.slots == 3 * (2 * window + 1) and multi.cfg.n_pairs == 3 * window
        _lanes_against_solo(multi, lambda: SequenceEngine(ctx, model, RigConfig(**rig_kw), window=window, **kw), sequences, window)


def test_rgbd_multi_sequence_engine_equals_the_single_sequence_engine(ctx):
    cam = RGBDCamConfig(fx=554.256258, fy=554.256258, center_x=319.5, center_y=239.5, depth_is_Z=False, min_range=0.8,
                        max_range=7.0)
    sequences = []
    for n, seed in ((7, 41), (5, 43)):
        bgr, depth, _ = synthetic.make_rgbd_sequence(n, seed=seed, max_t=40.0, max_deg=2.0, depth_is_Z=False)
        sequences.append([(bgr[i], depth[i]) for i in range(n)])
    kw = dict(num_of_features=1000, max_iter=210, adaptive=True, pose_est_algorithm="EPNP")
    for window in (1, 3, 4):
        multi = RGBDMultiSequenceEngine(ctx, cam, lanes=2, window=window, **kw)
        _lanes_against_solo(multi, lambda: RGBDSequenceEngine(ctx, cam, window=window, **kw), sequences, window)


# ---- 3. bad arguments -----------------------------------------------------------------------------------------------
def test_multi_sequence_entry_points_refuse_bad_arguments(ctx):
    gs, rig_kw = _rig()
    model = DeviceImageModel(ctx, gs, (480, 640))
    eng = MultiSequenceEngine(ctx, model, RigConfig(**rig_kw), lanes=2, window=2, num_of_features=100, kp_cap=128, frame_cap=512)
    m, W, slots, ws = eng.model, eng.window, eng.slots, eng.workspace
    omni = torch.zeros((3, model.H, model.W, 3), dtype=torch.uint8, device=ctx.device)
    before = ctx.sequence_frame_counts(eng.cfg, W, slots, 0, slots, ws)

    def refused(name, call):
        with pytest.raises(SosvoError) as e:
            call()
        assert "SOSVO_ERR_ARG: " + name + ":" in str(e.value), str(e.value)     # the status, and the entry point's own name
    fe = lambda table: ctx.sequence_front_end_slots(eng.rig, eng.cfg, W, slots, omni[:len(table)], table, m.unwrap_table,  # noqa: E731
                                                    m.mask_bits, m.pattern, ws)
    refused("sosvo_sequence_front_end_slots", lambda: fe([0, 3, 0]))                  # a slot twice
    refused("sosvo_sequence_front_end_slots", lambda: fe([0, slots, 1]))              # outside the store
    refused("sosvo_sequence_front_end_slots", lambda: fe([0, -1]))
    big = torch.zeros((W + 1, model.H, model.W, 3), dtype=torch.uint8, device=ctx.device)
    refused("sosvo_sequence_front_end_slots", lambda: ctx.sequence_front_end_slots(
        eng.rig, eng.cfg, W, slots, big, list(range(W + 1)), m.unwrap_table, m.mask_bits, m.pattern, ws))   # more than the window
    cp = lambda src, dst: ctx.sequence_copy_slots(eng.cfg, W, slots, src, dst, ws)  # noqa: E731
    refused("sosvo_sequence_copy_slots", lambda: cp([0, 1], [4, 4]))                  # a destination twice
    refused("sosvo_sequence_copy_slots", lambda: cp([0, 4], [4, 9]))                  # a source that is a destination
    refused("sosvo_sequence_copy_slots", lambda: cp([3], [3]))
    refused("sosvo_sequence_copy_slots", lambda: cp([0], [slots]))
    refused("sosvo_sequence_copy_slots", lambda: cp(list(range(W + 1)), list(range(W + 1, 2 * W + 2))))   # > cfg.n_pairs
    out = torch.zeros((W + 1, 16), dtype=torch.float64, device=ctx.device)
    tr = lambda r, c, sd: ctx.sequence_track_seeds(eng.rig, eng.cfg, W, slots, r, c, sd, ws, out)  # noqa: E731
    refused("sosvo_sequence_track_seeds", lambda: tr([0] * (W + 1), [1] * (W + 1), [0] * (W + 1)))       # > cfg.n_pairs
    refused("sosvo_sequence_track_seeds", lambda: tr([0], [slots], [0]))
    # null pointers, through the raw library: the seed array of the tracking and the RANSAC entries, the slot table
    import ctypes
    from vo_single_camera_sos_amd import _lib
    lib = _lib.load()
    one = (ctypes.c_int32 * 1)(0)
    cast = lambda s_: ctypes.cast(ctypes.pointer(s_), _lib.c_p)  # noqa: E731
    P = lambda t: _lib.c_p(t.data_ptr())  # noqa: E731
    rc = lib.sosvo_sequence_track_seeds(ctx._h, cast(eng.rig), cast(eng.cfg), W, slots, ctypes.cast(one, _lib.c_p),
                                        ctypes.cast(one, _lib.c_p), None, 1, P(ws), int(ws.numel()), P(out))
    assert rc == -1 and "sosvo_sequence_track_seeds" in lib.sosvo_last_error(ctx._h).decode()
    rc = lib.sosvo_sequence_front_end_slots(ctx._h, cast(eng.rig), cast(eng.cfg), W, slots, P(omni), 1, None, P(m.unwrap_table),
                                            P(m.mask_bits), P(m.pattern), P(ws), int(ws.numel()))
    assert rc == -1 and "sosvo_sequence_front_end_slots" in lib.sosvo_last_error(ctx._h).decode()
    f = torch.zeros((1, 8, 3), dtype=torch.float64, device=ctx.device)
    n = torch.tensor([8], dtype=torch.int32, device=ctx.device)
    T, mask, idx = torch.zeros((1, 3, 4), dtype=torch.float64, device=ctx.device), torch.zeros((1, 8), dtype=torch.uint8,
                                                                                            device=ctx.device), \
        torch.zeros((1, 8), dtype=torch.int32, device=ctx.device)
    info = torch.zeros((1, 4), dtype=torch.int32, device=ctx.device)
    rc = lib.sosvo_ransac_abs_pose_seeds(ctx._h, P(f), P(f), None, None, None, 1, 0, P(n), 1, 8, 0.01, 10, 0, None, P(T), P(mask),
                                         P(idx), P(n), P(info), None)
    assert rc == -1 and "sosvo_ransac_abs_pose_seeds" in lib.sosvo_last_error(ctx._h).decode()
    # RGB-D family: the same checks, a sample of them
    cam = RGBDCamConfig(fx=554.256258, fy=554.256258, center_x=319.5, center_y=239.5, depth_is_Z=False, min_range=0.8, max_range=7.0)
    reng = RGBDMultiSequenceEngine(ctx, cam, lanes=2, window=2, num_of_features=200)
    bgr = torch.zeros((2, 480, 640, 3), dtype=torch.uint8, device=ctx.device)
    dep = torch.zeros((2, 480, 640), dtype=torch.float32, device=ctx.device)
    refused("sosvo_rgbd_sequence_front_end_slots", lambda: ctx.rgbd_sequence_front_end_slots(
        reng.cam, reng.cfg, reng.window, reng.slots, bgr, dep, [1, 1], reng.mask_bits, reng.pattern, reng.workspace))
    refused("sosvo_rgbd_sequence_copy_slots", lambda: ctx.rgbd_sequence_copy_slots(reng.cfg, reng.window, reng.slots, [0, 1], [1, 2],
                                                                                   reng.workspace))
    refused("sosvo_rgbd_sequence_track_seeds", lambda: ctx.rgbd_sequence_track_seeds(
        reng.cfg, reng.window, reng.slots, [0], [reng.slots], [0], reng.workspace, out))
    # nothing was launched: the store's counts are what they were, and the context still works
    ctx.synchronize()
    assert ctx.sequence_frame_counts(eng.cfg, W, slots, 0, slots, ws) == before


def test_copy_slots_copies_every_pair_in_one_call(ctx):
    """Two frames through the slot table into scattered slots; copy_slots to two more; tracking (copy, frame) equals
    tracking (original, frame), and the counts travel."""
    gs, rig_kw = _rig()
    room, rng = synthetic.Room(seed=61), np.random.default_rng(62)
    frames = np.stack([synthetic.render_omni(gs, room, R, t, 2.0, rng) for R, t in synthetic.trajectory(3, 61, max_t=40.0, max_deg=2.0)])
    model = DeviceImageModel(ctx, gs, (480, 640))
    eng = MultiSequenceEngine(ctx, model, RigConfig(**rig_kw), lanes=3, window=2, num_of_features=300, kp_cap=320, frame_cap=1024)
    W, slots, ws, m = eng.window, eng.slots, eng.workspace, eng.model
    omni = torch.from_numpy(frames).to(ctx.device)
    ctx.sequence_front_end_slots(eng.rig, eng.cfg, W, slots, omni, [11, 2, 7], m.unwrap_table, m.mask_bits, m.pattern, ws)
    ctx.sequence_copy_slots(eng.cfg, W, slots, [11, 2], [0, 14], ws)
    out = torch.zeros((4, 16), dtype=torch.float64, device=ctx.device)
    ctx.sequence_track_seeds(eng.rig, eng.cfg, W, slots, [11, 0, 2, 14], [7, 7, 7, 7], [5, 5, 2 ** 35, 2 ** 35], ws, out)
    counts = ctx.sequence_frame_counts(eng.cfg, W, slots, 0, slots, ws)
    rec = out.cpu().numpy()
    assert counts[0] == counts[11] > 50 and counts[14] == counts[2] > 50
    assert np.array_equal(rec[0], rec[1]) and np.array_equal(rec[2], rec[3]) and rec[0, 14] == 0 and rec[0, 12] > 30
    # and the single-sequence calls give the same records for the same (frames, seed)
    solo = SequenceEngine(ctx, model, RigConfig(**rig_kw), window=3, num_of_features=300, kp_cap=320, frame_cap=1024)
    solo.push_window(list(frames))
    assert np.array_equal(solo.track(0, 2, 5), rec[0]) and np.array_equal(solo.track(1, 2, 2 ** 35), rec[2])


def _scattered(n, slots):
    """n distinct slots spread over the store, and the slots they leave free."""
    table = [(7 * i + 3) % slots for i in range(n)]
    assert len(set(table)) == n
    return table, [v for v in range(slots) if v not in set(table)]


def test_tables_beyond_the_kernel_arguments_sos(ctx):
    """260 frames in one sosvo_sequence_front_end_slots call (the table travels 256 frames per assemble launch: the second
    launch starts at frame 256) and 20 pairs in one sosvo_sequence_copy_slots call (beyond 16 the lists are copied to the
    device): the records are those of small calls on the same images -- counts equal, tracking against them bit-identical."""
    from vo_single_camera_sos_amd.pipeline import batch_cfg
    gs, rig_kw = _rig()
    room, rng = synthetic.Room(seed=61), np.random.default_rng(62)
    three = np.stack([synthetic.render_omni(gs, room, R, t, 2.0, rng) for R, t in synthetic.trajectory(3, 61, max_t=40.0, max_deg=2.0)])
    model = DeviceImageModel(ctx, gs, (480, 640))
    if getattr(model, "unwrap_table", None) is None:
        model.unwrap_table = ctx.unwrap_prepare(model.omni_masks, model.map_x, model.map_y, (model.H, model.W))
    n, W, slots = 260, 260, 600
    cfg = batch_cfg(model, 40, 300, 320, 1024, 11, 0.01, 5.0, 31, None, 210, True, 0, 30, "GP3P", "GFT")
    rig = RigConfig(**rig_kw).as_struct()
    ws = torch.empty((ctx.sequence_workspace(cfg, W, slots),), dtype=torch.uint8, device=ctx.device)
    small = torch.from_numpy(three).to(ctx.device)
    omni = small[torch.arange(n, device=ctx.device) % 3].contiguous()           # frame i shows image i % 3
    table, free = _scattered(n, slots)
    fe = lambda frames, tab: ctx.sequence_front_end_slots(rig, cfg, W, slots, frames, tab, model.unwrap_table,  # noqa: E731
                                                          model.mask_bits, model.pattern, ws)
    fe(omni, table)
    ref = free[:3]                                                                # the three images again, a small call
    fe(small, ref)
    counts = ctx.sequence_frame_counts(cfg, W, slots, 0, slots, ws)
    assert min(counts[v] for v in ref) > 50
    assert [counts[table[i]] for i in range(n)] == [counts[ref[i % 3]] for i in range(n)]
    out = torch.zeros((40, 16), dtype=torch.float64, device=ctx.device)
    track = lambda r, c, sd: ctx.sequence_track_seeds(rig, cfg, W, slots, r, c, sd, ws, out)[:len(r)].cpu().numpy().copy()  # noqa: E731
    # image 0 -> image 1 from both sides of the 256-frame boundary, against the small call's slots
    pairs = [(0, 1), (255, 256), (258, 259), (3, 259)]
    got = track([table[a] for a, _ in pairs], [table[b] for _, b in pairs], [5] * 4)
    want = track([ref[0]], [ref[1]], [5])
    assert want[0, 14] == 0 and want[0, 12] > 30
    assert all(np.array_equal(g, want[0]) for g in got)
    # 20 promotions in one call
    src, dst = [table[3 * k] for k in range(20)], free[3:23]                     # image 0 every time, from 20 slots
    ctx.sequence_copy_slots(cfg, W, slots, src, dst, ws)
    counts = ctx.sequence_frame_counts(cfg, W, slots, 0, slots, ws)
    assert [counts[v] for v in dst] == [counts[v] for v in src] == [counts[ref[0]]] * 20
    seeds = [2 ** 34 + 3 * k for k in range(20)]                                  # (and 20 pairs with their seeds, copied)
    a = track(dst, [table[1]] * 20, seeds)
    b = track(src, [table[1]] * 20, seeds)
    assert np.array_equal(a, b) and (a[:, 14] == 0).all()
    assert not np.array_equal(a[0], a[1])                                          # (the seeds entered)
    # a copied list with a swapped pair would have gone wrong here: one source differs from the others
    src2, dst2 = [table[3 * k + (1 if k == 17 else 0)] for k in range(20)], free[23:43]
    ctx.sequence_copy_slots(cfg, W, slots, src2, dst2, ws)
    one = track([dst2[17], dst2[16]], [table[2]] * 2, [9, 9])
    two = track([ref[1], ref[0]], [ref[2]] * 2, [9, 9])
    assert np.array_equal(one, two) and not np.array_equal(one[0], one[1])


def test_tables_beyond_the_kernel_arguments_rgbd(ctx):
    """The same for the RGB-D family: 258 frames through sosvo_rgbd_sequence_front_end_slots, 18 copies in one call."""
    from vo_single_camera_sos_amd.pipeline import rgbd_batch_cfg
    cam = RGBDCamConfig(fx=554.256258, fy=554.256258, center_x=319.5, center_y=239.5, depth_is_Z=False, min_range=0.8, max_range=7.0)
    helper = RGBDMultiSequenceEngine(ctx, cam, lanes=1, window=1, num_of_features=1000)     # (its mask, pattern and camera struct)
    bgr3, depth3, _ = synthetic.make_rgbd_sequence(3, seed=41, max_t=40.0, max_deg=2.0, depth_is_Z=False)
    n, W, slots = 258, 258, 400
    cfg = rgbd_batch_cfg(cam, 32, (480, 640), 1000, None, None, 0, 0.01, 5.0, 31, None, 210, True, 0, 30, "EPNP", "GFT")
    ws = torch.empty((ctx.rgbd_sequence_workspace(cfg, W, slots),), dtype=torch.uint8, device=ctx.device)
    sb, sd_ = torch.from_numpy(bgr3).to(ctx.device), torch.from_numpy(np.ascontiguousarray(depth3, dtype=np.float32)).to(ctx.device)
    pick = torch.arange(n, device=ctx.device) % 3
    table, free = _scattered(n, slots)
    fe = lambda b, d, tab: ctx.rgbd_sequence_front_end_slots(helper.cam, cfg, W, slots, b, d, tab, helper.mask_bits,  # noqa: E731
                                                             helper.pattern, ws)
    fe(sb[pick].contiguous(), sd_[pick].contiguous(), table)
    ref = free[:3]
    fe(sb, sd_, ref)
    counts = ctx.rgbd_sequence_frame_counts(cfg, W, slots, 0, slots, ws)
    assert min(counts[v] for v in ref) > 100
    assert [counts[table[i]] for i in range(n)] == [counts[ref[i % 3]] for i in range(n)]
    out = torch.zeros((32, 16), dtype=torch.float64, device=ctx.device)
    track = lambda r, c, sd: ctx.rgbd_sequence_track_seeds(cfg, W, slots, r, c, sd, ws, out)[:len(r)].cpu().numpy().copy()  # noqa: E731
    got = track([table[0], table[255], table[255]], [table[1], table[256], table[1]], [5] * 3)
    want = track([ref[0]], [ref[1]], [5])
    assert want[0, 14] == 0 and all(np.array_equal(g, want[0]) for g in got)
    src, dst = [table[3 * k + (1 if k == 17 else 0)] for k in range(18)], free[3:21]
    ctx.rgbd_sequence_copy_slots(cfg, W, slots, src, dst, ws)
    counts = ctx.rgbd_sequence_frame_counts(cfg, W, slots, 0, slots, ws)
    assert [counts[v] for v in dst] == [counts[v] for v in src]
    one = track([dst[17], dst[16]], [table[2]] * 2, [9, 9])
    two = track([ref[1], ref[0]], [ref[2]] * 2, [9, 9])
    assert np.array_equal(one, two) and not np.array_equal(one[0], one[1])


def test_run_vo_many_refuses_a_sequence_of_another_frame_size(ctx, tmp_path):
    """Two in-memory RGB-D sources on one camera model, 640x480 and 320x240: whichever lane builds the engine, the other
    does not fit it and run_VO_many raises, after the fitting lane has finished."""
    from vo_single_camera_sos_amd.omnistereo.camera_models import RGBDCamModel
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO_many
    bgr, depth, _ = synthetic.make_rgbd_sequence(3, seed=41, max_t=40.0, max_deg=2.0, depth_is_Z=False)

    def source(b, d):
        def frames():
            for i in range(b.shape[0]):
                yield i, b[i], d[i]
        return frames
    half = np.ascontiguousarray(bgr[:, ::2, ::2]), np.ascontiguousarray(depth[:, ::2, ::2])
    cam = RGBDCamModel(fx=554.256258, fy=554.256258, center_x=319.5, center_y=239.5, scaling_factor=1. / 1000.0,
                       do_undistortion=False, depth_is_Z=False, focal_length_m=1. / 1000.0)
    many = [dict(results_path=str(tmp_path / "full"), _live_frames=source(bgr, depth)),
            dict(results_path=str(tmp_path / "half"), _live_frames=source(*half))]
    with pytest.raises(ValueError, match="does not fit the lanes' engine"):
        run_VO_many(cam, many, frame_window=2)
    assert sum(os.path.exists(os.path.join(q["results_path"], FILES[0])) for q in many) == 2     # both runs closed their files


# ---- 4 - 6. the whole path ----------------------------------------------------------------------------------------------
def _read(results):
    return scenes.read_results(results, FILES)


@pytest.fixture(scope="module")
def sos_sequences(tmp_path_factory):
    return scenes.write_sos_sequences(tmp_path_factory.mktemp("multi_sos"), SOS_SEEDS, SOS_FRAMES)


def _sos_main(seqs, window, *extra):
    import demo_vo_sos
    return demo_vo_sos.main_sos_vo(list(seqs) + ["--calibrated_gums_file", os.path.join(seqs[0], "gums-calibrated.json"),
                                                 "--frame_window", str(window)] + list(extra))


@pytest.mark.parametrize("window", [8, 1])
def test_demo_with_several_sequences_writes_each_sequences_solo_files(ctx, sos_sequences, window):
    solo = []
    for seq, n in zip(sos_sequences, SOS_FRAMES):
        out = _sos_main([seq], window)
        assert isinstance(out, dict) and out["tracked"] == n - 1, (seq, out["tracked"])      # every frame tracked
        solo.append(_read(os.path.join(seq, "results-omni")))
    outs = _sos_main(sos_sequences, window)
    assert isinstance(outs, list) and [o["tracked"] for o in outs] == [n - 1 for n in SOS_FRAMES]
    for seq, want, o in zip(sos_sequences, solo, outs):
        assert _read(os.path.join(seq, "results-omni")) == want, seq
        assert len(want[0].splitlines()) == len(o["poses"])
        sm = o["sequence_mode"]
        assert sm["lanes"] == 3 and sm["frame_window"] == window
        assert 0 < sm["front_end_launches"] < sum(-(-n // window) for n in SOS_FRAMES)     # shared launches
    if window == 8:      # two lanes for three sequences: a lane is reused
        outs2 = _sos_main(sos_sequences, window, "--lanes", "2")
        assert sorted(o["sequence_mode"]["lane"] for o in outs2) in ([0, 0, 1], [0, 1, 1])
        for seq, want in zip(sos_sequences, solo):
            assert _read(os.path.join(seq, "results-omni")) == want, seq


def test_the_batched_serial_call_is_taken(ctx, sos_sequences, tmp_path):
    """W = 1 with run_VO_live's keyframe thresholds (50 mm / 5 degrees): the synthetic steps are below them, so frame 1 of every
    lane stays un-promoted and frame 2 has to be tracked against keyframe 0, which no speculation covers at W = 1."""
    from vo_single_camera_sos_amd.omnistereo.gum import load_gums_json
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO, run_VO_many
    gums = os.path.join(sos_sequences[0], "gums-calibrated.json")
    want = []
    for k, (seq, n) in enumerate(zip(sos_sequences, SOS_FRAMES)):
        res = str(tmp_path / ("solo_%d" % k))
        out = run_VO(None, load_gums_json(gums), frame_window=1, _keyframe_thresholds=LIVE_THRESHOLDS, **_sos_kwargs(seq, n, res))
        assert out["tracked"] == n - 1 and out["sequence_mode"]["serial_tracking_calls"] > 0
        want.append((_read(res), out["sequence_mode"]["serial_tracking_calls"]))
    many = [_sos_kwargs(seq, n, str(tmp_path / ("many_%d" % k))) for k, (seq, n) in enumerate(zip(sos_sequences, SOS_FRAMES))]
    outs = run_VO_many(load_gums_json(gums), many, frame_window=1, _keyframe_thresholds=LIVE_THRESHOLDS)
    for q, (files, serial), o in zip(many, want, outs):
        assert _read(q["results_path"]) == files
        sm = o["sequence_mode"]
        assert sm["serial_tracking_calls"] == serial > 0
        assert sm["max_serial_pairs"] >= 2 and sm["serial_track_launches"] < sum(w[1] for w in want)


def test_rgbd_demo_with_two_sequences(ctx, tmp_path):
    import demo_vo_rgbd
    seqs = []
    for k, (seed, n) in enumerate(zip(RGBD_SEEDS, RGBD_FRAMES)):
        seq = str(tmp_path / ("rgbd_%d" % k))
        synthetic.write_rgbd_sequence(seq, n_frames=n, seed=seed, max_t=40.0, max_deg=2.0, depth_is_Z=False)
        seqs.append(seq)
    for window in (8, 1):
        solo = []
        for seq, n in zip(seqs, RGBD_FRAMES):
            out = demo_vo_rgbd.main_rgbd_vo([seq, "--is_synthetic", "true", "--frame_window", str(window)])
            assert out["tracked"] == n - 1
            solo.append(_read(os.path.join(seq, "results-rgbd")))
        outs = demo_vo_rgbd.main_rgbd_vo(seqs + ["--is_synthetic", "true", "--frame_window", str(window)])
        assert [o["tracked"] for o in outs] == [n - 1 for n in RGBD_FRAMES]
        for seq, want in zip(seqs, solo):
            assert _read(os.path.join(seq, "results-rgbd")) == want, (window, seq)
        assert outs[0]["sequence_mode"]["front_end_launches"] < sum(-(-n // window) for n in RGBD_FRAMES)


def test_a_lane_that_stops_early_and_a_lane_whose_reader_raises(ctx, sos_sequences, tmp_path, monkeypatch):
    from vo_single_camera_sos_amd.omnistereo import common_cv
    from vo_single_camera_sos_amd.omnistereo.common_cv import imwrite
    from vo_single_camera_sos_amd.omnistereo.gum import load_gums_json
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO, run_VO_many
    gs, _ = _rig()
    black = str(tmp_path / "seq_black")
    synthetic.write_sos_sequence(black, gs, n_frames=9, seed=5, max_t=40.0, max_deg=2.0)
    imwrite(os.path.join(black, "omni", "image-0005.png"), np.zeros((480, 640, 3), np.uint8))
    gums = os.path.join(black, "gums-calibrated.json")
    seqs, frames = [sos_sequences[0], black, sos_sequences[2]], [SOS_FRAMES[0], 9, SOS_FRAMES[2]]
    want = []
    for k, (seq, n) in enumerate(zip(seqs, frames)):
        res = str(tmp_path / ("solo_%d" % k))
        if seq == black:
            with pytest.warns(UserWarning):
                out = run_VO(None, load_gums_json(gums), frame_window=4, **_sos_kwargs(seq, n, res))
            assert [p[0] for p in out["poses"]] == [0, 1, 2, 3, 4]
        else:
            out = run_VO(None, load_gums_json(gums), frame_window=4, **_sos_kwargs(seq, n, res))
            assert out["tracked"] == n - 1
        want.append((_read(res), [p[1] for p in out["poses"]]))
    many = [_sos_kwargs(seq, n, str(tmp_path / ("many_%d" % k))) for k, (seq, n) in enumerate(zip(seqs, frames))]
    with pytest.warns(UserWarning):
        outs = run_VO_many(load_gums_json(gums), many, frame_window=4)
    assert [p[0] for p in outs[1]["poses"]] == [0, 1, 2, 3, 4]                 # the same frame ...
    for q, (files, poses), o in zip(many, want, outs):
        assert _read(q["results_path"]) == files                                  # ... and everybody's solo files
        assert all(np.array_equal(a[1], b) for a, b in zip(o["poses"], poses))
    # a reader that raises in lane 1 (frame 6 of the black sequence's twin, a good sequence): the others finish first
    name = os.path.join(sos_sequences[1], "omni", "image-0006.png")
    imread = common_cv.imread

    def failing_imread(filename):
        if os.path.realpath(filename) == os.path.realpath(name):
            raise OSError("simulated read error: %s" % filename)
        return imread(filename)
    monkeypatch.setattr(common_cv, "imread", failing_imread)
    seqs2, frames2 = list(sos_sequences), list(SOS_FRAMES)
    many2 = [_sos_kwargs(seq, n, str(tmp_path / ("fail_%d" % k))) for k, (seq, n) in enumerate(zip(seqs2, frames2))]
    with pytest.raises(OSError, match="image-0006.png"):
        run_VO_many(load_gums_json(gums), many2, frame_window=4)
    assert _read(many2[0]["results_path"]) == want[0][0] and _read(many2[2]["results_path"]) == want[2][0]
    lines = open(os.path.join(many2[1]["results_path"], FILES[0])).read().splitlines()
    assert [int(x.split()[0]) for x in lines] == list(range(6))                   # the frames before the failure


def test_run_vo_many_after_an_aborted_one_on_the_same_camera_model(ctx, sos_sequences, tmp_path, monkeypatch):
    from vo_single_camera_sos_amd.omnistereo import common_cv
    from vo_single_camera_sos_amd.omnistereo.gum import load_gums_json
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO, run_VO_many
    gums = os.path.join(sos_sequences[0], "gums-calibrated.json")
    model = load_gums_json(gums)
    name = os.path.realpath(os.path.join(sos_sequences[0], "omni", "image-0009.png"))
    imread = common_cv.imread

    def failing_imread(filename):
        if os.path.realpath(filename) == name:
            raise OSError("simulated read error: %s" % filename)
        return imread(filename)
    with monkeypatch.context() as mp:
        mp.setattr(common_cv, "imread", failing_imread)
        with pytest.raises(OSError, match="image-0009.png"):
            run_VO_many(model, [_sos_kwargs(seq, n, str(tmp_path / ("a_%d" % k)))
                                for k, (seq, n) in enumerate(zip(sos_sequences[:2], SOS_FRAMES[:2]))], frame_window=4)
    engines = list(model.__dict__["_multi_sequence_engines"].values())
    assert len(engines) == 1 and not engines[0]._live
    many = [_sos_kwargs(seq, n, str(tmp_path / ("b_%d" % k))) for k, (seq, n) in enumerate(zip(sos_sequences[1:], SOS_FRAMES[1:]))]
    outs = run_VO_many(model, many, frame_window=4)
    assert list(model.__dict__["_multi_sequence_engines"].values()) == engines      # the same engine served the second call
    for q, seq, n, o in zip(many, sos_sequences[1:], SOS_FRAMES[1:], outs):
        res = str(tmp_path / ("fresh_" + os.path.basename(seq)))
        fresh = run_VO(None, load_gums_json(gums), frame_window=4, **_sos_kwargs(seq, n, res))
        assert o["tracked"] == fresh["tracked"] == n - 1
        assert _read(q["results_path"]) == _read(res)
