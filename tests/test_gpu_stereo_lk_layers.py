"""GPU: the sub-pixel static stereo (sosvo_refine_stereo_lk, SOSVO_FLAG_LK_STEREO) through the layers, on the two small
rendered pairs of tests/test_gpu_lk.py (seed 99, GFT 330 per mask, 500 iterations).  Every record comparison is bit for bit.
The chain rests on the stage against tests/refstereolk.py (tests/test_gpu_stereo_lk.py).  Here:
  1. FramePairPipeline(stereo_refine="lk"): the refined bottom keypoints are the reference's, the frame records are those of the
     reference flow's stereo assembly (tests/refflow.py on the oracle, unchanged) fed the refined kp_bot; off: as before;
  2. the one-call batch, also split over the library's internal streams, and the stream-split pipeline give the pair pipeline's
     records -- alone, with subpix, with the ratio rule, with f2f_tracker="lk", gated with the cross-check, and with the ORB
     and FAST detectors;
  3. the sequence engine gives the pair batch's records for windows 1, 2 and 5; the lanes of a multi-sequence engine a solo
     engine's;
  4. run_VO writes the same pose file whatever the frame window, and so do the per-frame mirror path and the lanes of
     run_VO_many; the demo's flags;
  5. the pose error on the two pairs beside the option off (figures printed, tracking must succeed)."""
import os

import numpy as np
import pytest
import torch

import matching_scenes as scenes
import refflow
import refstereolk as ref
import synth
from vo_single_camera_sos_amd.frontend import ImageFrontEnd
from vo_single_camera_sos_amd.pipeline import (FramePairBatch, FramePairPipeline, MultiSequenceEngine, OverlappedFramePairs, RigConfig,
                                               SequenceEngine)

pytestmark = pytest.mark.gpu

NFEAT, FRAME_CAP, ITERS = 330, 2048, 500
KW = dict(num_of_features=NFEAT, frame_cap=FRAME_CAP, max_iter=ITERS)
SEQ_KW = dict(num_of_features=NFEAT, frame_cap=FRAME_CAP, max_iter=210, adaptive=True, ransac_solver="GP3P")
SLK = dict(half=3, max_shift=2.0)                    # settings that are not the context's defaults


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _scene(ctx):
    """The translating scene's first 2 pairs and first 5 frames."""
    s = scenes.translating_scene(ctx)
    return dict(s, omni=s["omni"][:4], poses=s["poses"][:2], seq=s["seq"][:5])


def _pipe(ctx, s, **kw):
    """-> (front end, pair pipeline) over the two pairs, stepped once."""
    fe = ImageFrontEnd(ctx, s["model"], 4, detection_method="GFT", num_of_features=NFEAT, keep_panoramas=False)
    pipe = FramePairPipeline(ctx, RigConfig(**s["rig_kw"]), 2, frame_cap=FRAME_CAP, max_iter=ITERS, seed=5, front_end=fe, **kw)
    fe.load_frames(s["omni"])
    return fe, pipe


def _records(ctx, s, frames, **kw):
    """The one-call batch's records under this module's settings."""
    return scenes.batch_records(ctx, s, frames, **dict(KW, **kw))


# ---- 1. the pair pipeline ----------------------------------------------------------------------------------------------------
def test_pair_pipeline_refines_between_sort_and_assemble(ctx):
    s = _scene(ctx)
    fe, pipe = _pipe(ctx, s, stereo_refine="lk")
    fe.run()
    F, NM, cap = 4, fe.model.nmask, fe.kp_cap
    before = fe.kp.cpu().numpy().copy()
    desc_before = fe.desc.cpu().numpy().copy()
    pipe.stereo()
    ctx.synchronize()
    kp, n, desc = fe.kp.cpu().numpy(), fe.n.cpu().numpy(), fe.desc.cpu().numpy()
    h = F * NM
    st = pipe.s_lk_status.cpu().numpy()
    assert np.array_equal(before, np.rint(before))                                         # GFT: the detector's integer grid
    assert np.array_equal(_u32(kp[:h]), _u32(before[:h])) and np.array_equal(desc, desc_before)   # the top view, the descriptors
    moved = (_u32(kp[h:]) != _u32(before[h:])).any(axis=2)
    assert moved.sum() > 200 and not (moved & (st == 0)).any()
    assert np.abs(kp[h:] - before[h:]).max() <= 4.0
    print("accepted %d of %d bottom keypoints, moved %d" % (st.sum(), n[h:].sum(), moved.sum()))
    # the stage's rule on frame 0, masks 0 and 1 (the reference is slow): the device's positions are the reference's
    gray, keys = fe.gray.cpu().numpy(), pipe.s_keys.cpu().numpy().reshape(h, cap)
    rr = None if fe.keep_panoramas else fe.gray_rows.cpu().numpy()
    n_bot = n[h:h + NM].copy()
    n_bot[2:] = 0
    want, want_st = ref.refine(gray[[0, F]], NM, before[:NM], n[:NM], before[h:h + NM], n_bot, keys[:NM], row_range=rr,
                               min_disp=s["rig_kw"].get("stereo_min_disp", 1.0), max_hdiff=s["rig_kw"].get("stereo_max_hdiff", 2.5))
    for p in range(2):
        assert n_bot[p] > 20
        assert np.array_equal(_u32(kp[h + p, :n_bot[p]]), _u32(want[p, :n_bot[p]])), p
        assert np.array_equal(st[p, :n_bot[p]], want_st[p, :n_bot[p]]), p
    # the frame records: the reference flow's stereo assembly, unchanged, fed the refined kp_bot
    rp = refflow.RigParams(**s["rig_kw"])
    got = {k: v.cpu().numpy() for k, v in pipe.frames.items()}
    for f in range(F):
        tops, bots = [f * NM + m for m in range(NM)], [h + f * NM + m for m in range(NM)]
        w = refflow.stereo_frame(rp, [kp[p, :n[p]] for p in tops], [kp[p, :n[p]] for p in bots], [desc[p, :n[p]] for p in tops],
                                 [desc[p, :n[p]] for p in bots])
        M = len(w["X"])
        assert got["M"][f] == M and M > 300, (f, got["M"][f], M)
        for key in ("m_top", "m_bot", "d_top", "d_bot", "X", "b_top", "b_bot"):
            assert np.array_equal(got[key][f, :M], w[key]), (f, key)
        assert (got["m_bot"][f, :M] != np.rint(got["m_bot"][f, :M])).any()
    # off: as before -- the keypoints stay on the grid, the records are those of the pipeline without the argument
    fe0, off = _pipe(ctx, s)
    off.step()
    fe1, none = _pipe(ctx, s, stereo_refine=None)
    none.step()
    ctx.synchronize()
    assert np.array_equal(off.results().cpu().numpy(), none.results().cpu().numpy())
    assert np.array_equal(fe0.kp.cpu().numpy(), before) and not hasattr(off, "s_lk_status")
    assert np.array_equal(_records(ctx, s, s["omni"], kp_cap=fe.kp_cap), off.results().cpu().numpy())


# ---- 2. the one-call batch -----------------------------------------------------------------------------------------------------
COMBOS = [dict(), dict(stereo_lk=SLK), dict(subpix=3), dict(ratio_stereo=True, ratio_f2f=True, ratio=0.75),
          dict(f2f_tracker="lk", lk=dict(half=4, levels=3, max_iter=10, fb_max=0.5)), dict(gated_stereo=True, cross_check_stereo=True)]


@pytest.mark.parametrize("more", COMBOS, ids=["alone", "half3_shift2", "subpix3", "ratio", "f2f_lk", "gated_cross"])
def test_one_call_batch_equals_the_pair_pipeline(ctx, more):
    s = _scene(ctx)
    fe, pipe = _pipe(ctx, s, stereo_refine="lk", **more)
    pipe.step()
    want = pipe.results().cpu().numpy()
    assert (want[:, 14] == 0).all() and (want[:, 13] > 50).all(), want[:, 12:16]
    got = _records(ctx, s, s["omni"], kp_cap=fe.kp_cap, stereo_refine="lk", fill=0xA5, **more)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.argwhere(got != want)[:6]
    off = _records(ctx, s, s["omni"], kp_cap=fe.kp_cap, **{k: v for k, v in more.items() if k != "stereo_lk"})
    assert not np.array_equal(got, off)                              # the switch does something
    if not more or "stereo_lk" in more:                              # the streams form and the stream-split pipeline
        two = _records(ctx, s, s["omni"], kp_cap=fe.kp_cap, stereo_refine="lk", n_streams=2, **more)
        assert np.array_equal(two.view(np.uint64), want.view(np.uint64)), np.argwhere(two != want)[:6]
    if "stereo_lk" in more:
        over = OverlappedFramePairs(ctx.device.index, s["gs"], (480, 640), RigConfig(**s["rig_kw"]), 2, n_streams=2, num_of_features=NFEAT,
                                    kp_cap=fe.kp_cap, frame_cap=FRAME_CAP, max_iter=ITERS, seed=5, stereo_refine="lk", **more)
        over.load_frames(s["omni"])
        over.step()
        res = over.results().clone()
        torch.cuda.synchronize()
        over.close()
        assert np.array_equal(res.cpu().numpy().view(np.uint64), want.view(np.uint64))
        assert not np.array_equal(got, _records(ctx, s, s["omni"], kp_cap=fe.kp_cap, stereo_refine="lk"))   # the settings arrive


@pytest.mark.parametrize("method", ["ORB", "FAST"])
def test_other_detectors(ctx, method):
    """ORB (the stage acts on kp_xy; kp4 keeps the detector's positions) and FAST (every gray row: no row range)."""
    s = _scene(ctx)
    fe = ImageFrontEnd(ctx, s["model"], 4, detection_method=method, num_of_features=250, keep_panoramas=False)
    pipe = FramePairPipeline(ctx, RigConfig(**s["rig_kw"]), 2, frame_cap=1024, max_iter=300, seed=11, front_end=fe, stereo_refine="lk")
    fe.load_frames(s["omni"])
    fe.run()
    before = fe.kp.cpu().numpy().copy()
    kp4 = fe.kp4.cpu().numpy().copy() if method == "ORB" else None
    pipe.stereo()
    pipe.track()
    want = pipe.results().cpu().numpy()
    h = 4 * fe.model.nmask
    after = fe.kp.cpu().numpy()
    assert (want[:, 14] == 0).all() and (want[:, 13] > 0).all(), want[:, 12:]
    assert np.array_equal(_u32(after[:h]), _u32(before[:h])) and (_u32(after[h:]) != _u32(before[h:])).any()
    if method == "ORB":
        assert np.array_equal(_u32(fe.kp4.cpu().numpy()), _u32(kp4))
    kw = dict(num_of_features=250, kp_cap=fe.kp_cap, frame_cap=1024, max_iter=300, seed=11, detection_method=method)
    b = FramePairBatch(ctx, s["model"], RigConfig(**s["rig_kw"]), 2, stereo_refine="lk", **kw)
    b.load_frames(s["omni"])
    got = b.step().cpu().numpy().copy()
    ctx.synchronize()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.argwhere(got != want)[:6]
    off = FramePairBatch(ctx, s["model"], RigConfig(**s["rig_kw"]), 2, **kw)
    off.load_frames(s["omni"])
    assert not np.array_equal(off.step().cpu().numpy(), got)


# ---- 3. the sequence engines ---------------------------------------------------------------------------------------------------
def _pair_record(ctx, s, a, b, seed, **kw):
    return scenes.pair_record(ctx, s, a, b, seed, **dict(SEQ_KW, **kw))


@pytest.mark.parametrize("more", [dict(stereo_refine="lk"), dict(stereo_refine="lk", stereo_lk=SLK, f2f_tracker="lk", lk=dict(half=4, max_iter=10))],
                         ids=["alone", "half3_with_f2f_lk"])
def test_sequence_engine_equals_the_pair_batch_for_every_window(ctx, more):
    s = _scene(ctx)
    n = 5
    want = np.stack([_pair_record(ctx, s, t - 1, t, t - 1, **more) for t in range(1, n)])
    assert (want[:, 14] == 0).all() and (want[:, 12] > 50).all(), want[:, 12:16]
    assert not np.array_equal(want[0], _pair_record(ctx, s, 0, 1, 0))
    for window in (1, 2, 5):
        eng = SequenceEngine(ctx, s["model"], RigConfig(**s["rig_kw"]), window=window, **more, **SEQ_KW)
        eng.workspace.fill_(0x5A)
        got = scenes.hop_records(eng, s["seq"][:n], window)
        assert np.array_equal(got, want), (window, np.argwhere(got != want)[:6])


def test_multi_sequence_lanes_equal_solo_engines(ctx):
    s = _scene(ctx)
    seqs = [s["seq"][0:4], s["seq"][1:5]]
    new = lambda cls, **kw: cls(ctx, s["model"], RigConfig(**s["rig_kw"]), window=2, stereo_refine="lk", stereo_lk=SLK, **kw, **SEQ_KW)  # noqa: E731
    got = scenes.drive_lanes(new(MultiSequenceEngine, lanes=2), seqs, 2)
    for k in range(2):
        want = scenes.drive(new(SequenceEngine), seqs[k], 2)
        assert len(got[k]) == len(want) == 4
        scenes.assert_same_drive(got[k], want)
        assert want[3][4] is not None and want[3][4][14] == 0


# ---- 4. run_VO -------------------------------------------------------------------------------------------------------------------
def test_run_vo_pose_file_does_not_depend_on_the_frame_window(ctx, tmp_path):
    """A 10-frame sequence through run_VO with the option: byte-identical pose and keyframe files for frame windows 32, 5 and 1;
    so does the per-frame mirror path (frame_window 0); the run without the option writes another file; two lanes of one
    engine (run_VO_many) write their solo runs' files; the demo's command line writes the option's."""
    import demo_vo_sos
    from vo_single_camera_sos_amd.omnistereo.gum import load_gums_json
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO, run_VO_many
    n = 10
    seq, seq_b = scenes.write_sos_sequences(tmp_path, seeds=(77, 61), frames=n)
    gums = os.path.join(seq, "gums-calibrated.json")
    cam = load_gums_json(gums)
    texts, outs = scenes.run_vo_windows(cam, seq, n, tmp_path, (32, 5, 1, 0), stereo_refine="lk", stereo_lk=SLK)
    assert texts[32] == texts[5] == texts[1] and len(texts[32][0].splitlines()) == n
    results = str(tmp_path / "results_off")
    off = run_VO(None, cam, frame_window=32, **scenes.sos_kwargs(seq, n, results))
    assert off["tracked"] == n - 1, off["message"]
    assert texts[32][0] != scenes.read_results(results)[0]
    assert "sequence_mode" not in outs[0] and len(outs[0]["poses"]) == n
    assert texts[0] == texts[32]                                     # the per-frame mirror path writes the same bytes
    # two lanes of one engine (run_VO_many): every sequence gets the files of its solo run
    solo_b = str(tmp_path / "results_solo_b")
    assert run_VO(None, load_gums_json(gums), frame_window=5, stereo_refine="lk", stereo_lk=SLK, **scenes.sos_kwargs(seq_b, n, solo_b))["tracked"] == n - 1
    many = [scenes.sos_kwargs(q, n, str(tmp_path / ("many_%d" % k))) for k, q in enumerate((seq, seq_b))]
    outs = run_VO_many(load_gums_json(gums), many, frame_window=5, lanes=2, stereo_refine="lk", stereo_lk=SLK)
    assert [o["tracked"] for o in outs] == [n - 1, n - 1]
    assert scenes.read_results(many[0]["results_path"]) == texts[32] and scenes.read_results(many[1]["results_path"]) == scenes.read_results(solo_b)
    assert scenes.read_results(solo_b) != texts[32]
    out = demo_vo_sos.main_sos_vo([seq, "--calibrated_gums_file", gums, "--frame_window", "5", "--stereo_refine", "lk", "--stereo_lk_half", "3",
                                   "--stereo_lk_max_shift", "2.0"])
    assert out["tracked"] == n - 1
    assert scenes.read_results(os.path.join(seq, "results-omni")) == texts[32]


# ---- 5. accuracy (reported) --------------------------------------------------------------------------------------------------------
def test_pose_error_with_and_without_the_option(ctx):
    """The two pairs with the option off and at half 2, 4 and 10: status 0 and a rotation error below the reference's own
    5-degree inlier threshold; the figures are printed, not asserted."""
    s = _scene(ctx)
    for name, kw in (("off", {}), ("half 2", dict(stereo_refine="lk", stereo_lk=dict(half=2))), ("half 4", dict(stereo_refine="lk")),
                     ("half 10", dict(stereo_refine="lk", stereo_lk=dict(half=10)))):
        rec = _records(ctx, s, s["omni"], **kw)
        err = [synth.pose_error(rec[i, :12].reshape(3, 4), R, t) for i, (R, t) in enumerate(s["poses"])]
        print("%-8s inliers / correspondences %d / %d = %.3f, rotation error %s deg, translation error %s mm" % (
            name, rec[:, 12].sum(), rec[:, 13].sum(), rec[:, 12].sum() / max(rec[:, 13].sum(), 1),
            ["%.3f" % np.degrees(e[0]) for e in err], ["%.1f" % np.linalg.norm(rec[i, 3:12:4] - t) for i, (R, t) in enumerate(s["poses"])]))
        assert (rec[:, 14] == 0).all(), name
        assert max(np.degrees(e[0]) for e in err) < 5.0, name
