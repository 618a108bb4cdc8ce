"""GPU: Lucas-Kanade tracking (SOSVO_FLAG_LK_F2F) in the one-call batches, sequence mode and run_VO.  Every record comparison
is bit for bit.  The chain rests on what is pinned elsewhere: the tracker against tests/reflk.py and the pair pipeline's LK
step (tests/test_gpu_lk.py).  Here:
  1. the one-call batch gives the pair pipeline's records, also split over the library's internal streams;
  2. the records do not depend on what the workspace held;
  3. the sequence engine gives the pair batch's records for windows 1, 2 and 5;
  4. a promoted keyframe takes its images along;
  5. the lanes of a multi-sequence engine give a solo engine's records;
  6. run_VO writes the same pose file whatever the frame window, and the demo's command line writes it too;
  7. the refusals of the device entries, and sosvo_set_lk_options keeping the previous settings;
  8. the one condition on accuracy test_pair_pipeline_tracks_with_lk has."""
import ctypes
import os

import numpy as np
import pytest

import matching_scenes as scenes
import synth
from matching_scenes import FRAME_CAP, ITERS, KW, LK_CHECKED, LK_WAVE, NFEAT, SEQ_KW
from vo_single_camera_sos_amd import _lib
from vo_single_camera_sos_amd.device import SosvoError
from vo_single_camera_sos_amd.frontend import ImageFrontEnd
from vo_single_camera_sos_amd.pipeline import FramePairBatch, FramePairPipeline, MultiSequenceEngine, RigConfig, SequenceEngine

pytestmark = pytest.mark.gpu

_scene = scenes.translating_scene      # 3 pairs and a 6-frame sequence, used whole


def _pair_record(ctx, s, a, b, seed, lk):
    """The pair batch's record of frames (a, b) of the sequence under the tracker's settings."""
    return scenes.pair_record(ctx, s, a, b, seed, f2f_tracker="lk", lk=lk, **SEQ_KW)


# ---- 1. the one-call batch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lk,subpix", [(LK_CHECKED, None), (LK_WAVE, None), (LK_CHECKED, 2)], ids=["half4_fb", "half10", "half4_fb_subpix2"])
def test_one_call_batch_equals_the_pair_pipeline(ctx, lk, subpix):
    s = _scene(ctx)
    omni = s["omni"][:4]
    fe = ImageFrontEnd(ctx, s["model"], 4, detection_method="GFT", num_of_features=NFEAT, keep_panoramas=False)
    pipe = FramePairPipeline(ctx, RigConfig(**s["rig_kw"]), 2, frame_cap=FRAME_CAP, max_iter=ITERS, seed=5, front_end=fe, subpix=subpix,
                             f2f_tracker="lk", lk=lk)
    fe.load_frames(omni)
    pipe.step()
    want = pipe.results().cpu().numpy()
    got = scenes.batch_records(ctx, s, omni, **KW, kp_cap=fe.kp_cap, subpix=subpix, f2f_tracker="lk", lk=lk)
    assert (want[:, 14] == 0).all() and (want[:, 13] > 50).all(), want[:, 12:16]
    assert np.array_equal(got, want), np.argwhere(got != want)[:6]
    matched = scenes.batch_records(ctx, s, omni, **KW, kp_cap=fe.kp_cap, subpix=subpix)
    assert not np.array_equal(got, matched)                      # the switch does something


def test_streams_batch_gives_the_single_calls_records(ctx):
    """3 pairs over 2 internal streams with settings that are not the context's defaults: they reach the internal contexts."""
    s = _scene(ctx)
    one = scenes.batch_records(ctx, s, s["omni"], **KW, f2f_tracker="lk", lk=LK_CHECKED)
    two = scenes.batch_records(ctx, s, s["omni"], **KW, f2f_tracker="lk", lk=LK_CHECKED, n_streams=2)
    assert np.array_equal(one, two), np.argwhere(one != two)[:6]
    assert not np.array_equal(one, scenes.batch_records(ctx, s, s["omni"], **KW, f2f_tracker="lk", lk=dict(LK_CHECKED, half=5)))


# ---- 2. the workspace's contents ---------------------------------------------------------------------------------------------
def test_records_do_not_depend_on_the_workspaces_contents(ctx):
    """Rows outside the gray range and levels that are not built keep what the workspace held: nothing may read them."""
    s = _scene(ctx)
    for lk in (LK_CHECKED, LK_WAVE):
        a = scenes.batch_records(ctx, s, s["omni"][:4], **KW, fill=0x00, f2f_tracker="lk", lk=lk)
        b = scenes.batch_records(ctx, s, s["omni"][:4], **KW, fill=0xFF, f2f_tracker="lk", lk=lk)
        assert np.array_equal(a, b), np.argwhere(a != b)[:6]
    for fill in (0x00, 0xFF):                                    # ... and the sequence store: slots not written, the other half
        eng = SequenceEngine(ctx, s["model"], RigConfig(**s["rig_kw"]), window=2, f2f_tracker="lk", lk=LK_CHECKED, **SEQ_KW)
        eng.workspace.fill_(fill)
        got = scenes.hop_records(eng, s["seq"][:4], 2)
        assert np.array_equal(got, np.stack([_pair_record(ctx, s, t - 1, t, t - 1, LK_CHECKED) for t in (1, 2, 3)])), fill


# ---- 3. the sequence engine ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lk", [LK_CHECKED, LK_WAVE], ids=["half4_fb", "half10"])
def test_sequence_engine_equals_the_pair_batch_for_every_window(ctx, lk):
    s = _scene(ctx)
    n = 5
    want = np.stack([_pair_record(ctx, s, t - 1, t, t - 1, lk) for t in range(1, n)])
    assert (want[:, 14] == 0).all() and (want[:, 12] > 50).all(), want[:, 12:16]
    for window in (1, 2, 5):
        eng = SequenceEngine(ctx, s["model"], RigConfig(**s["rig_kw"]), window=window, f2f_tracker="lk", lk=lk, **SEQ_KW)
        got = scenes.hop_records(eng, s["seq"][:n], window)
        assert np.array_equal(got, want), (window, np.argwhere(got != want)[:6])


# ---- 4. promotion ----------------------------------------------------------------------------------------------------------------
def test_a_promoted_keyframe_takes_its_images_along(ctx):
    s = _scene(ctx)
    eng = SequenceEngine(ctx, s["model"], RigConfig(**s["rig_kw"]), window=2, f2f_tracker="lk", lk=LK_CHECKED, **SEQ_KW)
    infos = eng.push_window(list(s["seq"][0:2]))
    eng.promote(infos[1]["slot"])                                 # frame 1, in half 0
    slot3 = eng.push_window(list(s["seq"][2:4]))[1]["slot"]       # half 1
    slot5 = eng.push_window(list(s["seq"][4:6]))[1]["slot"]       # refills half 0: frame 1's record and images move first
    assert slot5 == infos[1]["slot"]
    got = eng.track(eng.key_slot, slot3, seed=2)
    assert np.array_equal(got, _pair_record(ctx, s, 1, 3, 2, LK_CHECKED)), (got, _pair_record(ctx, s, 1, 3, 2, LK_CHECKED))
    assert not np.array_equal(got, _pair_record(ctx, s, 2, 3, 2, LK_CHECKED))
    assert not np.array_equal(got[:12], _pair_record(ctx, s, 5, 3, 2, LK_CHECKED)[:12])   # (what the slot frame 1 left now holds)
    # the list form moves images too: key slot -> the slot frame 4 sits in would be refused (read and written); copy frame 3's
    # slot over the key slot and track frame 5 against it
    eng.fam.copy_slots([slot3], [eng.key_slot])
    assert np.array_equal(eng.track(eng.key_slot, slot5, seed=4), _pair_record(ctx, s, 3, 5, 4, LK_CHECKED))


# ---- 5. several sequences --------------------------------------------------------------------------------------------------------
def test_multi_sequence_lanes_equal_solo_engines(ctx):
    """Two 4-frame sequences through the lanes of one engine (one host thread each, as run_VO_many drives them) against each
    through a SequenceEngine alone: counts, seeds, both speculative records and the serial records."""
    s = _scene(ctx)
    seqs = [s["seq"][0:4], s["seq"][2:6]]
    new = lambda cls, **kw: cls(ctx, s["model"], RigConfig(**s["rig_kw"]), window=2, f2f_tracker="lk", lk=LK_CHECKED, **kw, **SEQ_KW)  # noqa: E731
    got = scenes.drive_lanes(new(MultiSequenceEngine, lanes=2), seqs, 2)
    for k in range(2):
        want = scenes.drive(new(SequenceEngine), seqs[k], 2)
        assert len(got[k]) == len(want) == 4
        scenes.assert_same_drive(got[k], want)
        assert want[3][4] is not None and want[3][4][14] == 0


# ---- 6. run_VO -------------------------------------------------------------------------------------------------------------------
def test_run_vo_pose_file_does_not_depend_on_the_frame_window(ctx, tmp_path):
    """A 24-frame sequence through run_VO with the tracker: byte-identical pose and keyframe files for frame windows 32, 5 and
    1; the per-frame mirror path (frame_window 0) agrees to the standard test_gpu_sequence.py applies to it (rtol 1e-6, atol
    1e-9 on every pose); the matcher's run writes another file; the demo's command line writes the tracker's."""
    import demo_vo_sos
    from vo_single_camera_sos_amd.omnistereo.gum import load_gums_json
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO
    n = 24
    seq = scenes.write_sos_sequences(tmp_path, seeds=(77,), frames=n)[0]
    gums = os.path.join(seq, "gums-calibrated.json")
    cam = load_gums_json(gums)
    lk = dict(half=4, max_iter=10, fb_max=0.5)
    texts, outs = scenes.run_vo_windows(cam, seq, n, tmp_path, (32, 5, 1, 0), f2f_tracker="lk", lk=lk)
    assert texts[32] == texts[5] == texts[1] and len(texts[32][0].splitlines()) == n
    results = str(tmp_path / "results_match")
    match = run_VO(None, cam, frame_window=32, f2f_tracker="match", **scenes.sos_kwargs(seq, n, results))
    assert match["tracked"] == n - 1, match["message"]
    assert texts[32][0] != scenes.read_results(results)[0]
    assert "sequence_mode" not in outs[0] and len(outs[0]["poses"]) == n
    for (i, Ta), (j, Tb) in zip(outs[0]["poses"], outs[32]["poses"]):
        assert i == j and np.allclose(Ta, Tb, rtol=1e-6, atol=1e-9), (i, np.abs(Ta - Tb).max())
    out = demo_vo_sos.main_sos_vo([seq, "--calibrated_gums_file", gums, "--frame_window", "5", "--f2f_tracker", "lk", "--lk_half", "4",
                                   "--lk_max_iter", "10", "--lk_fb_max", "0.5"])
    assert out["tracked"] == n - 1
    assert scenes.read_results(os.path.join(seq, "results-omni")) == texts[32]


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_the_device_entries_refuse_and_keep_the_previous_settings(ctx):
    s = _scene(ctx)
    batch = FramePairBatch(ctx, s["model"], RigConfig(**s["rig_kw"]), 2, seed=5, f2f_tracker="lk", lk=LK_CHECKED, **KW)
    batch.load_frames(s["omni"][:4])
    want = batch.step().cpu().numpy().copy()
    m = s["model"]
    for bit in (_lib.FLAG_CROSS_CHECK_F2F, _lib.FLAG_GATED_F2F, _lib.FLAG_RATIO_F2F | (48 << _lib.RATIO_64THS_SHIFT)):
        batch.cfg.ransac_flags |= bit
        with pytest.raises(SosvoError, match="SOSVO_ERR_ARG"):
            ctx.frame_pair_batch(batch.rig, batch.cfg, batch.omni, m.unwrap_table, m.mask_bits, m.pattern, batch.workspace, results=batch.out)
        with pytest.raises(SosvoError, match="SOSVO_ERR_ARG"):
            ctx.sequence_track(batch.rig, batch.cfg, 4, 4, [0], [1], 0, batch.workspace, batch.out)
        batch.cfg.ransac_flags &= ~bit
    from cfg_fakes import rgbd_cfg
    lib, h = _lib.load(), ctx._h
    c = rgbd_cfg(_lib.FLAG_LK_F2F)
    assert lib.sosvo_rgbd_pair_batch_workspace(ctypes.byref(c)) == 0
    one = ctypes.c_void_p(batch.workspace.data_ptr())
    assert lib.sosvo_rgbd_pair_batch(h, one, ctypes.byref(c), one, one, one, one, one, batch.workspace.numel(), one) == -1
    assert lib.sosvo_rgbd_sequence_track(h, ctypes.byref(c), 4, 9, one, one, 1, 0, one, batch.workspace.numel(), one) == -1
    good = _lib.LKOptions.of(LK_CHECKED)
    for bad in (dict(half=1), dict(half=11), dict(levels=0), dict(levels=5), dict(max_iter=0), dict(max_iter=31), dict(eps=-1.0),
                dict(eps=float("nan")), dict(eps=float("inf")), dict(min_eig=-1e-9), dict(min_eig=float("nan")),
                dict(min_eig=float("inf"))):
        st = _lib.LkOptionsStruct.of(good)
        for k, v in bad.items():
            setattr(st, k, v)
        assert lib.sosvo_set_lk_options(h, ctypes.byref(st)) == -1, bad
        got = ctx.frame_pair_batch(batch.rig, batch.cfg, batch.omni, m.unwrap_table, m.mask_bits, m.pattern, batch.workspace,
                                   results=batch.out).cpu().numpy()
        assert np.array_equal(got, want), bad
    assert lib.sosvo_set_lk_options(h, None) == -1                   # (a null pointer is an argument error, as everywhere)
    ctx.set_lk_options(None)                                       # the defaults, which are not these settings
    assert ctx.lk_options == _lib.LKOptions()
    got = ctx.frame_pair_batch(batch.rig, batch.cfg, batch.omni, m.unwrap_table, m.mask_bits, m.pattern, batch.workspace,
                               results=batch.out).cpu().numpy()
    assert not np.array_equal(got, want)
    assert np.array_equal(batch.step().cpu().numpy(), want)         # (the engine puts its own back)


# ---- 8. accuracy ---------------------------------------------------------------------------------------------------------------------
def test_one_call_batch_tracks_with_lk(ctx):
    """The condition of test_pair_pipeline_tracks_with_lk on its two pairs (seed 99, GFT 330 features, one-mirror P3P with 500
    fixed iterations): status 0 and a rotation error below the reference's own 5-degree inlier threshold.  The figures are
    printed beside the matcher's, not asserted."""
    s = _scene(ctx)
    for name, kw in (("match", {}), ("lk half 4 + fb", dict(f2f_tracker="lk", lk=dict(half=4, max_iter=10, fb_max=0.5))),
                     ("lk half 10 + fb", dict(f2f_tracker="lk", lk=dict(half=10, max_iter=10, fb_max=0.5)))):
        rec = scenes.batch_records(ctx, s, s["omni"][:4], **dict(kw, num_of_features=330, frame_cap=2048, max_iter=500))
        rot = [np.degrees(synth.pose_error(rec[i, :12].reshape(3, 4), R, t)[0]) for i, (R, t) in enumerate(s["poses"][:2])]
        print("%-16s inliers / correspondences %d / %d = %.3f, rotation error %s deg" % (
            name, rec[:, 12].sum(), rec[:, 13].sum(), rec[:, 12].sum() / max(rec[:, 13].sum(), 1), ["%.3f" % r for r in rot]))
        assert (rec[:, 14] == 0).all(), name
        assert max(rot) < 5.0, name
