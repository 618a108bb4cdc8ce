"""GPU: the seam-free front end in the layers (SOSVO_FLAG_SEAM_FREE, cyclic_columns="seam_free"), every
record bit for bit, with the matcher (plain and gated_f2f), with f2f_tracker="lk" and with stereo_refine="lk": the one-call
batch equals the pair pipeline, also over two internal streams; records do not depend on the workspace's contents; the sequence
engine equals the pair batch for windows 1, 2 and 5 on the sequence that turns 7 degrees a frame (with the tracker this is the
store's padded level-0 fill under its row range against the pair batch's); multi-sequence lanes equal solo engines; run_VO
writes the same pose file whatever the window, the mirror path agrees to 1e-6 and the demo's command line writes the same file.
And what the option is for: a seam-free frame's stereo points are those of the CPU flow on the padded model
(oracle.flow.detect_view, refseam.unpad, refflow.stereo_frame), some of them inside the 31-column bands where the plain front
end has none.  The settings are those of tests/test_gpu_lk_layers.py (matching_scenes)."""
import os

import numpy as np
import pytest

import matching_scenes as scenes
import refflow
import refseam
from matching_scenes import FRAME_CAP, ITERS, KW, LK_CHECKED, NFEAT, SEQ_KW
from vo_single_camera_sos_amd import orb_pattern
from vo_single_camera_sos_amd.frontend import ImageFrontEnd
from vo_single_camera_sos_amd.pipeline import FramePairPipeline, MultiSequenceEngine, RigConfig, SequenceEngine

pytestmark = pytest.mark.gpu

SF = dict(cyclic_columns="seam_free")
SETTINGS = {"match": {}, "gated": dict(gated_f2f=True), "lk4_fb": dict(f2f_tracker="lk", lk=LK_CHECKED),
            "stereo_lk": dict(stereo_refine="lk"), "lk4_fb_stereo_lk_subpix": dict(f2f_tracker="lk", lk=LK_CHECKED, stereo_refine="lk", subpix=3)}


@pytest.fixture(scope="module")
def scene(ctx):
    """The turning scene (tests/test_gpu_cyclic_layers.py uses it too) with its -/+ 11-degree pairs as `omni`."""
    s = scenes.turning_scene(ctx)
    return dict(s, omni=s["yaw_omni"][11.0])


def _pipeline(ctx, s, omni, seam_free=True, **kw):
    model = s["model"].seam_free_form(ctx) if seam_free else s["model"]
    fe = ImageFrontEnd(ctx, model, len(omni), detection_method="GFT", num_of_features=NFEAT, keep_panoramas=False)
    pipe = FramePairPipeline(ctx, RigConfig(**s["rig_kw"]), len(omni) // 2, frame_cap=FRAME_CAP, max_iter=ITERS, seed=5, front_end=fe,
                             **kw, **(SF if seam_free else {}))
    fe.load_frames(omni)
    pipe.step()
    ctx.synchronize()
    return fe, pipe


@pytest.mark.parametrize("name", list(SETTINGS))
def test_one_call_batch_equals_the_pair_pipeline_also_over_two_streams(ctx, scene, name):
    kw, omni = SETTINGS[name], scene["omni"]
    fe, pipe = _pipeline(ctx, scene, omni, **kw)
    want = pipe.results().cpu().numpy()
    got = scenes.batch_records(ctx, scene, omni, kp_cap=fe.kp_cap, **KW, **kw, **SF)
    assert (want[:, 14] == 0).all() and (want[:, 13] > 50).all(), want[:, 12:16]
    assert np.array_equal(got, want), np.argwhere(got != want)[:6]
    two = scenes.batch_records(ctx, scene, omni, kp_cap=fe.kp_cap, n_streams=2, **KW, **kw, **SF)
    assert np.array_equal(two, want), np.argwhere(two != want)[:6]
    plain = scenes.batch_records(ctx, scene, omni, kp_cap=fe.kp_cap, cyclic_columns=True, **KW, **kw)
    assert not np.array_equal(got, plain)                          # the switch does something: there are points in the bands


@pytest.mark.parametrize("name", ["match", "lk4_fb", "stereo_lk"])
def test_records_do_not_depend_on_the_workspaces_contents(ctx, scene, name):
    kw = SETTINGS[name]
    a = scenes.batch_records(ctx, scene, scene["omni"], fill=0x00, **KW, **kw, **SF)
    b = scenes.batch_records(ctx, scene, scene["omni"], fill=0xFF, **KW, **kw, **SF)
    assert np.array_equal(a, b), np.argwhere(a != b)[:6]


@pytest.mark.parametrize("name", ["match", "gated", "lk4_fb", "stereo_lk"])
def test_sequence_engine_equals_the_pair_batch_for_every_window(ctx, scene, name):
    s, n = scene, 5
    want = np.stack([scenes.pair_record(ctx, s, t - 1, t, t - 1, **SEQ_KW, **SETTINGS[name], **SF) for t in range(1, n)])
    assert (want[:, 14] == 0).all() and (want[:, 12] > 30).all(), want[:, 12:16]
    for window in (1, 2, 5):
        eng = SequenceEngine(ctx, s["model"], RigConfig(**s["rig_kw"]), window=window, **SETTINGS[name], **SF, **SEQ_KW)
        got = scenes.hop_records(eng, s["seq"][:n], window)
        assert np.array_equal(got, want), (window, np.argwhere(got != want)[:6])
    off = SequenceEngine(ctx, s["model"], RigConfig(**s["rig_kw"]), window=5, cyclic_columns=True, **SETTINGS[name], **SEQ_KW)
    plain = scenes.hop_records(off, s["seq"][:n], 5)
    assert not np.array_equal(plain, want)


@pytest.mark.parametrize("name", ["match", "lk4_fb"])
def test_multi_sequence_lanes_equal_solo_engines(ctx, scene, name):
    s = scene
    seqs = [s["seq"][0:4], s["seq"][2:6]]
    new = lambda cls, **kw: cls(ctx, s["model"], RigConfig(**s["rig_kw"]), window=2, **SETTINGS[name], **SF, **kw, **SEQ_KW)  # noqa: E731
    got = scenes.drive_lanes(new(MultiSequenceEngine, lanes=2), seqs, 2)
    for k in range(2):
        want = scenes.drive(new(SequenceEngine), seqs[k], 2)
        assert len(got[k]) == len(want) == 4
        scenes.assert_same_drive(got[k], want)


@pytest.mark.parametrize("name", ["match", "lk4_fb_stereo_lk"])
def test_run_vo_pose_file_does_not_depend_on_the_frame_window(ctx, tmp_path, name):
    """An 11-frame sequence through run_VO with the option: byte-identical pose and keyframe files for frame windows 32, 5 and 1;
    the per-frame mirror path (frame_window 0) agrees to rtol 1e-6, atol 1e-9 on every pose, as tests/test_gpu_sequence.py
    asks of it; the demo's command line writes the same files."""
    import demo_vo_sos
    from vo_single_camera_sos_amd.omnistereo.gum import load_gums_json
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO
    n = 11      # (a sequence of this file's own: the demo writes into its directory)
    seq = scenes.write_sos_sequences(tmp_path, seeds=(77,), frames=n)[0]
    gums = os.path.join(seq, "gums-calibrated.json")
    cam = load_gums_json(gums)
    lk = dict(half=4, max_iter=10, fb_max=0.5)
    opt = dict(f2f_tracker="lk", lk=lk, stereo_refine="lk") if name.startswith("lk") else dict(f2f_tracker="match")
    texts, outs = scenes.run_vo_windows(cam, seq, n, tmp_path, (32, 5, 1, 0), cyclic_columns="seam_free", **opt)
    assert texts[32] == texts[5] == texts[1] and len(texts[32][0].splitlines()) == n
    for (i, Ta), (j, Tb) in zip(outs[0]["poses"], outs[32]["poses"]):
        assert i == j and np.allclose(Ta, Tb, rtol=1e-6, atol=1e-9), (i, np.abs(Ta - Tb).max())
    results = str(tmp_path / "results_plain")
    plain = run_VO(None, cam, **scenes.sos_kwargs(seq, n, results), frame_window=32, cyclic_columns=True, **opt)
    assert plain["tracked"] == n - 1 and scenes.read_results(results) != texts[32]       # the option does something
    flags = ["--f2f_tracker", "lk", "--lk_half", "4", "--lk_max_iter", "10", "--lk_fb_max", "0.5", "--stereo_refine", "lk"] \
        if name.startswith("lk") else []
    out = demo_vo_sos.main_sos_vo([seq, "--calibrated_gums_file", gums, "--frame_window", "5", "--seam_free"] + flags)
    assert out["tracked"] == n - 1
    assert scenes.read_results(os.path.join(seq, "results-omni")) == texts[32]


# ---- what the option is for ----------------------------------------------------------------------------------------------------
def _in_bands(x, cols):
    return (x < 31) | (x >= cols - 31)


def test_stereo_points_reach_the_seam_and_equal_the_cpu_flow(ctx, scene):
    """Frame 0 of the first pair.  The CPU flow on the padded model is the source of the numbers: it must have a stereo point
    inside the 31-column bands (the scene was picked so), and the device's frame record equals it row for row.  Outside the
    bands the seam-free record holds the plain run's points, give or take those that the changed masks' maxima move: the masks
    that touch the seam (0 and 11 of 12) see more pixels, so their threshold quality * maximum and their corner quota can
    differ, the other ten masks' points are the plain run's exactly."""
    s, omni = scene, scene["omni"][:2]
    m, cols = s["model"], s["model"].cols
    _, pipe = _pipeline(ctx, s, omni)
    _, pipe0 = _pipeline(ctx, s, omni, seam_free=False, cyclic_columns=True)
    M, M0 = int(pipe.frames["M"][0]), int(pipe0.frames["M"][0])
    top, bot = pipe.frames["m_top"][0, :M].cpu().numpy(), pipe.frames["m_bot"][0, :M].cpu().numpy()
    top0 = pipe0.frames["m_top"][0, :M0].cpu().numpy()
    # the CPU flow: detection on the padded model, the unpad, then the reference's static stereo
    ca, sa = orb_pattern.angle_cos_sin(orb_pattern.GFT_KEYPOINT_ANGLE)
    im = refflow.ImageModel(refseam.pad(m.map_x.cpu().numpy(), axis=2), refseam.pad(m.map_y.cpu().numpy(), axis=2), m.omni_masks.cpu().numpy(),
                            refseam.pad0(m.mask_bits_host), m.nmask, NFEAT, m.pattern_host, ca, sa, kp_cap=pipe.bucket_cap)
    import oracle.flow
    views = [oracle.flow.detect_view(im, omni[0], v)[:2] for v in (0, 1)]
    for kps, _ in views:
        for kp in kps:
            kp[:, 0] = refseam.unpad(kp[:, 0], cols)
    want = refflow.stereo_frame(refflow.RigParams(**s["rig_kw"]), views[0][0], views[1][0], views[0][1], views[1][1])
    n_band = int(_in_bands(want["m_top"][:, 0], cols).sum())
    print("frame 0: %d stereo points plain, %d seam-free (CPU flow: %d), %d of them inside the bands" % (M0, M, len(want["m_top"]), n_band))
    assert n_band >= 1                                             # the condition on the scene, from the CPU flow
    assert M == len(want["m_top"]) and np.array_equal(top, want["m_top"]) and np.array_equal(bot, want["m_bot"])
    assert int(_in_bands(top[:, 0], cols).sum()) == n_band and not _in_bands(top0[:, 0], cols).any()
    # outside the bands: the plain run's points, but for the masks beside the seam
    sector = cols // m.nmask
    inner = lambda p: p[(p[:, 0] >= sector) & (p[:, 0] < cols - sector)]  # noqa: E731
    assert np.array_equal(inner(top), inner(top0))
    outside, moved = top[~_in_bands(top[:, 0], cols)], 2 * NFEAT
    assert abs(len(outside) - M0) <= moved and len(outside) >= len(inner(top0))


def test_the_pair_batch_keeps_the_same_stereo_points(ctx, scene):
    """The frame store of the one-call batch (read through a sequence engine's counts): as many stereo points per frame as the
    pair pipeline's records hold."""
    s, omni = scene, scene["omni"]
    _, pipe = _pipeline(ctx, s, omni)
    want = pipe.frames["M"].cpu().numpy()
    eng = SequenceEngine(ctx, s["model"], RigConfig(**s["rig_kw"]), window=4, **SF, **dict(SEQ_KW, kp_cap=pipe.bucket_cap))
    got = [i["count"] for i in eng.push_window(list(omni))]
    assert list(got) == list(want) and min(got) > 50
