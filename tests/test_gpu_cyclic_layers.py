"""GPU: cyclic panorama columns in the layers.  First the pair pipeline
(FramePairPipeline(cyclic_columns=True)) on two
rendered pairs whose second frame is the first turned about the vertical axis, so that every feature moves sideways and the
ones beside the seam move across it.  With the option the correspondences hold pairs whose two columns lie more than half a
panorama apart and RANSAC keeps some of them; without it none crosses.  Once with the matcher (plain and gated), once with
the Lucas-Kanade tracker.

The angles: the front end keeps no keypoint within 31 columns of either border, so a MATCHED pair crosses only when the shift is
between 63 columns and the gate (75 = cols / 16 at 1200 columns): 21 degrees = 70 columns.  A TRACKED point needs 32 columns or
more: 11 degrees = 36.7 columns, within reach of a 21 x 21 window over 4 levels with the forward-backward check (on the
first run: 584 against 519 correspondences on the pair that turns one way, 2 of them across the seam and both inliers,
rotation error 0.03 / 0.06 degrees; at 12 degrees or without the check the tracker itself starts to fail on these pairs,
with and without the option).

Then SOSVO_FLAG_CYCLIC_F2F in the one-call batches, sequence mode and run_VO (the second half of the file), every record bit
for bit, with the matcher and with the tracker: the one-call batch equals the pair pipeline, also over two internal streams;
records do not depend on the workspace's contents; the sequence engine equals the pair batch for windows 1, 2 and 5; the
lanes of a multi-sequence engine equal solo engines; run_VO writes the same pose file whatever the frame window."""
import os

import numpy as np
import pytest

import matching_scenes as scenes
import synth
from matching_scenes import FRAME_CAP, ITERS, KW, LK_CHECKED, LK_WAVE, NFEAT, SEQ_KW
from vo_single_camera_sos_amd.frontend import ImageFrontEnd
from vo_single_camera_sos_amd.pipeline import FramePairPipeline, MultiSequenceEngine, RigConfig, SequenceEngine

pytestmark = pytest.mark.gpu

YAW_MATCH, YAW_LK = 21.0, 11.0
LK = dict(half=10, levels=4, max_iter=30, fb_max=0.5)


@pytest.fixture(scope="module")
def rigs(ctx):
    """The rig, and per yaw angle a front end that has run on the turning scene's two pairs."""
    s = scenes.turning_scene(ctx)
    out = dict(rig_kw=s["rig_kw"], cols=int(s["rig_kw"]["pano_top"][0]))
    for yaw in (YAW_MATCH, YAW_LK):
        fe = ImageFrontEnd(ctx, s["model"], 4, detection_method="GFT", num_of_features=330, keep_panoramas=False)
        fe.load_frames(s["yaw_omni"][yaw])
        fe.run()
        out[yaw] = (fe, s["yaw_poses"][yaw])
    return out


def _run(ctx, rigs, yaw, **kw):
    """-> (records [2, 16], rows): rows[i] = per correspondence of pair i (cam, u_ref, u_cur, inlier)."""
    fe, poses = rigs[yaw]
    pipe = FramePairPipeline(ctx, RigConfig(**rigs["rig_kw"]), 2, frame_cap=2048, max_iter=500, seed=5, front_end=fe, **kw)
    pipe.stereo()
    pipe.track()
    rec = pipe.results().cpu().numpy()
    ctx.synchronize()
    co = {k: v.cpu().numpy() for k, v in pipe.corr.items()}
    m = [pipe.frames["m_top"].cpu().numpy(), pipe.frames["m_bot"].cpu().numpy()]
    inl = pipe.ransac["mask"].cpu().numpy()
    trk = pipe._lk_out[0].cpu().numpy() if pipe.lk is not None else None
    rows = []
    for i in range(2):
        n = int(co["n"][i])
        cam, t, q = co["cam"][i, :n], co["t"][i, :n], co["q"][i, :n]
        u_ref = np.array([m[c][2 * i, k, 0] for c, k in zip(cam, t)])
        if trk is None:
            u_cur = np.array([m[c][2 * i + 1, k, 0] for c, k in zip(cam, q)])
        else:
            u_cur = np.array([trk[c * 2 + i, k, 0] for c, k in zip(cam, t)])
        rows.append(dict(cam=cam, t=t, q=q, u_ref=u_ref, u_cur=u_cur, inlier=inl[i, :n] != 0))
    rot = [np.degrees(synth.pose_error(rec[i, :12].reshape(3, 4), R, t)[0]) for i, (R, t) in enumerate(poses)]
    return rec, rows, rot


def _crossed(rows, cols):
    return [np.abs(r["u_cur"].astype(np.float64) - r["u_ref"]) > cols / 2 for r in rows]


@pytest.mark.parametrize("gated", [False, True])
def test_matched_pairs_cross_the_seam_with_the_option_only(ctx, rigs, gated):
    cols = rigs["cols"]
    kw = dict(gated_f2f=True) if gated else {}
    rec0, rows0, rot0 = _run(ctx, rigs, YAW_MATCH, **kw)
    rec1, rows1, rot1 = _run(ctx, rigs, YAW_MATCH, cyclic_columns=True, **kw)
    c0, c1 = _crossed(rows0, cols), _crossed(rows1, cols)
    print("matcher%s, yaw %.1f deg: correspondences %s -> %s, crossing %s -> %s (inliers among them %s), rotation error %s -> %s deg"
          % (" (gated)" if gated else "", YAW_MATCH, [len(r["t"]) for r in rows0], [len(r["t"]) for r in rows1], [int(c.sum()) for c in c0],
             [int(c.sum()) for c in c1], [int((c & r["inlier"]).sum()) for c, r in zip(c1, rows1)], ["%.3f" % r for r in rot0],
             ["%.3f" % r for r in rot1]))
    assert not any(c.any() for c in c0)                           # without the option none crosses
    assert sum(int(c.sum()) for c in c1) >= 1
    assert sum(int((c & r["inlier"]).sum()) for c, r in zip(c1, rows1)) >= 1
    assert (rec1[:, 14] == 0).all() and max(rot1) < 5.0
    for r0, r1, cross in zip(rows0, rows1, c1):
        if not gated:
            # the matcher is the same search: the cyclic gate only adds rows, in rank order per view -- the plain run's
            # correspondences are a subsequence of the cyclic run's, and what is added is exactly what crossed
            keep = ~cross
            for k in ("cam", "q", "t"):
                assert np.array_equal(r1[k][keep], r0[k]), k
        assert len(r1["t"]) >= len(r0["t"])


def test_tracked_points_cross_the_seam_with_the_option_only(ctx, rigs):
    cols = rigs["cols"]
    rec0, rows0, rot0 = _run(ctx, rigs, YAW_LK, f2f_tracker="lk", lk=LK)
    rec1, rows1, rot1 = _run(ctx, rigs, YAW_LK, f2f_tracker="lk", lk=LK, cyclic_columns=True)
    c0, c1 = _crossed(rows0, cols), _crossed(rows1, cols)
    print("lk half 10 / 4 levels + forward-backward 0.5 px, yaw %.1f deg: correspondences %s -> %s, crossing %s -> %s (inliers among them %s), rotation error "
          "%s -> %s deg" % (YAW_LK, [len(r["t"]) for r in rows0], [len(r["t"]) for r in rows1], [int(c.sum()) for c in c0],
                            [int(c.sum()) for c in c1], [int((c & r["inlier"]).sum()) for c, r in zip(c1, rows1)],
                            ["%.3f" % r for r in rot0], ["%.3f" % r for r in rot1]))
    assert not any(c.any() for c in c0)
    assert sum(int(c.sum()) for c in c1) >= 1
    assert sum(int((c & r["inlier"]).sum()) for c, r in zip(c1, rows1)) >= 1
    assert (rec1[:, 14] == 0).all() and max(rot1) < 5.0
    for r in rows1:
        assert ((r["u_cur"] >= 0) & (r["u_cur"] < cols)).all() and (r["q"] == -1).all()


def test_with_the_gate_disabled_the_option_changes_no_row(ctx, rigs):
    """f2f_max_hdiff < 0: both forms of the gate pass everything, the matcher path gives the plain pipeline's records and
    correspondences, row for row."""
    rig_kw = dict(rigs["rig_kw"], f2f_max_hdiff=-1.0)
    fe, _ = rigs[YAW_MATCH]
    out = []
    for kw in ({}, dict(cyclic_columns=True)):
        pipe = FramePairPipeline(ctx, RigConfig(**rig_kw), 2, frame_cap=2048, max_iter=200, seed=5, front_end=fe, **kw)
        pipe.stereo()
        pipe.track()
        ctx.synchronize()
        out.append((pipe.results().cpu().numpy(), {k: v.cpu().numpy() for k, v in pipe.corr.items()}))
    assert np.array_equal(out[0][0], out[1][0])
    for k in ("n", "n_top", "cam", "q", "t"):
        assert np.array_equal(out[0][1][k], out[1][1][k])


def test_the_constructor_refuses_what_cannot_be_cyclic(ctx, rigs):
    fe, _ = rigs[YAW_LK]
    rig_kw = rigs["rig_kw"]

    def wide(w):
        return RigConfig(**dict(rig_kw, pano_top=(w,) + tuple(rig_kw["pano_top"][1:]), pano_bot=(w,) + tuple(rig_kw["pano_bot"][1:])))
    with pytest.raises(ValueError, match="1204"):                 # 1204 is no multiple of 8
        FramePairPipeline(ctx, wide(1204), 2, front_end=fe, f2f_tracker="lk", lk=dict(half=4, levels=4), cyclic_columns=True)
    with pytest.raises(ValueError, match="1200.5"):
        FramePairPipeline(ctx, wide(1200.5), 2, front_end=fe, cyclic_columns=True)
    with pytest.raises(ValueError, match="ratio"):
        FramePairPipeline(ctx, RigConfig(**rig_kw), 2, front_end=fe, gated_f2f=True, ratio_f2f=True, ratio=0.75, cyclic_columns=True)
    assert FramePairPipeline(ctx, wide(1204), 2, front_end=fe, cyclic_columns=True).cyclic        # the matcher takes any integer width
    assert not FramePairPipeline(ctx, wide(1204), 2, front_end=fe, f2f_tracker="lk", lk=dict(half=4, levels=4)).cyclic


# ---- the batched layers: SOSVO_FLAG_CYCLIC_F2F in the one-call batches, sequence mode and run_VO --------------------------------
# Every record comparison is bit for bit, each once with the matcher (plain and gated) and once with the tracker, as
# tests/test_gpu_lk_layers.py does for the tracker alone, with its settings (matching_scenes): the turning scene's yaw pairs (21
# degrees for the matcher, 11 for the tracker) and its 6-frame sequence.
CYC = dict(cyclic_columns=True)
SETTINGS = {"match": {}, "gated": dict(gated_f2f=True), "lk4_fb": dict(f2f_tracker="lk", lk=LK_CHECKED),
            "lk10": dict(f2f_tracker="lk", lk=LK_WAVE), "lk10_4_fb": dict(f2f_tracker="lk", lk=LK)}


def _omni_of(s, name):
    return s["yaw_omni"][YAW_LK if name.startswith("lk") else YAW_MATCH]


@pytest.mark.parametrize("name", list(SETTINGS))
def test_one_call_batch_equals_the_pair_pipeline_also_over_two_streams(ctx, name):
    s = scenes.turning_scene(ctx)
    kw, omni = SETTINGS[name], _omni_of(s, name)
    fe = ImageFrontEnd(ctx, s["model"], 4, detection_method="GFT", num_of_features=NFEAT, keep_panoramas=False)
    pipe = FramePairPipeline(ctx, RigConfig(**s["rig_kw"]), 2, frame_cap=FRAME_CAP, max_iter=ITERS, seed=5, front_end=fe, **kw, **CYC)
    fe.load_frames(omni)
    pipe.step()
    want = pipe.results().cpu().numpy()
    got = scenes.batch_records(ctx, s, omni, kp_cap=fe.kp_cap, **KW, **kw, **CYC)
    assert (want[:, 14] == 0).all() and (want[:, 13] > 50).all(), want[:, 12:16]
    assert np.array_equal(got, want), np.argwhere(got != want)[:6]
    two = scenes.batch_records(ctx, s, omni, kp_cap=fe.kp_cap, n_streams=2, **KW, **kw, **CYC)
    assert np.array_equal(two, want), np.argwhere(two != want)[:6]
    plain = scenes.batch_records(ctx, s, omni, kp_cap=fe.kp_cap, **KW, **kw)
    # the bit does something on these pairs -- where a window can reach the seam at all: a window of half 4 over 3 levels
    # spans 24 columns and no keypoint lies within 31 of the border, and two levels of half 10 do not follow 37 columns
    if name in ("match", "gated", "lk10_4_fb"):
        assert not np.array_equal(got, plain)
    if name == "match":      # more correspondences: the crossings (a gated search finds every query a partner either way)
        assert (got[:, 13] >= plain[:, 13]).all() and got[:, 13].sum() > plain[:, 13].sum()


@pytest.mark.parametrize("name", ["match", "lk4_fb"])
def test_records_do_not_depend_on_the_workspaces_contents(ctx, name):
    s = scenes.turning_scene(ctx)
    kw, omni = SETTINGS[name], _omni_of(s, name)
    a = scenes.batch_records(ctx, s, omni, fill=0x00, **KW, **kw, **CYC)
    b = scenes.batch_records(ctx, s, omni, fill=0xFF, **KW, **kw, **CYC)
    assert np.array_equal(a, b), np.argwhere(a != b)[:6]


@pytest.mark.parametrize("name", ["match", "gated", "lk4_fb", "lk10"])
def test_sequence_engine_equals_the_pair_batch_for_every_window(ctx, name):
    s = scenes.turning_scene(ctx)
    n = 5
    want = np.stack([scenes.pair_record(ctx, s, t - 1, t, t - 1, **SEQ_KW, **SETTINGS[name], **CYC) for t in range(1, n)])
    assert (want[:, 14] == 0).all() and (want[:, 12] > 30).all(), want[:, 12:16]
    for window in (1, 2, 5):
        eng = SequenceEngine(ctx, s["model"], RigConfig(**s["rig_kw"]), window=window, **SETTINGS[name], **CYC, **SEQ_KW)
        got = scenes.hop_records(eng, s["seq"][:n], window)
        assert np.array_equal(got, want), (window, np.argwhere(got != want)[:6])
    off = SequenceEngine(ctx, s["model"], RigConfig(**s["rig_kw"]), window=5, **SETTINGS[name], **SEQ_KW)
    plain = scenes.hop_records(off, s["seq"][:n], 5)
    assert not np.array_equal(plain, want)


@pytest.mark.parametrize("name", ["match", "lk4_fb"])
def test_multi_sequence_lanes_equal_solo_engines(ctx, name):
    s = scenes.turning_scene(ctx)
    seqs = [s["seq"][0:4], s["seq"][2:6]]
    new = lambda cls, **kw: cls(ctx, s["model"], RigConfig(**s["rig_kw"]), window=2, **SETTINGS[name], **CYC, **kw, **SEQ_KW)  # noqa: E731
    got = scenes.drive_lanes(new(MultiSequenceEngine, lanes=2), seqs, 2)
    for k in range(2):
        want = scenes.drive(new(SequenceEngine), seqs[k], 2)
        assert len(got[k]) == len(want) == 4
        scenes.assert_same_drive(got[k], want)


@pytest.mark.parametrize("name", ["match", "lk4_fb"])
def test_run_vo_pose_file_does_not_depend_on_the_frame_window(ctx, tmp_path, name):
    """A 12-frame sequence through run_VO with the option: byte-identical pose and keyframe files for frame windows 32, 5 and 1;
    the per-frame mirror path (frame_window 0) agrees to rtol 1e-6, atol 1e-9 on every pose, as tests/test_gpu_sequence.py
    asks of it; the demo's command line writes the same files."""
    import demo_vo_sos
    from vo_single_camera_sos_amd.omnistereo.gum import load_gums_json
    n = 12
    seq = scenes.write_sos_sequences(tmp_path, seeds=(77,), frames=n)[0]
    gums = os.path.join(seq, "gums-calibrated.json")
    cam = load_gums_json(gums)
    lk = dict(half=4, max_iter=10, fb_max=0.5)
    opt = dict(f2f_tracker="lk", lk=lk) if name.startswith("lk") else dict(f2f_tracker="match")
    texts, outs = scenes.run_vo_windows(cam, seq, n, tmp_path, (32, 5, 1, 0), cyclic_columns=True, **opt)
    assert texts[32] == texts[5] == texts[1] and len(texts[32][0].splitlines()) == n
    for (i, Ta), (j, Tb) in zip(outs[0]["poses"], outs[32]["poses"]):
        assert i == j and np.allclose(Ta, Tb, rtol=1e-6, atol=1e-9), (i, np.abs(Ta - Tb).max())
    flags = ["--f2f_tracker", "lk", "--lk_half", "4", "--lk_max_iter", "10", "--lk_fb_max", "0.5"] if name.startswith("lk") else []
    out = demo_vo_sos.main_sos_vo([seq, "--calibrated_gums_file", gums, "--frame_window", "5", "--cyclic_columns"] + flags)
    assert out["tracked"] == n - 1
    assert scenes.read_results(os.path.join(seq, "results-omni")) == texts[32]
