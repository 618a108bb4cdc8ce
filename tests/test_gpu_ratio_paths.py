"""GPU: the ratio rule through the whole paths -- the stage-by-stage pipelines, the one-call batches and their streams form,
the sequence and multi-sequence engines, run_VO with its window sizes and the mirror path, RGB-D -- against tests/refflow.py
with the definition (tests/refmatch.py) as its two matchers, bit for bit; and the relations the definition implies on the
six rendered pairs.  ("The patched refflow" below is that: refflow under a setting's matchers.)

The scenes are those of tests/test_gpu_gated_matching.py (matching_scenes.omni_pairs / rgbd_pairs, built once for both modules,
and its sequences).

RATIO: the smallest of 48, 54 and 58 (in 64ths) for which, in the ratio-only settings, the patched refflow alone gives status
0 and at least 20 correspondences for every pair (checked again on the CPU side of the fixtures below: a parity test on
starved pairs shows nothing).  Chosen: 54.  Observed on one MI355X build (correspondences of the two pair tracks and the three
sequence hops, the hop between the two unrelated pairs being the smallest): at r = 48 the minima are 145 (stereo), 7 (f2f), 5
(both) and 16 (RGB-D f2f), so 48 starves; at r = 54 they are 156 (stereo), 37 (f2f), 28 (both) and 67 (RGB-D f2f), every status
0; at r = 58: 174, 68, 57 and 163.

The stage-by-stage pipelines also run the two combinations of {ratio, gate, cross-check} the settings above leave out, at
r = 54 too (neither starves; observed minima, stereo points per frame / correspondences per pair): both + gated at no cap,
no cross-check 930 / 1088; gated + cross-check without the rule 805 / 984, RGB-D 233 correspondences (its smallest hop)."""
import os

import numpy as np
import pytest
import torch

import matching_scenes as scenes
import refflow
from matching_scenes import CX, CY, FX, FY, N_SEQ, Setting, read_results, record, rgbd_kwargs, sos_kwargs
from refmatch import Matching
from vo_single_camera_sos_amd import synthetic
from vo_single_camera_sos_amd.frontend import DeviceImageModel, ImageFrontEnd
from vo_single_camera_sos_amd.pipeline import (FramePairBatch, FramePairPipeline, RGBDCamConfig, RGBDPairBatch, RGBDPairPipeline,
                                               RigConfig)

pytestmark = pytest.mark.gpu

RATIO = 54            # in 64ths (0.84375); the observed minimum over the ratio-only settings is 28 correspondences
MIN_CORR = 20


# ---- the settings ------------------------------------------------------------------------------------------------------------
SETTINGS = [Setting("stereo", ratio="stereo", r=RATIO), Setting("f2f", ratio="f2f", r=RATIO), Setting("both", ratio="both", r=RATIO),
            Setting("both_with_cross_check", ratio="both", cc=True, r=RATIO),
            Setting("both_gated_cap80_with_cross_check", ratio="both", gate=True, cap=80, cc=True, r=RATIO)]
OFF = Setting("off", r=RATIO)
# the combinations of {ratio, gate, cross-check} the settings above leave out: for the stage-by-stage pipelines only
GATED_NO_CC = Setting("both_gated", ratio="both", gate=True, r=RATIO)
GATED_CC_NO_RATIO = Setting("gated_with_cross_check", gate=True, cc=True, r=RATIO)
BY_NAME = {s.name: s for s in SETTINGS + [GATED_NO_CC, GATED_CC_NO_RATIO]}
NAMES = [s.name for s in SETTINGS]


def _starvation_check(name, tracks):
    """The condition on the scene: under a ratio-only setting every pair of the patched refflow alone ends with status 0 and at
    least MIN_CORR correspondences (the figures are printed, and recorded in the module docstring)."""
    n = [len(w["corr"]["cam"] if "cam" in w["corr"] else w["corr"]["q"]) for w in tracks]
    status = [int(w["ransac"]["status"]) for w in tracks]
    print("ratio-only setting %s at r = %d: correspondences %s, status %s" % (name, RATIO, n, status))
    assert min(n) >= MIN_CORR and not any(status), (name, n, status)


@pytest.fixture(scope="module")
def pairs(ctx):
    """The scene of test_gpu_gated_matching's `pairs`: 2 rendered pairs (GFT 330 features), the front end on the GPU, the
    detection on the oracle (once, shared), the trackers' solver settings."""
    return scenes.omni_pairs(ctx)


@pytest.fixture(scope="module")
def rgbd(ctx):
    return scenes.rgbd_pairs(ctx)


@pytest.fixture(scope="module")
def sos_sequences(tmp_path_factory):
    return scenes.write_sos_sequences(tmp_path_factory.mktemp("ratio_sos"))


def reference(s, setting):
    """-> (frames, pair tracks with seed + i, sequence tracks of (t - 1, t) with seed t - 1) of the scene under the setting."""
    out = s.frames(setting), s.pair_tracks(setting), s.hop_tracks(setting)
    if setting.ratio_only:
        _starvation_check(setting.name, out[1] + out[2])
    return out


def test_the_patched_refflow_without_a_switch_is_refflow(pairs):
    """The definition with every switch off (matching=Matching()) gives the frames and tracks of refflow's own matcher
    (matching=None)."""
    s = pairs
    assert OFF.matchings() == (Matching(), Matching())
    frames, tracks, _ = reference(s, OFF)
    plain = [refflow.stereo_frame(s.rp, v[0][0], v[1][0], v[0][1], v[1][1]) for v in s.views]
    for a, b in zip(frames, plain):
        assert all(np.array_equal(a[k], b[k]) for k in ("m_top", "m_bot", "d_top", "d_bot", "X")) and a["n_cand"] == b["n_cand"]
    w = refflow.track_pair(s.rp, plain[0], plain[1], s.thr, 210, seed=s.seed, adaptive=True, gp3p=True)
    assert np.array_equal(record(w).view(np.uint64), record(tracks[0]).view(np.uint64))


# ---- the omni paths --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES + [GATED_NO_CC.name, GATED_CC_NO_RATIO.name])
def test_pair_pipeline_stage_by_stage_equals_the_patched_refflow(ctx, pairs, name):
    s, setting = pairs, BY_NAME[name]
    frames, want, _ = reference(s, setting)
    pipe = FramePairPipeline(ctx, RigConfig(**s.rig_kw), s.B, frame_cap=2048, seed=s.seed, front_end=s.fe, **s.solver,
                             **setting.omni_kw())
    pipe.stereo()
    pipe.track()
    rec = pipe.results().cpu().numpy()
    M, n_cand = pipe.frames["M"].cpu().numpy(), pipe.frames["n_cand"].cpu().numpy()
    print("setting %s at r = %d: stereo points of the patched refflow %s, correspondences %s"
          % (name, setting.r, [len(fr["X"]) for fr in frames], [len(w["corr"]["cam"]) for w in want]))
    assert [int(x) for x in M] == [len(fr["X"]) for fr in frames] and M.min() >= MIN_CORR
    assert [int(x) for x in n_cand] == [fr["n_cand"] for fr in frames]
    for f, fr in enumerate(frames):
        for key in ("m_top", "m_bot", "d_top", "d_bot", "X"):
            assert np.array_equal(pipe.frames[key][f, : M[f]].cpu().numpy(), fr[key]), (f, key)
    mask = pipe.ransac["mask"].cpu().numpy()
    cq, ct = pipe.corr["q"].cpu().numpy(), pipe.corr["t"].cpu().numpy()
    for i, w in enumerate(want):
        n = len(w["corr"]["cam"])
        assert n > 0 and np.array_equal(cq[i, :n], w["corr"]["q"]) and np.array_equal(ct[i, :n], w["corr"]["t"])
        assert np.array_equal(mask[i, :n].astype(bool), w["ransac"]["mask"])
        assert np.array_equal(rec[i].view(np.uint64), record(w).view(np.uint64))
    off = reference(s, OFF)
    if setting.ratio_stereo and not setting.gate:             # the rule only removes stereo points, and it removes some
        assert all(len(a["X"]) <= len(b["X"]) for a, b in zip(frames, off[0]))
        assert sum(len(a["X"]) for a in frames) < sum(len(b["X"]) for b in off[0])
    if not setting.changes_stereo:                            # the stereo stage is untouched by the f2f switch
        assert all(np.array_equal(a["X"], b["X"]) for a, b in zip(frames, off[0]))


@pytest.mark.parametrize("name", NAMES)
def test_one_call_batches_and_streams_equal_the_patched_refflow(ctx, pairs, name):
    s, setting = pairs, BY_NAME[name]
    want = np.stack([record(w) for w in reference(s, setting)[1]])
    kw = dict(num_of_features=s.nfeat, kp_cap=s.fe.kp_cap, frame_cap=2048, seed=s.seed, **s.solver, **setting.omni_kw())
    for ns in (1, 2):
        batch = FramePairBatch(ctx, s.model, RigConfig(**s.rig_kw), s.B, n_streams=ns, **kw)
        batch.workspace.fill_(0xA5)
        batch.load_frames(s.omni)
        for _ in range(2):
            got = batch.step().clone()
            ctx.synchronize()
            assert np.array_equal(got.cpu().numpy().view(np.uint64), want.view(np.uint64)), ns
        if ns == 2:                                          # the enqueue / join form
            bufs = [torch.zeros_like(batch.out), torch.zeros_like(batch.out)]
            for k in range(4):
                batch.enqueue(bufs[k & 1])
            batch.join()
            ctx.synchronize()
            for b in bufs:
                assert np.array_equal(b.cpu().numpy().view(np.uint64), want.view(np.uint64))
    assert not np.array_equal(want[:, :12], np.stack([record(w) for w in reference(s, OFF)[1]])[:, :12])


@pytest.mark.parametrize("name", NAMES)
def test_sequence_engines_equal_the_patched_refflow_for_windows_1_and_5(ctx, pairs, name):
    from vo_single_camera_sos_amd.pipeline import SequenceEngine
    s, setting = pairs, BY_NAME[name]
    want = np.stack([record(w) for w in reference(s, setting)[2]])
    kw = dict(num_of_features=s.nfeat, kp_cap=s.fe.kp_cap, frame_cap=2048, **s.solver, **setting.omni_kw())
    n = 2 * s.B
    for window in (1, 5):
        eng = SequenceEngine(ctx, s.model, RigConfig(**s.rig_kw), window=window, **kw)
        got = scenes.hop_records(eng, s.omni[:n], window)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), window


@pytest.mark.parametrize("name", NAMES)
def test_multi_sequence_engine_equals_the_patched_refflow(ctx, pairs, name):
    """Two lanes of one MultiSequenceEngine (window 2, so slots = 2 * (2 * 2 + 1) and a tracking call of up to 4 gathered pairs
    shares one rivals buffer): lane 0 gets the fixture's four frames, lane 1 the first three (a ragged last window), one thread
    each, as run_VO_many drives them.  Frame 0 of a lane becomes its keyframe; every later frame's speculative record (against
    its predecessor, seed t - 1) and its serial record against the keyframe slot (the lanes' serial calls of one moment share a
    launch) equal the patched refflow bit for bit."""
    from vo_single_camera_sos_amd.pipeline import MultiSequenceEngine
    s, setting = pairs, BY_NAME[name]
    frames, _, hops = reference(s, setting)
    # (0, t) with the seed of frame t: what the serial call against the keyframe computes
    serial = [None] + [record(s.track(setting, 0, t, t - 1)) for t in range(1, 2 * s.B)]
    kw = dict(num_of_features=s.nfeat, kp_cap=s.fe.kp_cap, frame_cap=2048, **s.solver, **setting.omni_kw())
    multi = MultiSequenceEngine(ctx, s.model, RigConfig(**s.rig_kw), lanes=2, window=2, **kw)
    assert multi.slots == 2 * (2 * 2 + 1) and multi.cfg.n_pairs == 2 * 2
    sequences = [s.omni[:4], s.omni[:3]]
    got = scenes.drive_lanes(multi, sequences, 2)
    for lane in range(2):
        assert len(got[lane]) == len(sequences[lane])
        for t, (count, seed, spec, _, rec) in enumerate(got[lane]):
            assert count == len(frames[t]["X"]), (lane, t)
            if t == 0:
                assert spec is None and rec is None
                continue
            assert seed == t - 1
            assert np.array_equal(np.asarray(spec).view(np.uint64), record(hops[t - 1]).view(np.uint64)), (lane, t, "speculative")
            assert np.array_equal(np.asarray(rec).view(np.uint64), serial[t].view(np.uint64)), (lane, t, "serial")
    c = multi.counters
    assert c["front_end_launches"] == c["rounds"] == 2 and c["max_serial_pairs"] == 2


# ---- RGB-D -------------------------------------------------------------------------------------------------------------------
RGBD_SETTINGS = [Setting("f2f", ratio="f2f", r=RATIO), Setting("f2f_with_cross_check", ratio="f2f", cc=True, r=RATIO),
                 Setting("f2f_gated", ratio="f2f", gate=True, r=RATIO), GATED_CC_NO_RATIO]


@pytest.mark.parametrize("setting", RGBD_SETTINGS, ids=[x.name for x in RGBD_SETTINGS])
def test_rgbd_pair_paths_and_sequence_equal_the_patched_refflow(ctx, rgbd, setting):
    from vo_single_camera_sos_amd.pipeline import RGBDSequenceEngine
    s = rgbd
    want = [s.track(setting, 2 * i, 2 * i + 1, 31 + i) for i in range(s.B)]
    want_seq_tracks = [s.track(setting, t - 1, t, t - 1) for t in range(1, 2 * s.B)]
    want_seq = np.stack([record(w) for w in want_seq_tracks])
    print("rgbd setting %s at r = %d: correspondences of the patched refflow %s"
          % (setting.name, setting.r, [len(w["corr"]["q"]) for w in want + want_seq_tracks]))
    if setting.ratio_only:
        _starvation_check("rgbd " + setting.name, want + want_seq_tracks)
    plain = [s.track(None, 2 * i, 2 * i + 1, 31 + i) for i in range(s.B)]
    pipe = RGBDPairPipeline(ctx, s.cam, s.B, seed=31, **s.kw, **setting.rgbd_kw())
    pipe.load_frames(s.bgr, s.depth)
    pipe.step()
    rec, mask = pipe.results().cpu().numpy(), pipe.ransac["mask"].cpu().numpy()
    cq, ct = pipe.corr["q"].cpu().numpy(), pipe.corr["t"].cpu().numpy()
    for i, w in enumerate(want):
        n = len(w["corr"]["q"])
        assert n > 0 and np.array_equal(cq[i, :n], w["corr"]["q"]) and np.array_equal(ct[i, :n], w["corr"]["t"])
        assert np.array_equal(mask[i, :n].astype(bool), w["ransac"]["mask"])
        assert np.array_equal(rec[i].view(np.uint64), record(w).view(np.uint64))
        if setting.ratio_only:                               # the kept correspondences are a proper subset of the plain ones
            assert set(zip(w["corr"]["q"], w["corr"]["t"])) < set(zip(plain[i]["corr"]["q"], plain[i]["corr"]["t"]))
    one = RGBDPairBatch(ctx, s.cam, s.B, seed=31, **s.kw, **setting.rgbd_kw())
    one.load_frames(s.bgr, s.depth)
    got = one.step()
    ctx.synchronize()
    assert np.array_equal(got.cpu().numpy().view(np.uint64), rec.view(np.uint64))
    for window in (1, 5):
        eng = RGBDSequenceEngine(ctx, s.cam, window=window, **s.kw, **setting.rgbd_kw())
        got = scenes.hop_records(eng, list(zip(s.bgr, s.depth)), window)
        assert np.array_equal(got.view(np.uint64), want_seq.view(np.uint64)), window


def test_rgbd_refuses_the_stereo_bit_and_a_switch_without_a_ratio(ctx):
    from vo_single_camera_sos_amd import _lib
    from vo_single_camera_sos_amd.device import SosvoError
    cam = RGBDCamConfig(fx=FX, fy=FY, center_x=CX, center_y=CY, depth_is_Z=True, min_range=0.8, max_range=7.0)
    one = RGBDPairBatch(ctx, cam, 1, num_of_features=100)
    flags = one.cfg.flags
    one.cfg.flags = flags | _lib.FLAG_RATIO_STEREO | (48 << _lib.RATIO_64THS_SHIFT)
    with pytest.raises(SosvoError, match="RATIO_STEREO"):
        one.step()
    one.cfg.flags = flags | _lib.FLAG_RATIO_F2F              # the field is 0
    with pytest.raises(SosvoError, match="SOSVO_RATIO_64THS"):
        one.step()


def test_omni_batch_refuses_a_switch_without_a_ratio(ctx, pairs):
    from vo_single_camera_sos_amd import _lib
    from vo_single_camera_sos_amd.device import SosvoError
    s = pairs
    batch = FramePairBatch(ctx, s.model, RigConfig(**s.rig_kw), s.B, num_of_features=s.nfeat, kp_cap=s.fe.kp_cap, frame_cap=2048)
    batch.load_frames(s.omni)
    batch.cfg.ransac_flags |= _lib.FLAG_RATIO_F2F
    with pytest.raises(SosvoError, match="SOSVO_RATIO_64THS"):
        batch.step()


# ---- run_VO: the sequence engines and the mirror path -----------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_run_vo_windows_and_mirror_path(ctx, sos_sequences, tmp_path, name):
    """The pose files are byte-identical for frame windows 5 and 1 and for the per-frame mirror path (frame_window 0: the
    FeatureMatcher objects of the camera model carry the ratio and apply it on the device)."""
    from vo_single_camera_sos_amd.omnistereo.gum import load_gums_json
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO
    seq, kw = sos_sequences[0], BY_NAME[name].run_vo_kw()
    model = load_gums_json(os.path.join(seq, "gums-calibrated.json"))
    files, outs = scenes.run_vo_windows(model, seq, N_SEQ, tmp_path, (5, 1, 0), **kw)
    assert "sequence_mode" in outs[5] and "sequence_mode" not in outs[0]
    assert files[5] == files[1] and outs[0]["keyframe_ids"] == outs[5]["keyframe_ids"]
    print("max |pose difference| mirror path against window 5: %.3e" % max(
        float(np.abs(Ta - Tb).max()) for (_, Ta), (_, Tb) in zip(outs[0]["poses"], outs[5]["poses"])))
    assert files[0] == files[5]
    res = str(tmp_path / "off")
    off = run_VO(None, model, frame_window=5, ratio_test=False, **sos_kwargs(seq, N_SEQ, res))
    assert off["tracked"] == N_SEQ - 1 and read_results(res)[0] != files[5][0]
    res = str(tmp_path / "none")                             # None is the tracker's own setting: off
    run_VO(None, model, frame_window=5, ratio=0.75, **sos_kwargs(seq, N_SEQ, res))
    assert read_results(res) == read_results(str(tmp_path / "off"))


def test_run_vo_mirror_path_pose_file_is_byte_identical_to_the_engines_without_a_switch(ctx, sos_sequences, tmp_path):
    """With every switch off too: the per-frame mirror path takes its direction angles and bearings from the stage the engines'
    stereo assembly uses (sosvo_pano_to_bearing), so its pose file is the engines' byte for byte.  (With numpy's arithmetic
    there, one elevation in 70 differed in its last bit and the poses in their 15th digit: at most 3.98e-15.)"""
    from vo_single_camera_sos_amd.omnistereo.gum import load_gums_json
    seq = sos_sequences[0]
    model = load_gums_json(os.path.join(seq, "gums-calibrated.json"))
    files, outs = scenes.run_vo_windows(model, seq, N_SEQ, tmp_path, (5, 0))
    print("max |pose difference| mirror path against window 5: %.3e" % max(
        float(np.abs(Ta - Tb).max()) for (_, Ta), (_, Tb) in zip(outs[0]["poses"], outs[5]["poses"])))
    assert outs[0]["tracked"] == N_SEQ - 1 and files[0] == files[5]


@pytest.mark.parametrize("name", NAMES)
def test_run_vo_many_equals_the_solo_runs(ctx, sos_sequences, tmp_path, name):
    """Two sequences through the two lanes of one MultiSequenceEngine (run_VO_many) write the pose and keyframe files of their
    solo run_VO runs, byte for byte."""
    from vo_single_camera_sos_amd.omnistereo.gum import load_gums_json
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO
    gums = os.path.join(sos_sequences[0], "gums-calibrated.json")
    want, outs = scenes.run_vo_many_against_solo(gums, sos_sequences, N_SEQ, tmp_path, **BY_NAME[name].run_vo_kw())
    assert all(o["sequence_mode"]["lanes"] == 2 for o in outs)
    assert want[0] != want[1]
    res = str(tmp_path / "off")                              # (the rule did something to these sequences)
    run_VO(None, load_gums_json(gums), frame_window=5, **sos_kwargs(sos_sequences[0], N_SEQ, res))
    assert read_results(res)[0] != want[0][0]


def test_run_vo_refuses_a_ratio_that_is_no_64th(ctx, sos_sequences, tmp_path):
    from vo_single_camera_sos_amd.omnistereo.gum import load_gums_json
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO
    seq = sos_sequences[0]
    model = load_gums_json(os.path.join(seq, "gums-calibrated.json"))
    with pytest.raises(ValueError, match="nearest admissible"):
        run_VO(None, model, frame_window=5, ratio_test=True, ratio=0.8, **sos_kwargs(seq, N_SEQ, str(tmp_path / "bad")))


def test_rgbd_run_vo(ctx, tmp_path):
    from vo_single_camera_sos_amd.omnistereo.camera_models import RGBDCamModel
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO
    from vo_single_camera_sos_amd.omnistereo.transformations import rotation_matrix
    seq = str(tmp_path / "seq_rgbd")
    synthetic.write_rgbd_sequence(seq, n_frames=N_SEQ, seed=41, max_t=40.0, max_deg=2.0, depth_is_Z=False)
    model = RGBDCamModel(fx=FX, fy=FY, center_x=CX, center_y=CY, scaling_factor=1. / 1000.0, do_undistortion=False,
                         depth_is_Z=False, focal_length_m=1. / 1000.0)
    model.T_Cest_wrt_Rgt = rotation_matrix(-np.pi / 2.0, [1, 0, 0])
    files, outs = {}, {}
    for w in (5, 1, 0):
        res = str(tmp_path / ("w%d" % w))
        outs[w] = run_VO(None, model, frame_window=w, ratio_test=True, ratio=RATIO / 64.0, **rgbd_kwargs(seq, N_SEQ, res))
        files[w] = read_results(res)
        assert outs[w]["tracked"] == N_SEQ - 1
    assert files[5] == files[1] and files[0] == files[5]
    res = str(tmp_path / "off")
    run_VO(None, model, frame_window=5, **rgbd_kwargs(seq, N_SEQ, res))
    assert read_results(res)[0] != files[5][0]
    with pytest.raises(ValueError, match="no static-stereo matcher"):
        run_VO(None, model, frame_window=5, ratio_test="stereo", ratio=0.75, **rgbd_kwargs(seq, N_SEQ, str(tmp_path / "bad")))


# ---- the mirror matcher against the definition -------------------------------------------------------------------------------
def test_feature_matcher_with_a_ratio_equals_the_definition(ctx):
    from vo_single_camera_sos_amd.omnistereo.camera_models import FeatureMatcher
    rng = np.random.default_rng(5)
    desc, pos = scenes.descriptor_scene(rng, 2, 320, np.array([257, 300]))
    q, t, qp, tp = desc[1, :300], desc[0, :257], pos[1, :300], pos[0, :257]
    fm = FeatureMatcher("ORB", "BF", 1, context=ctx, ratio=0.75)
    plain = FeatureMatcher("ORB", "BF", 1, context=ctx).match(q, t)
    gate = (1.0, 2.5)
    for got, want in ((fm.match(q, t), Matching(ratio=48)(q, t, qp, tp, None)),
                      (fm.match_gated(q, t, qp, tp, 1.0, 2.5), Matching(gated=True, ratio=48)(q, t, qp, tp, gate)),
                      (fm.match_gated(q, t, qp, tp, 1.0, 2.5, max_distance=4), Matching(gated=True, cap=4, ratio=48)(q, t, qp, tp, gate)),
                      (MatchListOf(fm.match_arrays_many([(q, t), (t, q), (q[:0], t), (q, t[:1])])[0]),
                       Matching(ratio=48)(q, t, qp, tp, None))):
        wq, wt, wd = want
        assert 0 < len(wq) < 300
        assert np.array_equal(got.query_idx, wq) and np.array_equal(got.train_idx, wt) and np.array_equal(got.distances, wd)
    assert set(zip(fm.match(q, t).query_idx, fm.match(q, t).train_idx)) < set(zip(plain.query_idx, plain.train_idx))
    many = fm.match_arrays_many([(q, t), (t, q), (q[:0], t), (q, t[:1])])
    assert len(many[2][0]) == 0 and len(many[3][0]) == 0      # no query; a single train: no runner-up, dropped in the plain form
    assert len(fm.match_gated(q[:1], t[:1], qp[:1], qp[:1] + np.float32([0.0, 2.0]), 1.0, 2.5)) == 1   # ... kept in the gated one
    fmc = FeatureMatcher("ORB", "BF", 1, context=ctx, ratio=0.75, cross_check=True)
    for got, want in ((fmc.match(q, t), Matching(mutual=True, ratio=48)(q, t, qp, tp, None)),
                      (fmc.match_gated(q, t, qp, tp, 1.0, 2.5, max_distance=80),
                       Matching(gated=True, cap=80, mutual=True, ratio=48)(q, t, qp, tp, gate))):
        wq, wt, wd = want
        assert 0 < len(wq) and np.array_equal(got.query_idx, wq) and np.array_equal(got.train_idx, wt) and np.array_equal(got.distances, wd)


class MatchListOf(object):
    def __init__(self, triple):
        self.query_idx, self.train_idx, self.distances = triple


# ---- the relations of the definition on the six rendered pairs ----------------------------------------------------------------
def test_kept_matches_are_matches_without_the_rule_and_grow_with_the_ratio(ctx):
    """The six rendered pairs of test_gpu_cross_check.py (seed 4100, GFT 1000 features, kp_cap 512, frame_cap 2048).  Every
    stereo point / frame-to-frame correspondence kept under a ratio setting is one of the same setting without the rule, and
    the kept counts do not fall as r grows (32, 48, 58, 63)."""
    B = 6
    gs, rig_kw = scenes.rig()
    omni, _ = synthetic.make_frame_pairs(gs, B, seed=4100)
    model = DeviceImageModel(ctx, gs, (480, 640))
    fe = ImageFrontEnd(ctx, model, 2 * B, detection_method="GFT", num_of_features=1000, kp_cap=512)
    fe.load_frames(omni)
    fe.run()

    def run(**kw):
        pipe = FramePairPipeline(ctx, RigConfig(**rig_kw), B, frame_cap=2048, max_iter=200, seed=11, front_end=fe, **kw)
        pipe.stereo()
        ctx.synchronize()
        fr = {k: v.cpu().numpy() for k, v in pipe.frames.items()}
        stereo = []
        for f in range(2 * B):
            m = int(fr["M"][f])
            stereo.append(set(map(bytes, np.hstack([fr["m_top"][f, :m], fr["m_bot"][f, :m]]))))
        return stereo, pipe

    def f2f_of(pipe, frames_from):
        """The frame-to-frame correspondences of `pipe` on the frames of `frames_from` (the same train and query sets)."""
        for k in pipe.frames:
            pipe.frames[k].copy_(frames_from.frames[k])
        pipe.track()
        ctx.synchronize()
        co = {k: v.cpu().numpy() for k, v in pipe.corr.items()}
        out = []
        for i in range(B):
            n, nt = int(co["n"][i]), int(co["n_top"][i])
            out.append([set(zip(co["q"][i, lo:hi].tolist(), co["t"][i, lo:hi].tolist())) for lo, hi in ((0, nt), (nt, n))])
        return out
    for base in (dict(), dict(gated_stereo=True, gated_f2f=True, gated_max_distance=100), dict(cross_check_stereo=True, cross_check_f2f=True)):
        plain_s, plain_pipe = run(**base)
        plain_f = f2f_of(plain_pipe, plain_pipe)
        last_s, last_f = None, None
        for r in (32, 48, 58, 63):
            kept_s, pipe = run(ratio_stereo=True, ratio_f2f=True, ratio=r / 64.0, **base)
            kept_f = f2f_of(pipe, plain_pipe)
            for f in range(2 * B):
                assert kept_s[f] <= plain_s[f], (base, r, f)
            for i in range(B):
                for view in range(2):
                    assert kept_f[i][view] <= plain_f[i][view], (base, r, i, view)
            ns, nf = [len(x) for x in kept_s], [[len(v) for v in p] for p in kept_f]
            if last_s is not None:
                assert all(a >= b for a, b in zip(ns, last_s)) and all(a >= b for p, q in zip(nf, last_f) for a, b in zip(p, q)), (base, r)
            last_s, last_f = ns, nf
            print("%s r = %d: stereo points per frame %s of %s; correspondences per pair and view %s of %s" % (
                sorted(base), r, ns, [len(x) for x in plain_s], nf, [[len(v) for v in p] for p in plain_f]))
        assert sum(last_s) < sum(len(x) for x in plain_s) and sum(last_s) > 0
