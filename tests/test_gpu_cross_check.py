"""GPU: mutual-consistency (cross-check) matching, cv2.BFMatcher(NORM_HAMMING, crossCheck=True) -- the matcher the
reference carries commented out at omnistereo/camera_models.py:401 -- through every layer: the stage entry
(sosvo_cross_check_matches), FeatureMatcher, the pair pipelines and one-call batches, the sequence engines behind run_VO /
run_VO_many, and what the filter is for.

The CPU checker is the definition (tests/refmatch.py, Matching(mutual=True)): query i keeps its best train j iff the best
query of j, found by the same search with the roles swapped, is i.  refflow's flow functions take it as the matcher of either
stage (matching_scenes.Setting.matchings).  Everything is compared bit for bit or byte for byte; the mirror path
(frame_window 0) to 1e-6, as the existing sequence tests compare it."""
import os

import numpy as np
import pytest
import torch

import matching_scenes as scenes
import oracle
import refflow
import synth
from matching_scenes import CX, CY, FX, FY, N_SEQ, Setting, dev as _dev, read_results, rgbd_kwargs, sos_kwargs
from refmatch import IDX, NONE, Matching
from vo_single_camera_sos_amd import synthetic
from vo_single_camera_sos_amd.frontend import DeviceImageModel, ImageFrontEnd
from vo_single_camera_sos_amd.omnistereo.camera_models import FeatureMatcher
from vo_single_camera_sos_amd.pipeline import FramePairBatch, FramePairPipeline, RGBDPairBatch, RGBDPairPipeline, RigConfig

pytestmark = pytest.mark.gpu

MUTUAL = Matching(mutual=True)


def _descriptors(rng, nq, nt, stride):
    """Random descriptors; every third query is a train descriptor with 0-6 flipped bits (several queries may pick the same
    train: the filter has something to reject), and some trains are copies of each other (ties)."""
    q = rng.integers(0, 256, (stride, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (stride, 32), dtype=np.uint8)
    if nt > 0:
        for j in range(1, nt, 7):
            t[j] = t[rng.integers(0, j)]
        for i in range(0, nq, 3):
            d = t[rng.integers(0, max(1, nt // 2))].copy()
            for b in rng.integers(0, 256, rng.integers(0, 7)):
                d[b >> 3] ^= np.uint8(1 << (b & 7))
            q[i] = d
    return q, t


def _check_stage(ctx, q, t, nq, nt, q_slot=None, t_slot=None):
    """keys_out, n_kept and the sort order of one sosvo_cross_check_matches call against the composition -> the host keys."""
    P = len(nq) if q_slot is None else len(q_slot)
    qs = np.arange(P) if q_slot is None else q_slot
    ts = np.arange(P) if t_slot is None else t_slot
    dq, dt, dnq, dnt = _dev(ctx, q), _dev(ctx, t), _dev(ctx, nq.astype(np.int32)), _dev(ctx, nt.astype(np.int32))
    sl = {} if q_slot is None else dict(q_slot=_dev(ctx, q_slot.astype(np.int32)), t_slot=_dev(ctx, t_slot.astype(np.int32)))
    sl_rev = {} if q_slot is None else dict(q_slot=sl["t_slot"], t_slot=sl["q_slot"])
    fwd = ctx.match_hamming(dq, dt, dnq, dnt, k=1, **sl)
    rev = ctx.match_hamming(dt, dq, dnt, dnq, k=1, **sl_rev)
    out, n_kept = ctx.cross_check_matches(fwd, rev, dnq, dnt, **sl)
    order = ctx.sort_matches(out, dnq, q_slot=sl.get("q_slot"))
    alias = fwd.clone()
    out2, n_kept2 = ctx.cross_check_matches(alias, rev, dnq, dnt, keys_out=alias, **sl)   # keys_out aliased onto keys_fwd
    ctx.synchronize()
    assert out2.data_ptr() == alias.data_ptr()
    out_h, order_h, out2_h = out.cpu().numpy()[:, :, 0], order.cpu().numpy(), out2.cpu().numpy()[:, :, 0]
    assert np.array_equal(n_kept.cpu().numpy(), n_kept2.cpu().numpy())
    for p in range(P):
        n = int(nq[qs[p]])
        qd, td = q[qs[p], :n], t[ts[p], : int(nt[ts[p]])]
        want = MUTUAL.kept(qd, td, None, None, None)
        kept = int((want != NONE).sum())
        assert np.array_equal(out_h[p, :n], want), p
        assert np.array_equal(out2_h[p, :n], want), p
        assert int(n_kept.cpu().numpy()[p]) == kept, p
        assert np.array_equal(order_h[p, :n], oracle.sort_matches(want)), p
        assert np.array_equal(order_h[p, :kept], MUTUAL(qd, td, None, None, None)[0]), p
    return out_h


# ---- 1. the stage ----------------------------------------------------------------------------------------------------------
def test_stage_equals_the_oracle_composition(ctx):
    rng = np.random.default_rng(2024)
    shapes = [(0, 5), (5, 0), (1, 1), (31, 33), (129, 127), (300, 257)]   # the 32-query / 128-train tile edges of the matcher
    S = 320
    q, t = zip(*[_descriptors(rng, a, b, S) for a, b in shapes])
    nq, nt = np.array([s[0] for s in shapes]), np.array([s[1] for s in shapes])
    out = _check_stage(ctx, np.stack(q), np.stack(t), nq, nt)
    kept = [(out[p, : nq[p]] != NONE).sum() for p in range(len(shapes))]
    assert kept[0] == 0 and kept[1] == 0 and kept[2] == 1
    assert 0 < kept[4] < 129 and 0 < kept[5] < 257          # the filter rejected some and kept some


def test_stage_tie_case(ctx):
    """Trains 3 and 7 are identical and equal to queries 2 and 5: both queries choose train 3 (lowest index), train 3 and
    train 7 both choose query 2 -> query 2 keeps train 3, query 5 is rejected, no query keeps train 7."""
    rng = np.random.default_rng(7)
    q = rng.integers(0, 256, (1, 16, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (1, 16, 32), dtype=np.uint8)
    t[0, 7] = t[0, 3]
    q[0, 2] = q[0, 5] = t[0, 3]
    out = _check_stage(ctx, q, t, np.array([8]), np.array([10]))[0, :8]
    assert out[2] == 3                                       # distance 0, train 3
    assert out[5] == NONE
    assert not ((out != NONE) & ((out & IDX) == 7)).any()


def test_stage_with_slots(ctx):
    """A store of 3 blocks, problems (cur, ref) = (1, 0), (2, 0), (2, 1): what a tracking call matches."""
    rng = np.random.default_rng(11)
    S, M = 320, np.array([200, 129, 33])
    store = rng.integers(0, 256, (3, S, 32), dtype=np.uint8)
    for b in (1, 2):                                         # later blocks re-observe earlier ones, with noise and repeats
        for i in range(0, M[b], 2):
            d = store[b - 1, rng.integers(0, M[b - 1] // 2)].copy()
            d[rng.integers(0, 32)] ^= np.uint8(1 << rng.integers(0, 8))
            store[b, i] = d
    out = _check_stage(ctx, store, store, M, M, q_slot=np.array([1, 2, 2]), t_slot=np.array([0, 0, 1]))
    assert all(0 < (out[p, :n] != NONE).sum() < n for p, n in enumerate((129, 33, 33)))


# ---- 2. FeatureMatcher -------------------------------------------------------------------------------------------------------
def test_feature_matcher_cross_check(ctx):
    rng = np.random.default_rng(5)
    q, t = _descriptors(rng, 300, 257, 320)
    q, t = q[:300], t[:257]
    plain = FeatureMatcher("ORB", "BF", 1, context=ctx).match(q, t)
    fm = FeatureMatcher("ORB", "BF", 1, context=ctx, cross_check=True)
    got = fm.match(q, t)
    wq, wt, wd = MUTUAL(q, t, None, None, None)
    assert 0 < len(wq) < 300
    assert np.array_equal(got.query_idx, wq) and np.array_equal(got.train_idx, wt) and np.array_equal(got.distances, wd)
    assert [m.queryIdx for m in got] == list(wq) and [m.trainIdx for m in got] == list(wt)
    assert {(m.queryIdx, m.trainIdx, m.distance) for m in got} <= {(m.queryIdx, m.trainIdx, m.distance) for m in plain}
    assert len(set(got.query_idx)) == len(got) and len(set(got.train_idx)) == len(got)
    assert len(set(plain.train_idx)) < len(plain)            # (the plain matcher does hand one train to several queries)
    # the batched form the mirror path's static stereo uses, with an empty bucket
    many = fm.match_arrays_many([(q, t), (q[:0], t), (q[:40], t[:1])])
    assert np.array_equal(many[0][0], wq) and np.array_equal(many[0][1], wt) and len(many[1][0]) == 0
    assert np.array_equal(many[2][0], MUTUAL(q[:40], t[:1], None, None, None)[0]) and len(many[2][0]) == 1
    assert len(fm.match(q, t[:0])) == 0


# ---- 3 / 4. the pair path against refflow, and the one-call forms ---------------------------------------------------------
SETTINGS = {name: Setting(name, cc=name) for name in ("stereo", "f2f", "both")}
OFF = Setting("off")


@pytest.fixture(scope="module")
def pairs(ctx):
    """3 rendered pairs as in test_full_hot_path_from_images (GFT 330 features, one black frame): the front end on the GPU,
    the detection on the oracle (once, shared), one-mirror P3P with 500 fixed iterations."""
    return scenes.omni_pairs(ctx, B=3, black=(5,), solver=(("max_iter", 500),))


@pytest.fixture(scope="module")
def pipes(ctx, pairs):
    """The stage-by-stage pipeline per switch setting, run."""
    s, out = pairs, {}
    for name, setting in dict(SETTINGS, off=OFF).items():
        out[name] = pipe = FramePairPipeline(ctx, RigConfig(**s.rig_kw), s.B, frame_cap=2048, seed=s.seed, front_end=s.fe, **s.solver,
                                             cross_check_stereo=setting.cc_stereo, cross_check_f2f=setting.cc_f2f)
        pipe.stereo()
        pipe.track()
    ctx.synchronize()
    return out


def records(pipes, name):
    return pipes[name].results().cpu().numpy()


@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_pair_path_equals_refflow_with_the_mutual_matcher(ctx, pairs, pipes, name):
    s, setting = pairs, SETTINGS[name]
    st, ff = setting.cc_stereo, setting.cc_f2f
    pipe, rec = pipes[name], records(pipes, name)
    assert pipe.thr == s.thr
    frames, want = s.frames(setting), s.pair_tracks(setting)
    M, n_cand = pipe.frames["M"].cpu().numpy(), pipe.frames["n_cand"].cpu().numpy()
    assert [int(x) for x in M] == [len(fr["X"]) for fr in frames]
    assert [int(x) for x in n_cand] == [fr["n_cand"] for fr in frames]
    assert M[:5].min() > 100 and M[5] == 0
    mask = pipe.ransac["mask"].cpu().numpy()
    cq, ct = pipe.corr["q"].cpu().numpy(), pipe.corr["t"].cpu().numpy()
    for i, w in enumerate(want):
        n = len(w["corr"]["cam"])
        assert rec[i, 13] == n and np.array_equal(cq[i, :n], w["corr"]["q"]) and np.array_equal(ct[i, :n], w["corr"]["t"])
        assert rec[i, 14] == w["ransac"]["status"] and rec[i, 12] == w["ransac"]["n_inliers"]
        assert rec[i, 15] == w["ransac"]["best_iter"]
        assert np.array_equal(mask[i, :n].astype(bool), w["ransac"]["mask"])
        assert np.array_equal(rec[i, :12].reshape(3, 4), w["T"])
    assert rec[2, 14] == 1 and rec[2, 13] == 0 and (rec[:2, 14] == 0).all()
    off = records(pipes, "off")
    if ff:
        assert (rec[:2, 13] < off[:2, 13]).all()             # fewer correspondences than the plain matcher gives
    if st:
        assert (M[:5] < pipes["off"].frames["M"].cpu().numpy()[:5]).all()   # ... fewer stereo points
    if name == "both":
        assert not np.array_equal(rec[:2, :12], off[:2, :12])
    if name == "f2f":                                        # the stereo stage is untouched by the f2f switch
        assert np.array_equal(M, pipes["off"].frames["M"].cpu().numpy())


def test_pair_path_with_a_fraction_of_the_mutual_matches(ctx, pairs, pipes):
    """pct_good_matches = 0.75 with both switches: int(0.75 * len(matches)) counts the KEPT matches per bucket and per view
    (camera_models.py:3045, pose_est_tools.py:225), in the stage path and behind the one C call."""
    s = pairs
    rig_kw = dict(s.rig_kw, pct_good_matches=0.75)
    pipe = FramePairPipeline(ctx, RigConfig(**rig_kw), s.B, frame_cap=2048, seed=s.seed, front_end=s.fe, **s.solver,
                             cross_check_stereo=True, cross_check_f2f=True)
    pipe.stereo()
    pipe.track()
    rec = pipe.results().cpu().numpy()
    assert pipe.thr == s.thr
    frames, want = s.frames(SETTINGS["both"], pct=0.75), s.pair_tracks(SETTINGS["both"], pct=0.75)
    M, n_cand = pipe.frames["M"].cpu().numpy(), pipe.frames["n_cand"].cpu().numpy()
    assert [int(x) for x in M] == [len(fr["X"]) for fr in frames]
    assert [int(x) for x in n_cand] == [fr["n_cand"] for fr in frames]
    assert (n_cand[:5] < pipes["both"].frames["n_cand"].cpu().numpy()[:5]).all()
    mask = pipe.ransac["mask"].cpu().numpy()
    for i, w in enumerate(want):
        n = len(w["corr"]["cam"])
        assert rec[i, 13] == n and rec[i, 14] == w["ransac"]["status"] and rec[i, 12] == w["ransac"]["n_inliers"]
        assert np.array_equal(mask[i, :n].astype(bool), w["ransac"]["mask"])
        assert np.array_equal(rec[i, :12].reshape(3, 4), w["T"])
    batch = FramePairBatch(ctx, s.model, RigConfig(**rig_kw), s.B, num_of_features=s.nfeat, kp_cap=s.fe.kp_cap, frame_cap=2048,
                           seed=s.seed, **s.solver, cross_check_stereo=True, cross_check_f2f=True)
    batch.load_frames(s.omni)
    got = batch.step()
    ctx.synchronize()
    assert np.array_equal(got.cpu().numpy().view(np.uint64), rec.view(np.uint64))


@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_one_call_batches_give_the_pair_path_records(ctx, pairs, pipes, name):
    s, setting = pairs, SETTINGS[name]
    want = records(pipes, name)
    kw = dict(num_of_features=s.nfeat, kp_cap=s.fe.kp_cap, frame_cap=2048, seed=s.seed, **s.solver,
              cross_check_stereo=setting.cc_stereo, cross_check_f2f=setting.cc_f2f)
    sizes = {}
    for ns in (1, 2):
        batch = FramePairBatch(ctx, s.model, RigConfig(**s.rig_kw), s.B, n_streams=ns, **kw)
        sizes[ns] = batch.workspace.numel()
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
    off = FramePairBatch(ctx, s.model, RigConfig(**s.rig_kw), s.B, **dict(kw, cross_check_stereo=False, cross_check_f2f=False))
    assert off.workspace.numel() < sizes[1]                  # the workspace grows only with a switch set


def test_rgbd_pair_path_and_batch(ctx):
    """RGBDPairPipeline and RGBDPairBatch with cross_check=True on 2 pairs against refflow.track_pair_rgbd under the mutual
    matcher."""
    s, iters = scenes.rgbd_pairs(ctx), 300
    B, bgr, depth, cam, rc, frames = s.B, s.bgr, s.depth, s.cam, s.rc, s.frames
    kw = dict(num_of_features=s.nfeat, max_iter=iters, seed=31, pose_est_algorithm="EPNP")
    recs = {}
    for on in (False, True):
        pipe = RGBDPairPipeline(ctx, cam, B, cross_check=on, **kw)
        pipe.load_frames(bgr, depth)
        pipe.step()
        recs[on] = pipe.results().cpu().numpy()
        one = RGBDPairBatch(ctx, cam, B, cross_check=on, **kw)
        one.load_frames(bgr, depth)
        got = one.step()
        ctx.synchronize()
        assert np.array_equal(got.cpu().numpy().view(np.uint64), recs[on].view(np.uint64)), on
    rec, mask = recs[True], pipe.ransac["mask"].cpu().numpy()
    cq, ct = pipe.corr["q"].cpu().numpy(), pipe.corr["t"].cpu().numpy()
    want = [refflow.track_pair_rgbd(rc, frames[2 * i], frames[2 * i + 1], pipe.thr, iters, seed=31 + i, epnp=True, matching=MUTUAL)
            for i in range(B)]
    for i, w in enumerate(want):
        n = len(w["corr"]["q"])
        assert rec[i, 13] == n and np.array_equal(cq[i, :n], w["corr"]["q"]) and np.array_equal(ct[i, :n], w["corr"]["t"])
        assert rec[i, 14] == w["ransac"]["status"] == 0 and rec[i, 12] == w["ransac"]["n_inliers"]
        assert rec[i, 15] == w["ransac"]["best_iter"]
        assert np.array_equal(mask[i, :n].astype(bool), w["ransac"]["mask"])
        assert np.array_equal(rec[i, :12].reshape(3, 4), w["T"])
    assert (rec[:, 13] < recs[False][:, 13]).all() and (rec[:, 13] > 100).all()


# ---- 5. sequence mode ---------------------------------------------------------------------------------------------------------
def _rgbd_model():
    from vo_single_camera_sos_amd.omnistereo.camera_models import RGBDCamModel
    from vo_single_camera_sos_amd.omnistereo.transformations import rotation_matrix
    cam = RGBDCamModel(fx=FX, fy=FY, center_x=CX, center_y=CY, scaling_factor=1. / 1000.0, do_undistortion=False,
                       depth_is_Z=False, focal_length_m=1. / 1000.0)
    cam.T_Cest_wrt_Rgt = rotation_matrix(-np.pi / 2.0, [1, 0, 0])
    return cam


@pytest.fixture(scope="module")
def sos_sequences(tmp_path_factory):
    return scenes.write_sos_sequences(tmp_path_factory.mktemp("cross_check_sos"))


def test_run_vo_cross_check_windows_and_mirror_path(ctx, sos_sequences, tmp_path):
    from vo_single_camera_sos_amd.omnistereo.gum import load_gums_json
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO
    seq = sos_sequences[0]
    model = load_gums_json(os.path.join(seq, "gums-calibrated.json"))
    files, outs = scenes.run_vo_windows(model, seq, N_SEQ, tmp_path, (5, 1, 0), cross_check=True)
    assert files[5] == files[1] and "sequence_mode" in outs[5] and "sequence_mode" not in outs[0]
    for (i, Ta), (j, Tb) in zip(outs[0]["poses"], outs[5]["poses"]):
        assert i == j and np.allclose(Ta, Tb, rtol=1e-6, atol=1e-9), (i, np.abs(Ta - Tb).max())
    assert outs[0]["keyframe_ids"] == outs[5]["keyframe_ids"]
    res = str(tmp_path / "off")
    off = run_VO(None, model, frame_window=5, cross_check=False, **sos_kwargs(seq, N_SEQ, res))
    assert off["tracked"] == N_SEQ - 1 and read_results(res)[0] != files[5][0]
    # one matcher alone is a third result, and None is the tracker's own setting: off
    res = str(tmp_path / "f2f")
    run_VO(None, model, frame_window=5, cross_check="f2f", **sos_kwargs(seq, N_SEQ, res))
    assert read_results(res)[0] not in (files[5][0], read_results(str(tmp_path / "off"))[0])
    res = str(tmp_path / "none")
    run_VO(None, model, frame_window=5, **sos_kwargs(seq, N_SEQ, res))
    assert read_results(res) == read_results(str(tmp_path / "off"))


def test_run_vo_many_cross_check_equals_the_solo_runs(ctx, sos_sequences, tmp_path):
    gums = os.path.join(sos_sequences[0], "gums-calibrated.json")
    want, outs = scenes.run_vo_many_against_solo(gums, sos_sequences, N_SEQ, tmp_path, cross_check=True)
    assert all(o["sequence_mode"]["lanes"] == 2 for o in outs)
    assert want[0] != want[1]


def test_rgbd_run_vo_cross_check(ctx, tmp_path):
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO
    seq = str(tmp_path / "seq_rgbd")
    synthetic.write_rgbd_sequence(seq, n_frames=N_SEQ, seed=41, max_t=40.0, max_deg=2.0, depth_is_Z=False)
    model = _rgbd_model()
    files, outs = {}, {}
    for w in (5, 1, 0):
        res = str(tmp_path / ("w%d" % w))
        outs[w] = run_VO(None, model, frame_window=w, cross_check=True, **rgbd_kwargs(seq, N_SEQ, res))
        files[w] = read_results(res)
        assert outs[w]["tracked"] == N_SEQ - 1
    assert files[5] == files[1]
    for (i, Ta), (_, Tb) in zip(outs[5]["poses"], outs[0]["poses"]):
        assert np.allclose(Ta, Tb, rtol=1e-9, atol=1e-12), (i, np.abs(Ta - Tb).max())
    res = str(tmp_path / "off")
    run_VO(None, model, frame_window=5, **rgbd_kwargs(seq, N_SEQ, res))
    assert read_results(res)[0] != files[5][0]
    with pytest.raises(ValueError, match="no static-stereo matcher"):
        run_VO(None, model, frame_window=5, cross_check="stereo", **rgbd_kwargs(seq, N_SEQ, str(tmp_path / "bad")))


# ---- 6. what it is for ----------------------------------------------------------------------------------------------------------
def test_cross_check_raises_the_inlier_share_and_lowers_the_pose_error(ctx):
    """Six rendered pairs (seed 4100), GFT 1000 features, kp_cap 512, one-mirror P3P with 2000 fixed iterations, pipeline
    seed 11, LM 30, the reference's 5-degree threshold.  With both switches the summed inliers / summed correspondences is
    higher, and the mean rotation and the mean translation error over the six pairs are both lower, than with the switches
    off.  Relations, not thresholds; the CPU oracle flow gives 0.981 vs 0.913, 0.284 vs 0.602 degrees, 18.2 vs 25.2 mm, and
    the pair path equals that flow bit for bit (test_pair_path_equals_refflow_with_the_mutual_matcher)."""
    B = 6
    gs, rig_kw = scenes.rig()
    omni, poses = synthetic.make_frame_pairs(gs, B, seed=4100)
    model = DeviceImageModel(ctx, gs, (480, 640))
    fe = ImageFrontEnd(ctx, model, 2 * B, detection_method="GFT", num_of_features=1000, kp_cap=512)
    fe.load_frames(omni)
    fe.run()
    stats = {}
    for on in (False, True):
        pipe = FramePairPipeline(ctx, RigConfig(**rig_kw), B, frame_cap=2048, max_iter=2000, seed=11, front_end=fe,
                                 cross_check_stereo=on, cross_check_f2f=on)
        pipe.stereo()
        pipe.track()
        rec = pipe.results().cpu().numpy()
        assert (rec[:, 14] == 0).all()
        rot = [np.degrees(synth.pose_error(rec[i, :12].reshape(3, 4), R, t)[0]) for i, (R, t) in enumerate(poses)]
        trans = [np.linalg.norm(rec[i, 3:12:4] - t) for i, (R, t) in enumerate(poses)]
        stats[on] = (rec[:, 12].sum() / rec[:, 13].sum(), float(np.mean(rot)), float(np.mean(trans)), int(rec[:, 12].sum()),
                     int(rec[:, 13].sum()), [int(x) for x in pipe.frames["M"].cpu().numpy()[:2]])
        print("cross_check=%s: inliers / correspondences %d / %d = %.3f, mean rotation error %.3f deg, mean translation error "
              "%.1f mm, stereo points of frames 0, 1: %s" % (on, stats[on][3], stats[on][4], stats[on][0], stats[on][1],
                                                              stats[on][2], stats[on][5]))
    assert stats[True][0] > stats[False][0]
    assert stats[True][1] < stats[False][1]
    assert stats[True][2] < stats[False][2]
