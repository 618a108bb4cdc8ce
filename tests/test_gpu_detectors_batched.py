"""GPU: ORB, FAST and AGAST behind the batch and sequence entry points (sosvo_batch_cfg.detector, the RGB-D flags bits
8-9), every assertion bit for bit:
  * sosvo_frame_pair_batch / _streams (1-3 streams) give the records of FramePairPipeline on ImageFrontEnd with the same
    detector (that path is pinned against the CPU oracle in test_gpu_endtoend.py), also through plain ctypes;
  * SequenceEngine's speculative records equal the pair batch's, and run_VO with detection_method="ORB" writes the same
    pose file for every frame window;
  * the RGB-D front end with ORB / FAST / AGAST equals the oracle flow (detection, descriptors, depth at the truncated
    pixel, back-projection), RGBDPairBatch equals RGBDPairPipeline, RGBDSequenceEngine equals RGBDPairBatch, run_VO's
    RGB-D pose file does not depend on the window and equals the per-frame path, and a planted motion is recovered;
  * degenerate inputs (flat image, empty mask, a mask without rows inside the 31-px border) give M = 0 and a failed
    track, with no fault."""
import ctypes
import os

import numpy as np
import pytest
import torch

import refflow
import synth
from matching_scenes import hop_records
from vo_single_camera_sos_amd import _lib, orb_pattern, synthetic
from vo_single_camera_sos_amd.frontend import DeviceImageModel, ImageFrontEnd
from vo_single_camera_sos_amd.omnistereo.gum import synthetic_gums
from vo_single_camera_sos_amd.omnistereo.panorama import Panorama
from vo_single_camera_sos_amd.pipeline import (FramePairBatch, FramePairPipeline, RGBDCamConfig, RGBDFrontEnd,
                                               RGBDPairBatch, RGBDPairPipeline, RGBDSequenceEngine, RigConfig,
                                               SequenceEngine)

pytestmark = pytest.mark.gpu

METHODS = ("ORB", "FAST", "AGAST")
FX = FY = 554.256258
CX, CY = 319.5, 239.5


def _gums():
    gs = synthetic_gums()
    for m in (gs.top_model, gs.bot_model):
        m.panorama = Panorama(m, width=1200)
    gs.make_annulus_masks((480, 640))
    pano = gs.top_model.panorama
    geo = (pano.cols, pano.rows, pano.pixel_size, pano.cyl_height_max)
    rig_kw = dict(pano_top=geo, pano_bot=geo, F_top=gs.top_model.F[:3, 0], F_bot=gs.bot_model.F[:3, 0], min_range=500.0,
                  max_range=7000.0, stereo_min_disp=1.0, stereo_max_hdiff=2.5, f2f_max_hdiff=0.125 * 0.5 * pano.cols,
                  pct_good_matches=1.0)
    return gs, rig_kw


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("method", METHODS)
def test_pair_batch_equals_the_stage_sequence(ctx, method):
    B, nfeat = 3, 250
    gs, rig_kw = _gums()
    model = DeviceImageModel(ctx, gs, (480, 640))
    omni, _ = synthetic.make_frame_pairs(gs, B, seed=4242)
    omni[5] = 0                                                   # pair 2: black current frame
    fe = ImageFrontEnd(ctx, model, 2 * B, detection_method=method, num_of_features=nfeat, keep_panoramas=False)
    pipe = FramePairPipeline(ctx, RigConfig(**rig_kw), B, frame_cap=1024, max_iter=300, seed=11, front_end=fe)
    fe.load_frames(omni)
    pipe.step()
    want = pipe.results().cpu().numpy()
    assert (want[:2, 13] > 0).all() and want[2, 14] == 1 and want[2, 13] == 0, want[:, 12:]
    for ns in (1, 2, 3):
        batch = FramePairBatch(ctx, model, RigConfig(**rig_kw), B, num_of_features=nfeat, frame_cap=1024, max_iter=300, seed=11,
                               n_streams=ns, detection_method=method)
        assert batch.cfg.detector == _lib.DETECTORS[method] and batch.cfg.kp_cap == fe.kp_cap
        batch.workspace.fill_(0xA5)
        batch.load_frames(omni)
        for _ in range(2):                                        # a second step on the dirty workspace: the same records
            got = batch.step().cpu().numpy()
            assert np.array_equal(_bits(got), _bits(want)), (method, ns, got[:, 12:], want[:, 12:])
    if method == "ORB":   # the enqueue form over three streams, two calls before the join
        multi = FramePairBatch(ctx, model, RigConfig(**rig_kw), B, num_of_features=nfeat, frame_cap=1024, max_iter=300, seed=11,
                               n_streams=3, detection_method=method)
        multi.load_frames(omni)
        bufs = [torch.zeros_like(multi.out), torch.zeros_like(multi.out)]
        multi.enqueue(bufs[0])
        multi.enqueue(bufs[1])
        multi.join()
        ctx.synchronize()
        for b in bufs:
            assert np.array_equal(_bits(b.cpu().numpy()), _bits(want))


def test_plain_ctypes_call_with_the_detector_field(ctx):
    """The C caller's view (examples/c_abi_batch.c): sosvo_frame_pair_batch called straight through ctypes, no engine, with
    `detector` = ORB; the ORB workspace is larger than GFT's; an unknown detector or an ORB kp_cap above 2048 is refused."""
    B, nfeat = 2, 250
    gs, rig_kw = _gums()
    model = DeviceImageModel(ctx, gs, (480, 640))
    omni, _ = synthetic.make_frame_pairs(gs, B, seed=99)
    ref = FramePairBatch(ctx, model, RigConfig(**rig_kw), B, num_of_features=nfeat, frame_cap=1024, max_iter=300, seed=3,
                         detection_method="ORB")
    ref.load_frames(omni)
    want = ref.step().cpu().numpy()
    lib = _lib.load()
    c = _lib.BatchCfg()
    ctypes.memmove(ctypes.addressof(c), ctypes.addressof(ref.cfg), ctypes.sizeof(c))
    assert c.detector == _lib.DETECTOR_ORB
    nbytes = lib.sosvo_frame_pair_batch_workspace(ctypes.byref(c))
    c0 = _lib.BatchCfg()
    ctypes.memmove(ctypes.addressof(c0), ctypes.addressof(c), ctypes.sizeof(c))
    c0.detector = _lib.DETECTOR_GFT
    assert nbytes > lib.sosvo_frame_pair_batch_workspace(ctypes.byref(c0)) > 0
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=ctx.device)
    out = torch.zeros((B, 16), dtype=torch.float64, device=ctx.device)
    dev_omni = torch.from_numpy(omni).to(ctx.device)
    rig = RigConfig(**rig_kw).as_struct()
    ctx.synchronize()
    rc = lib.sosvo_frame_pair_batch(ctx._h, ctypes.byref(rig), ctypes.byref(c), dev_omni.data_ptr(),
                                    model.unwrap_table.data_ptr(), model.mask_bits.data_ptr(), model.pattern.data_ptr(),
                                    ws.data_ptr(), nbytes, out.data_ptr())
    assert rc == 0
    ctx.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    for bad_det, cap in ((4, c.kp_cap), (-1, c.kp_cap), (_lib.DETECTOR_ORB, 2112)):
        c.detector, c.kp_cap = bad_det, cap
        assert lib.sosvo_frame_pair_batch_workspace(ctypes.byref(c)) == 0
        assert lib.sosvo_frame_pair_batch(ctx._h, ctypes.byref(rig), ctypes.byref(c), dev_omni.data_ptr(),
                                          model.unwrap_table.data_ptr(), model.mask_bits.data_ptr(), model.pattern.data_ptr(),
                                          ws.data_ptr(), nbytes, out.data_ptr()) == -1   # SOSVO_ERR_ARG


def _sequence_frames(gs, n, seed):
    room = synthetic.Room(seed=seed)
    poses = synthetic.trajectory(n, seed, max_t=40.0, max_deg=2.0)
    rng = np.random.default_rng(seed + 1)
    return np.stack([synthetic.render_omni(gs, room, R, t, 2.0, rng) for R, t in poses])


@pytest.mark.parametrize("method", METHODS)
def test_sequence_engine_equals_the_pair_batch(ctx, method):
    gs, rig_kw = _gums()
    n = 6
    frames = _sequence_frames(gs, n, seed=61)
    model = DeviceImageModel(ctx, gs, (480, 640))
    kw = dict(num_of_features=1000, kp_cap=(1280 if method == "ORB" else 1024), frame_cap=2048, max_iter=210, adaptive=True,
              ransac_solver="GP3P", detection_method=method)
    want = []
    for t in range(1, n):
        pb = FramePairBatch(ctx, model, RigConfig(**rig_kw), 1, seed=t - 1, **kw)
        pb.load_frames(frames[t - 1:t + 1])
        want.append(pb.step().cpu().numpy()[0].copy())
    want = np.stack(want)
    # consecutive frames of the synthetic sequence track with every detector (n_inliers, n_correspondences, status)
    assert (want[:, 14] == 0).all() and (want[:, 12] >= 6).all(), (method, want[:, 12:16])
    for window in (1, 4, 6):
        eng = SequenceEngine(ctx, model, RigConfig(**rig_kw), window=window, **kw)
        assert eng.cfg.detector == _lib.DETECTORS[method]
        got = hop_records(eng, frames, window)
        assert np.array_equal(_bits(got), _bits(want)), (method, window)


def test_run_vo_with_orb_does_not_depend_on_the_frame_window(ctx, tmp_path):
    """run_VO(detection_method="ORB") in sequence mode: byte-identical pose and keyframe files for windows 32, 5 and 1; the
    per-frame mirror path (window 0) runs the same detector and agrees to rounding, as for GFT (test_gpu_sequence.py)."""
    import demo_vo_sos
    gs, _ = _gums()
    n = 40
    seq = str(tmp_path / "seq_orb")
    synthetic.write_sos_sequence(seq, gs, n_frames=n, seed=77, max_t=40.0, max_deg=2.0)
    gums = os.path.join(seq, "gums-calibrated.json")
    res = os.path.join(seq, "results-omni")
    outs, texts = {}, {}
    for w in (32, 5, 1, 0):
        outs[w] = demo_vo_sos.main_sos_vo([seq, "--calibrated_gums_file", gums, "--frame_window", str(w),
                                           "--detection_method", "ORB"])
        texts[w] = (open(os.path.join(res, "estimated_frame_poses_TUM.txt")).read(),
                    open(os.path.join(res, "keyframe_ids.txt")).read())
    for w in (32, 5, 1):
        assert outs[w]["sequence_mode"]["frame_window"] == w and outs[w]["tracked"] == outs[32]["tracked"], w
    assert "sequence_mode" not in outs[0]
    assert texts[32] == texts[5] == texts[1]
    assert outs[32]["tracked"] == n - 1 and len(texts[32][0].splitlines()) == n
    for (i, Ta), (j, Tb) in zip(outs[0]["poses"], outs[32]["poses"]):
        assert i == j and np.allclose(Ta, Tb, rtol=1e-6, atol=1e-9), (i, np.abs(Ta - Tb).max())
    # the engine the run used is the ORB one (the cache key carries the method); a GFT run on the same model gets its own
    eng = outs[32]["sequence_mode"]
    assert eng["windows"] == -(-n // 32)
    gft = demo_vo_sos.main_sos_vo([seq, "--calibrated_gums_file", gums, "--frame_window", "32"])
    assert gft["tracked"] == n - 1 and open(os.path.join(res, "estimated_frame_poses_TUM.txt")).read() != texts[32][0]


# ---- RGB-D -----------------------------------------------------------------------------------------------------------
YAW = np.deg2rad(40.0)
R_YAW = np.array([[np.cos(YAW), -np.sin(YAW), 0.0], [np.sin(YAW), np.cos(YAW), 0.0], [0.0, 0.0, 1.0]])


def _rgbd_pairs(B, seed0=900):
    bgr, depth, poses = [], [], []
    for i in range(B):
        rng = np.random.default_rng(seed0 + i)
        room = synthetic.Room(seed=seed0 + i, half_x=(1800.0, 2600.0), half_y=(2500.0, 3500.0), cells=(150.0, 40.0))
        R, t = synthetic.random_step(rng, max_t=80.0, max_deg=8.0)
        for (Rw, tw) in ((R_YAW, np.zeros(3)), (R_YAW @ R, R_YAW @ t)):
            im, dp = synthetic.render_rgbd(room, Rw, tw, rng, FX, FY, CX, CY, depth_is_Z=True)
            bgr.append(im)
            depth.append(dp)
        poses.append((R, t))
    return np.stack(bgr), np.stack(depth), poses


@pytest.mark.parametrize("method", METHODS)
def test_rgbd_front_end_equals_the_oracle_and_the_batched_paths(ctx, method):
    B, nfeat = 2, 1000
    bgr, depth, poses = _rgbd_pairs(B)
    cam = RGBDCamConfig(fx=FX, fy=FY, center_x=CX, center_y=CY, depth_is_Z=True, min_range=0.8, max_range=7.0)
    thr = 1.0 - np.cos(np.deg2rad(0.5))
    # (AGAST on an 11x11 median: the unfiltered 640x480 texture has more than the 16384 FAST corners per image
    # sosvo_detect_agast holds before its suppression, status bit 1)
    med = 11 if method == "AGAST" else 0
    pipe = RGBDPairPipeline(ctx, cam, B, num_of_features=nfeat, max_iter=400, seed=31, thr=thr, detection_method=method,
                            median_win_size=med)
    fe = pipe.front_end
    assert fe.method == method
    pipe.load_frames(bgr, depth)
    pipe.step()
    rec = pipe.results().cpu().numpy()
    g = {k: v.cpu().numpy() for k, v in pipe.frames.items()}
    n_kp = pipe.n.cpu().numpy()
    # (bit 0, more corners than kp_cap, is exact: the first kp_cap in raster order are kept, as the oracle flow keeps them)
    assert not (pipe.status.cpu().numpy() & 2).any(), (method, pipe.status.cpu().numpy())
    if method == "ORB":
        assert not np.isnan(fe.kp4.cpu().numpy()).any()
    rc = refflow.RGBDParams(FX, FY, CX, CY, cam.focal_length_m, True, cam.min_range, cam.max_range)
    ca, sa = orb_pattern.angle_cos_sin(orb_pattern.GFT_KEYPOINT_ANGLE)
    pat = orb_pattern.orb_pattern()
    for f in range(2 * B):
        w = refflow.rgbd_frame(rc, bgr[f], depth[f], nfeat, pat, ca, sa, median_ksize=med, method=method, kp_cap=fe.kp_cap)
        M = int(g["M"][f])
        assert n_kp[f] == w["n_kp"] and M == len(w["X"]), (method, f, n_kp[f], w["n_kp"], M, len(w["X"]))
        assert np.array_equal(g["m"][f, :M], w["m"]) and np.array_equal(g["d"][f, :M], w["d"]), (method, f)
        assert np.array_equal(g["X"][f, :M], w["X"]) and np.array_equal(g["b"][f, :M], w["b"]), (method, f)
        assert M > 100, (method, f, M)
    if method == "ORB":   # ORB's upper-level keypoints have fractional coordinates: the depth pixel is the truncated one
        m = g["m"][0, :int(g["M"][0])]
        assert (m != np.floor(m)).any()
    # the planted motion is recovered (0.5-degree threshold; the loose bound of test_gpu_rgbd.py): pose of the current camera
    # in the reference camera frame, metres
    C = np.array([[1.0, 0, 0], [0, 0, 1.0], [0, -1.0, 0]])
    for i, (R, t) in enumerate(poses):
        assert rec[i, 14] == 0 and rec[i, 12] >= 20, (method, rec[i, 12:])
        T = rec[i, :12].reshape(3, 4)
        ang, _ = synth.pose_error(T, C.T @ R @ C, C.T @ t * 1e-3)
        assert ang < np.deg2rad(1.0) and np.linalg.norm(T[:, 3] - C.T @ t * 1e-3) < 0.05, (method, i, ang, T[:, 3])
    one = RGBDPairBatch(ctx, cam, B, num_of_features=nfeat, max_iter=400, seed=31, thr=thr, detection_method=method,
                        median_win_size=med)
    assert one.cfg.flags >> 8 == _lib.DETECTORS[method] and one.cfg.kp_cap == fe.kp_cap
    one.workspace.fill_(0x5A)
    one.load_frames(bgr, depth)
    got = one.step().cpu().numpy()
    assert np.array_equal(_bits(got), _bits(rec)), (method, got[:, 12:], rec[:, 12:])


@pytest.mark.parametrize("method", METHODS)
def test_rgbd_sequence_engine_and_run_vo(ctx, tmp_path, method):
    import demo_vo_rgbd
    from vo_single_camera_sos_amd.omnistereo.common_cv import get_depthmap_float32_from_png, get_images, imread
    n = 10
    seq = str(tmp_path / ("seq_rgbd_" + method))
    synthetic.write_rgbd_sequence(seq, n_frames=n, seed=41, max_t=40.0, max_deg=2.0, depth_is_Z=False)
    names = get_images(os.path.join(seq, "rgbd", "rgb", "*.png"), indices_list=None, return_names_only=True)
    dnames = get_images(os.path.join(seq, "rgbd", "depth", "*.png"), indices_list=None, return_names_only=True)
    bgr = np.stack([np.ascontiguousarray(imread(f)[..., ::-1]) for f in names])
    depth = np.stack([get_depthmap_float32_from_png(f, 1.0 / 1000.0) for f in dnames])
    cam = RGBDCamConfig(fx=FX, fy=FY, center_x=CX, center_y=CY, depth_is_Z=False, min_range=0.8, max_range=7.0)
    kw = dict(num_of_features=1000, max_iter=210, adaptive=True, pose_est_algorithm="EPNP", detection_method=method)
    want = []
    for t in range(1, 5):
        pb = RGBDPairBatch(ctx, cam, 1, seed=t - 1, **kw)
        pb.load_frames(bgr[t - 1:t + 1], depth[t - 1:t + 1])
        want.append(pb.step().cpu().numpy()[0].copy())
    want = np.stack(want)
    assert (want[:, 14] == 0).all() and (want[:, 12] >= 20).all(), (method, want[:, 12:16])
    for window in (1, 3, 5):
        eng = RGBDSequenceEngine(ctx, cam, window=window, **kw)
        got = hop_records(eng, list(zip(bgr[:5], depth[:5])), window)
        assert np.array_equal(_bits(got), _bits(want)), (method, window)
    outs, texts = {}, {}
    for w in (8, 1, 0):
        outs[w] = demo_vo_rgbd.main_rgbd_vo([seq, "--is_synthetic", "true", "--frame_window", str(w), "--detection_method",
                                             method])
        assert outs[w]["tracked"] == n - 1, (method, w, outs[w]["tracked"])
        texts[w] = open(os.path.join(seq, "results-rgbd", "estimated_frame_poses_TUM.txt")).read()
    assert texts[8] == texts[1] and "sequence_mode" in outs[8] and "sequence_mode" not in outs[0]
    for (i, Ta), (_, Tb) in zip(outs[8]["poses"], outs[0]["poses"]):
        assert np.allclose(Ta, Tb, rtol=1e-9, atol=1e-12), (method, i, np.abs(Ta - Tb).max())


def test_degenerate_inputs_with_orb(ctx):
    """A flat image (no keypoints), a mask with no pixel set, a mask whose only rows lie within the 31-px border: M = 0 and
    a failed-track record (status 1, no correspondences) from the pair batch, the per-frame front end and the SOS batch."""
    rows, cols = 480, 640
    bgr, depth, _ = _rgbd_pairs(1)
    cam = RGBDCamConfig(fx=FX, fy=FY, center_x=CX, center_y=CY, depth_is_Z=True, min_range=0.8, max_range=7.0)
    flat = np.full_like(bgr, 128)
    border = np.zeros((rows, cols), np.uint8)
    border[:20] = 1
    border[-20:] = 1
    cases = [("flat", flat, None), ("empty_mask", bgr, np.zeros((rows, cols), np.uint8)), ("border_mask", bgr, border)]
    for name, images, mask in cases:
        fe = RGBDFrontEnd(ctx, cam, 2, num_of_features=500, mask=mask, detection_method="ORB")
        fe.load_frames(images, depth)
        fe.run()
        ctx.synchronize()
        assert (fe.frames["M"].cpu().numpy() == 0).all(), name
        one = RGBDPairBatch(ctx, cam, 1, num_of_features=500, mask=mask, detection_method="ORB")
        one.load_frames(images, depth)
        rec = one.step().cpu().numpy()
        assert rec[0, 13] == 0 and rec[0, 14] == 1 and rec[0, 12] == 0, (name, rec)
    gs, rig_kw = _gums()
    model = DeviceImageModel(ctx, gs, (480, 640))
    batch = FramePairBatch(ctx, model, RigConfig(**rig_kw), 1, num_of_features=250, frame_cap=1024, max_iter=300,
                           detection_method="ORB")
    batch.load_frames(np.full((2, 480, 640, 3), 77, np.uint8))
    rec = batch.step().cpu().numpy()
    assert rec[0, 13] == 0 and rec[0, 14] == 1, rec
