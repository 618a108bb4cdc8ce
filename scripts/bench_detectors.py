"""Throughput per keypoint detector (GFT, ORB, FAST, AGAST) of the paths that take one:
  pairs      sosvo_frame_pair_batch_streams (C2 setting: 1440-px panoramas, 12 masks, 1000 features per mask) and
             sosvo_rgbd_pair_batch (C5 setting: 640x480, 2000 features, 2000 RANSAC iterations, EPNP), pairs/s
  sequence   the demos' run_VO on a synthetic sequence written to disk (SOS: 256 frames, RGB-D: 128 frames) in sequence mode
             (frame_window 32) and on the per-frame mirror path (frame_window 0), frames/s (wall clock of the whole run: PNG
             decoding and result files included, so host-bound; bench.py's `sequence` record times in-memory frames)
One JSON line per (path, detector).
    python scripts/bench_detectors.py [--pairs 64] [--rgbd-pairs 32] [--sos-frames 256] [--rgbd-frames 128] [--only pairs|sequence]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

METHODS = ("GFT", "ORB", "FAST", "AGAST")


def timed(fn, sync, warmup=2, steps=5):
    for _ in range(warmup):
        fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    sync()
    return (time.perf_counter() - t0) / steps


def bench_pairs(args):
    from vo_single_camera_sos_amd import synthetic
    from vo_single_camera_sos_amd.device import Context
    from vo_single_camera_sos_amd.frontend import DeviceImageModel
    from vo_single_camera_sos_amd.omnistereo.gum import synthetic_gums
    from vo_single_camera_sos_amd.omnistereo.panorama import Panorama
    from vo_single_camera_sos_amd.pipeline import FramePairBatch, RGBDCamConfig, RGBDPairBatch, RigConfig
    gs = synthetic_gums()
    for m in (gs.top_model, gs.bot_model):
        m.panorama = Panorama(m, width=1440)
    gs.make_annulus_masks((480, 640))
    omni, _ = synthetic.make_frame_pairs(gs, args.pairs, seed=1)
    B5 = args.rgbd_pairs
    bgr, depth = [], []
    for i in range(B5):
        rng = np.random.default_rng(900 + i)
        room = synthetic.Room(seed=900 + i, half_x=(1800.0, 2600.0), half_y=(2500.0, 3500.0), cells=(150.0, 40.0), yaw_deg=40.0)
        R, t = synthetic.random_step(rng, max_t=80.0, max_deg=8.0)
        for (Rw, tw) in ((np.eye(3), np.zeros(3)), (R, t)):
            im, dp = synthetic.render_rgbd(room, Rw, tw, rng, depth_is_Z=True)
            bgr.append(im)
            depth.append(dp)
    bgr, depth = np.stack(bgr), np.stack(depth)
    ctx = Context(0)
    pano = gs.top_model.panorama
    geo = (pano.cols, pano.rows, pano.pixel_size, pano.cyl_height_max)
    rig = RigConfig(pano_top=geo, pano_bot=geo, F_top=gs.top_model.F[:3, 0], F_bot=gs.bot_model.F[:3, 0], min_range=500.0,
                    max_range=7000.0)
    model = DeviceImageModel(ctx, gs, (480, 640))
    cam = RGBDCamConfig(fx=554.256258, fy=554.256258, center_x=319.5, center_y=239.5, depth_is_Z=True, min_range=0.8, max_range=7.0)
    for method in METHODS:
        eng = FramePairBatch(ctx, model, rig, args.pairs, num_of_features=1000, frame_cap=2048, max_iter=2000, n_streams=2,
                             detection_method=method)
        eng.load_frames(omni)
        dt = timed(eng.step, ctx.synchronize)
        rec = eng.results().cpu().numpy()
        print(json.dumps({"path": "C2 pair batch (sosvo_frame_pair_batch_streams, 2 streams)", "detector": method,
                          "pairs": args.pairs, "kp_cap": int(eng.cfg.kp_cap), "pairs_per_s": round(args.pairs / dt, 1),
                          "median_inliers": float(np.median(rec[:, 12])), "tracked": int((rec[:, 14] == 0).sum())}), flush=True)
        del eng
        one = RGBDPairBatch(ctx, cam, B5, num_of_features=2000, max_iter=2000, seed=1, pose_est_algorithm="EPNP",
                            detection_method=method)
        one.load_frames(bgr, depth)
        dt = timed(one.step, ctx.synchronize)
        rec = one.results().cpu().numpy()
        print(json.dumps({"path": "C5 RGB-D pair batch (sosvo_rgbd_pair_batch)", "detector": method, "pairs": B5,
                          "kp_cap": int(one.cfg.kp_cap), "pairs_per_s": round(B5 / dt, 1),
                          "median_inliers": float(np.median(rec[:, 12])), "tracked": int((rec[:, 14] == 0).sum())}), flush=True)
        del one
    ctx.close()


def bench_sequence(args):
    import demo_vo_rgbd
    import demo_vo_sos
    from vo_single_camera_sos_amd import synthetic
    from vo_single_camera_sos_amd.omnistereo.gum import synthetic_gums
    from vo_single_camera_sos_amd.omnistereo.panorama import Panorama
    tmp = tempfile.mkdtemp(prefix="bench_detectors_")
    gs = synthetic_gums()
    for m in (gs.top_model, gs.bot_model):
        m.panorama = Panorama(m, width=1200)
    gs.make_annulus_masks((480, 640))
    sos = os.path.join(tmp, "sos")
    synthetic.write_sos_sequence(sos, gs, n_frames=args.sos_frames, seed=77, max_t=40.0, max_deg=2.0)
    rgbd = os.path.join(tmp, "rgbd")
    synthetic.write_rgbd_sequence(rgbd, n_frames=args.rgbd_frames, seed=41, max_t=40.0, max_deg=2.0, depth_is_Z=False)
    runs = [("SOS", args.sos_frames, lambda w, m: demo_vo_sos.main_sos_vo(
                [sos, "--calibrated_gums_file", os.path.join(sos, "gums-calibrated.json"), "--frame_window", str(w),
                 "--detection_method", m, "--use_multithreads_for_VO", "false"])),
            ("RGB-D", args.rgbd_frames, lambda w, m: demo_vo_rgbd.main_rgbd_vo(
                [rgbd, "--is_synthetic", "true", "--frame_window", str(w), "--detection_method", m,
                 "--use_multithreads_for_VO", "false"]))]
    for name, n, run in runs:
        for method in METHODS:
            rates = {}
            for w in (32, 0):
                run(w, method)                       # warm-up: engine, front ends, kernels
                t0 = time.perf_counter()
                out = run(w, method)
                rates[w] = (n / (time.perf_counter() - t0), int(out["tracked"]))
            print(json.dumps({"path": "%s run_VO" % name, "detector": method, "frames": n,
                              "sequence_mode_frames_per_s": round(rates[32][0], 1), "sequence_mode_tracked": rates[32][1],
                              "per_frame_frames_per_s": round(rates[0][0], 1), "per_frame_tracked": rates[0][1]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--rgbd-pairs", type=int, default=32)
    ap.add_argument("--sos-frames", type=int, default=256)
    ap.add_argument("--rgbd-frames", type=int, default=128)
    ap.add_argument("--only", default="", choices=("", "pairs", "sequence"))
    args = ap.parse_args()
    if args.only != "sequence":
        bench_pairs(args)
    if args.only != "pairs":
        bench_sequence(args)


if __name__ == "__main__":
    main()
