"""What Lucas-Kanade tracking (run_VO(f2f_tracker="lk"), SOSVO_FLAG_LK_F2F) gives and costs in SEQUENCE MODE beside the
frame-to-frame matcher, measured in ONE process on the 256-frame synthetic sequence of bench.py's `sequence` sub-record
(seed 1234 + 7, panorama width 1440, the trackers' reference settings, frame_window 32).  Settings:
  match            the descriptor matcher (the default)
  match+ratio_f2f  ... with the ratio rule frame to frame at r = 48/64
  lk4+fb           the tracker, window half-size 4, 3 levels, max_iter 30, forward-backward check at 0.5 px
  lk10+fb          ... half-size 10
Every setting gets one untimed run (engine, scratch, first-use costs), then the settings ALTERNATE --reps times; the figure is
the median of a setting's runs by the host clock around run_VO (which ends in a synchronise).  One JSON line per setting,
appended to --out (default profiles/lk/bench_lk_sequence.jsonl): frames/s, per-hop rotation / translation error against the
planted trajectory, keyframes, serial tracking calls.  No thresholds.
  --window-trace: instead, push ONE window of 32 frames twice through a SequenceEngine with lk4+fb, promote a frame and copy
  it -- the workload of a `rocprofv3 --kernel-trace --stats` run for the times of the store's image kernels.
    python scripts/bench_lk_sequence.py [--frames 256] [--reps 7] [--render-workers 8] [--window-trace]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = {"match": {}, "match+ratio_f2f": dict(ratio_test="f2f", ratio=0.75),
            "lk4+fb": dict(f2f_tracker="lk", lk=dict(half=4, fb_max=0.5)), "lk10+fb": dict(f2f_tracker="lk", lk=dict(half=10, fb_max=0.5))}


def _gums(width, shape):
    from vo_single_camera_sos_amd.omnistereo.gum import synthetic_gums
    from vo_single_camera_sos_amd.omnistereo.panorama import Panorama
    gs = synthetic_gums()
    for m in (gs.top_model, gs.bot_model):
        m.panorama = Panorama(m, width=width)
    gs.make_annulus_masks(shape)
    return gs


def _hop_errors(poses, planted):
    from vo_single_camera_sos_amd.omnistereo import transformations as tr
    rot, tra = [], []
    for k in range(1, len(poses)):
        Tg = [np.identity(4), np.identity(4)]
        for j, q in enumerate((k - 1, k)):
            Tg[j][:3, :3], Tg[j][:3, 3] = planted[q][0], planted[q][1] * 1e-3
        E = tr.rpe(tr.concatenate_matrices(tr.inverse_matrix(Tg[0]), Tg[1]),
                   tr.concatenate_matrices(tr.inverse_matrix(poses[k - 1][1]), poses[k][1]))
        rot.append(np.degrees(tr.rpe_rotation_metric(E)))
        tra.append(1e3 * tr.rpe_translation_metric(E))
    return rot, tra


def window_trace(args, omni):
    import torch
    from vo_single_camera_sos_amd.frontend import DeviceImageModel
    from vo_single_camera_sos_amd.pipeline import RigConfig, SequenceEngine
    from vo_single_camera_sos_amd.runtime import default_context
    gs = _gums(args.pano_width, omni.shape[1:3])
    pano = gs.top_model.panorama
    geo = (pano.cols, pano.rows, pano.pixel_size, pano.cyl_height_max)
    rig = RigConfig(pano_top=geo, pano_bot=geo, F_top=gs.top_model.F[:3, 0], F_bot=gs.bot_model.F[:3, 0], min_range=500.0,
                    max_range=7000.0, f2f_max_hdiff=0.125 * 0.5 * pano.cols)
    ctx = default_context()
    eng = SequenceEngine(ctx, DeviceImageModel(ctx, gs, omni.shape[1:3]), rig, window=32, frame_cap=4096, **SETTINGS["lk4+fb"])
    for w0 in (0, 32):
        infos = eng.push_window(list(omni[w0:w0 + 32]))
        eng.promote(infos[5]["slot"])
        eng.track(eng.key_slot, infos[9]["slot"], 9)       # (flushes the promotion: one slot copy with its images)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--pano-width", type=int, default=1440)
    ap.add_argument("--render-workers", type=int, default=8)
    ap.add_argument("--window-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lk", "bench_lk_sequence.jsonl"))
    args = ap.parse_args()
    from vo_single_camera_sos_amd import synthetic
    omni, planted = synthetic.make_sequence(_gums(args.pano_width, (480, 640)), args.frames, seed=args.seed + 7,
                                            workers=args.render_workers)      # (rendered before the GPU is touched)
    if args.window_trace:
        return window_trace(args, omni)
    import torch
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO
    N = omni.shape[0]
    models = {name: _gums(args.pano_width, omni.shape[1:3]) for name in SETTINGS}      # (an engine per camera model)

    def frames(n=N):
        for k in range(n):
            yield k, omni[k], None
    runs, last = {name: [] for name in SETTINGS}, {}
    with tempfile.TemporaryDirectory() as d, contextlib.redirect_stdout(io.StringIO()):
        for name, kw in SETTINGS.items():
            run_VO(None, models[name], results_path=d, _live_frames=lambda: frames(min(N, 34)), frame_window=32, **kw)
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for name, kw in SETTINGS.items():
                t0 = time.perf_counter()
                last[name] = run_VO(None, models[name], results_path=d, _live_frames=frames, frame_window=32, **kw)
                torch.cuda.synchronize()
                runs[name].append(time.perf_counter() - t0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for name in SETTINGS:
            r, dts = last[name], sorted(runs[name])
            dt = dts[len(dts) // 2]
            rot, tra = _hop_errors(r["poses"], planted)
            rec = {"record": "sequence_256", "setting": name, "frames": N, "frame_window": 32, "reps": args.reps,
                   "frames_per_s": N / dt, "us_per_frame": 1e6 * dt / N, "runs_s": runs[name], "tracked": r["tracked"],
                   "keyframes": len(r["keyframe_ids"]), "serial_tracking_calls": r["sequence_mode"]["serial_tracking_calls"],
                   "gpu_windows_s": r["sequence_mode"]["stage_s"]["gpu_windows"],
                   "hop_rotation_deg": {"mean": float(np.mean(rot)), "median": float(np.median(rot)), "max": float(np.max(rot))},
                   "hop_translation_mm": {"mean": float(np.mean(tra)), "median": float(np.median(tra)), "max": float(np.max(tra))}}
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec))


if __name__ == "__main__":
    main()
