"""What the seam-free front end gives and costs, measured in ONE process with the settings alternating.
Records (one JSON line each, appended to --out, default profiles/seam_free/bench_seam_free.jsonl; no thresholds):
  accuracy   FramePairPipeline per setting (the matcher; LK half 4 and half 10, 3 levels, max_iter 30, forward-backward 0.5 px)
             and per set of rendered pairs at 1200 columns, GFT 1000 features, one-mirror P3P with 2000 iterations -- `six` =
             the six pairs of tests/test_gpu_cross_check.py (seed 4100, no deliberate yaw), `yaw5` / `yaw10` / `yaw20` = six
             rooms each, the second frame turned by +/- that angle about the vertical axis and moved by up to 40 mm -- with
             cyclic_columns False, True and "seam_free": stereo points per frame (and how many of them lie within 31 columns
             of the seam), correspondences, crossings (pairs whose two columns lie more than half a panorama apart), inlier
             share, rotation / translation error
  step       the headline step (OverlappedFramePairs, --pairs pairs at --cols columns, 3 streams) with cyclic_columns=True and
             "seam_free", alternating, wall time of a step with the device synchronised, median of --reps
  kernels    one --pairs step of FramePairBatch on one stream under the library's per-kernel event profile, with the matcher
             and with LK half 4 (the store's padded level-0 fill), for True and "seam_free": the milliseconds of every kernel,
             summed by name, and the seam_free / True ratio per kernel
  gray_unpad sosvo_gray_unpad on the 4 * pairs gray panoramas of a step, on its own (HIP events around the call)
  run_vo     run_VO(frame_window=32) on a rendered --vo-frames sequence with cyclic_columns=True and "seam_free", alternating,
             wall time, median of --reps
Each time is taken after one warm-up call.
    python scripts/bench_seam_free.py [--only accuracy|step|kernels|run_vo] [--pairs 256] [--cols 1440] [--reps 7] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

FB = 0.5
SETTINGS = {"match": {}, "lk4+fb": dict(f2f_tracker="lk", lk=dict(half=4, fb_max=FB)), "lk10+fb": dict(f2f_tracker="lk", lk=dict(half=10, fb_max=FB))}
COLUMNS = (False, True, "seam_free")


def _crossings(pipe, cols):
    """Correspondences whose reference and current columns lie more than half a panorama apart."""
    co = {k: v.cpu().numpy() for k, v in pipe.corr.items()}
    m = [pipe.frames["m_top"].cpu().numpy(), pipe.frames["m_bot"].cpu().numpy()]
    trk = pipe._lk_out[0].cpu().numpy() if pipe.lk is not None else None
    total = 0
    for i in range(pipe.B):
        n = int(co["n"][i])
        cam, t, q = co["cam"][i, :n], co["t"][i, :n], co["q"][i, :n]
        u_ref = np.array([m[c][2 * i, k, 0] for c, k in zip(cam, t)], np.float64)
        if trk is None:
            u_cur = np.array([m[c][2 * i + 1, k, 0] for c, k in zip(cam, q)], np.float64)
        else:
            u_cur = np.array([trk[c * pipe.B + i, k, 0] for c, k in zip(cam, t)], np.float64)
        total += int((np.abs(u_cur - u_ref) > cols / 2).sum())
    return total


def bench_accuracy(emit):
    import bench_gated_matching as gated
    from bench_cross_check import _rig
    from bench_cyclic import _yaw_pairs
    from vo_single_camera_sos_amd import synthetic
    from vo_single_camera_sos_amd.frontend import DeviceImageModel, ImageFrontEnd
    from vo_single_camera_sos_amd.pipeline import FramePairPipeline, RigConfig
    from vo_single_camera_sos_amd.runtime import default_context
    gs, rig_kw = _rig(1200)
    sets = {"six": synthetic.make_frame_pairs(gs, 6, seed=4100)}          # (rendered before the GPU is touched)
    for yaw in (5, 10, 20):
        sets["yaw%d" % yaw] = _yaw_pairs(gs, float(yaw), 6, 4200 + yaw)
    ctx = default_context()
    model = DeviceImageModel(ctx, gs, (480, 640))
    cols = model.cols
    for name, (omni, poses) in sets.items():
        B = len(poses)
        fes = {sf: ImageFrontEnd(ctx, model.seam_free_form(ctx) if sf else model, 2 * B, detection_method="GFT", num_of_features=1000,
                                 kp_cap=512, keep_panoramas=False) for sf in (False, True)}
        for fe in fes.values():
            fe.load_frames(omni)
        for setting, kw in SETTINGS.items():
            for value in COLUMNS:
                pipe = FramePairPipeline(ctx, RigConfig(**rig_kw), B, frame_cap=2048, max_iter=2000, seed=11,
                                         front_end=fes[value == "seam_free"], cyclic_columns=value, **kw)
                pipe.step()
                ctx.synchronize()
                M = pipe.frames["M"].cpu().numpy()
                x = np.concatenate([pipe.frames["m_top"][f, :M[f]].cpu().numpy()[:, 0] for f in range(2 * B)])
                out = {"record": "accuracy", "pairs_set": name, "setting": setting, "cyclic_columns": value}
                out.update(gated._accuracy(pipe.results().cpu().numpy(), poses, M))
                out.update(stereo_points_in_the_bands_per_frame=round(float(((x < 31) | (x >= cols - 31)).sum()) / (2 * B), 1),
                           crossings=_crossings(pipe, cols))
                emit(out)


def _rig_at(cols):
    from bench_cross_check import _rig
    return _rig(cols)


def bench_step(args, emit):
    import torch
    from vo_single_camera_sos_amd import synthetic
    from vo_single_camera_sos_amd.pipeline import OverlappedFramePairs, RigConfig
    gs, rig_kw = _rig_at(args.cols)
    few, _ = synthetic.make_frame_pairs(gs, 8, seed=1234)
    omni = np.concatenate([few] * (args.pairs // 8))                     # (distinct content per 8 pairs is enough for timing)
    engines = {}
    for value in (True, "seam_free"):
        e = OverlappedFramePairs(0, gs, (480, 640), RigConfig(**rig_kw), args.pairs, n_streams=3, num_of_features=1000, kp_cap=512,
                                 frame_cap=2048, max_iter=2000, seed=1234, cyclic_columns=value)
        e.load_frames(omni)
        e.step()
        e.results()
        torch.cuda.synchronize()
        engines[value] = e
    times = {True: [], "seam_free": []}
    for _ in range(args.reps):
        for value, e in engines.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.step()
            e.results()
            torch.cuda.synchronize()
            times[value].append((time.perf_counter() - t0) * 1e3)
    a, b = float(np.median(times[True])), float(np.median(times["seam_free"]))
    emit(dict(record="step", pairs=args.pairs, cols=args.cols, streams=3, reps=args.reps, cyclic_ms=round(a, 3), seam_free_ms=round(b, 3),
              seam_free_over_cyclic=round(b / a, 4), cyclic_all_ms=[round(t, 3) for t in times[True]],
              seam_free_all_ms=[round(t, 3) for t in times["seam_free"]],
              expected_from_the_columns=round((args.cols + 80) / args.cols, 4)))
    for e in engines.values():
        e.close()


def bench_kernels(args, emit):
    from vo_single_camera_sos_amd import synthetic
    from vo_single_camera_sos_amd.frontend import DeviceImageModel
    from vo_single_camera_sos_amd.pipeline import FramePairBatch, RigConfig
    from vo_single_camera_sos_amd.runtime import default_context
    gs, rig_kw = _rig_at(args.cols)
    few, _ = synthetic.make_frame_pairs(gs, 8, seed=1234)
    omni = np.concatenate([few] * (args.pairs // 8))
    ctx = default_context()
    model = DeviceImageModel(ctx, gs, (480, 640))
    for setting in ("match", "lk4+fb"):
        _bench_kernels_of(args, emit, ctx, model, rig_kw, omni, setting)
    # sosvo_gray_unpad on its own (the pair pipeline's tracker reads the interior): the 4 * pairs gray panoramas of a step
    import torch
    gray = torch.zeros((4 * args.pairs, model.rows, model.cols + 80), dtype=torch.uint8, device=ctx.device)
    out = ctx.gray_unpad(gray, model.cols)
    ms = []
    for _ in range(args.reps):
        ctx.timer_start()
        ctx.gray_unpad(gray, model.cols, out=out)
        ctx.timer_stop()
        ms.append(ctx.timer_elapsed_ms())
    emit(dict(record="gray_unpad", images=4 * args.pairs, rows=model.rows, cols=model.cols, reps=args.reps, ms=round(float(np.median(ms)), 4),
              gb_per_s=round(2 * out.numel() / (float(np.median(ms)) * 1e-3) / 1e9, 1)))


def _bench_kernels_of(args, emit, ctx, model, rig_kw, omni, setting):
    from vo_single_camera_sos_amd.pipeline import FramePairBatch, RigConfig
    per = {}
    for value in (True, "seam_free", True, "seam_free"):                  # (the second round is the one kept)
        b = FramePairBatch(ctx, model, RigConfig(**rig_kw), args.pairs, num_of_features=1000, kp_cap=512, frame_cap=2048, max_iter=2000,
                           seed=1234, cyclic_columns=value, **SETTINGS[setting])
        b.load_frames(omni)
        b.step()
        ctx.synchronize()
        ctx.profile_enable(True)
        b.step()
        ctx.synchronize()
        sums = {}
        for name, ms in ctx.profile_read():
            sums[name] = sums.get(name, 0.0) + ms
        ctx.profile_enable(False)
        per[value] = sums
        del b
    names = sorted(set(per[True]) | set(per["seam_free"]), key=lambda k: -per["seam_free"].get(k, 0.0))
    emit(dict(record="kernels", setting=setting, pairs=args.pairs, cols=args.cols, total_cyclic_ms=round(sum(per[True].values()), 3),
              total_seam_free_ms=round(sum(per["seam_free"].values()), 3),
              kernels={k: dict(cyclic_ms=round(per[True].get(k, 0.0), 4), seam_free_ms=round(per["seam_free"].get(k, 0.0), 4),
                               ratio=round(per["seam_free"].get(k, 0.0) / per[True][k], 4) if per[True].get(k) else None) for k in names}))


def bench_run_vo(args, emit):
    from vo_single_camera_sos_amd import synthetic
    from vo_single_camera_sos_amd.omnistereo.gum import load_gums_json
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO
    import matching_scenes as scenes
    gs, _ = _rig_at(1200)
    with tempfile.TemporaryDirectory() as root:
        seq = os.path.join(root, "seq")
        synthetic.write_sos_sequence(seq, gs, n_frames=args.vo_frames, seed=77, max_t=40.0, max_deg=2.0)
        cam = load_gums_json(os.path.join(seq, "gums-calibrated.json"))
        times, tracked = {True: [], "seam_free": []}, {}
        for rep in range(args.reps + 1):
            for value in (True, "seam_free"):
                t0 = time.perf_counter()
                out = run_VO(None, cam, **scenes.sos_kwargs(seq, args.vo_frames, os.path.join(root, "results_%s" % value)), frame_window=32,
                             cyclic_columns=value)
                if rep:
                    times[value].append((time.perf_counter() - t0) * 1e3)
                tracked[value] = out["tracked"]
    a, b = float(np.median(times[True])), float(np.median(times["seam_free"]))
    emit(dict(record="run_vo", frames=args.vo_frames, frame_window=32, reps=args.reps, cyclic_ms=round(a, 2), seam_free_ms=round(b, 2),
              seam_free_over_cyclic=round(b / a, 4), tracked_cyclic=tracked[True], tracked_seam_free=tracked["seam_free"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--cols", type=int, default=1440)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--vo-frames", type=int, default=48)
    ap.add_argument("--only", default=None, choices=["accuracy", "step", "kernels", "run_vo"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seam_free", "bench_seam_free.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        for name, fn in (("accuracy", lambda: bench_accuracy(emit)), ("kernels", lambda: bench_kernels(args, emit)),
                         ("step", lambda: bench_step(args, emit)), ("run_vo", lambda: bench_run_vo(args, emit))):
            if args.only in (None, name):
                fn()


if __name__ == "__main__":
    main()
