"""What the pyramidal Lucas-Kanade tracker (sosvo_gray_pyramid + sosvo_track_lk + sosvo_f2f_assemble_tracked,
FramePairPipeline(f2f_tracker="lk")) gives and costs beside the frame-to-frame matcher, measured in ONE process.  Settings:
  match                 the descriptor matcher (the default)
  match+ratio_f2f       ... with the ratio rule frame to frame at r = 48/64 (README's recommended matcher setting)
  lk4 / lk10            the tracker, window half-size 4 / 10, 3 levels, max_iter 30, eps 0.01
  lk4+fb / lk10+fb      ... with the forward-backward check at 0.5 px
Records (one JSON line each, appended to --out, default profiles/lk/bench_lk.jsonl; no thresholds):
  six        the six rendered pairs of tests/test_gpu_cross_check.py (seed 4100, GFT 1000 features): inliers / correspondences,
             pose error against the planted motion, per setting; the front end runs once
  kernel     one profiled FramePairPipeline.track() of --kernel-pairs pairs per setting (HIP events around every launch: the sum
             is kernel time, not wall time): the time of every kernel of the tracking step by name, so the pyramid, the tracker
             and the tracked assemble stand beside the matcher, sort and assemble kernels they replace
  bench      `python bench.py` in this tree and in --parent (a built checkout of the parent commit), alternating, --reps times:
             with the option off nothing changed.  Skipped without --parent.
    python scripts/bench_lk.py [--only six|kernel|bench] [--kernel-pairs 256] [--parent DIR] [--reps 3] [--frames-cache FILE]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bench_gated_matching as gated  # noqa: E402
from bench_cross_check import _rig  # noqa: E402

FB = 0.5
SETTINGS = {"match": {}, "match+ratio_f2f": dict(ratio_f2f=True, ratio=0.75),
            "lk4": dict(f2f_tracker="lk", lk=dict(half=4)), "lk4+fb": dict(f2f_tracker="lk", lk=dict(half=4, fb_max=FB)),
            "lk10": dict(f2f_tracker="lk", lk=dict(half=10)), "lk10+fb": dict(f2f_tracker="lk", lk=dict(half=10, fb_max=FB))}


def _front_end(B, seed, workers, keep_panoramas):
    from vo_single_camera_sos_amd import synthetic
    from vo_single_camera_sos_amd.frontend import DeviceImageModel, ImageFrontEnd
    from vo_single_camera_sos_amd.runtime import default_context
    gs, rig_kw = _rig(1200)
    omni, poses = synthetic.make_frame_pairs(gs, B, seed=seed, workers=workers)      # (rendered before the GPU is touched)
    ctx = default_context()
    fe = ImageFrontEnd(ctx, DeviceImageModel(ctx, gs, (480, 640)), 2 * B, detection_method="GFT", num_of_features=1000, kp_cap=512,
                       keep_panoramas=keep_panoramas)
    fe.load_frames(omni)
    fe.run()
    return ctx, fe, rig_kw, poses


def bench_six(args, emit, names):
    from vo_single_camera_sos_amd.pipeline import FramePairPipeline, RigConfig
    ctx, fe, rig_kw, poses = _front_end(6, 4100, 1, True)
    for name in names:
        pipe = FramePairPipeline(ctx, RigConfig(**rig_kw), 6, frame_cap=2048, max_iter=2000, seed=11, front_end=fe, **SETTINGS[name])
        pipe.stereo()
        pipe.track()
        out = {"record": "six_pairs", "setting": name}
        out.update(gated._accuracy(pipe.results().cpu().numpy(), poses, pipe.frames["M"].cpu().numpy()))
        emit(out)


def bench_kernel(args, emit, names):
    from vo_single_camera_sos_amd.pipeline import FramePairPipeline, RigConfig
    B = args.kernel_pairs
    ctx, fe, rig_kw, poses = _front_end(B, args.seed, args.render_workers, False)
    for name in names:
        pipe = FramePairPipeline(ctx, RigConfig(**rig_kw), B, frame_cap=2048, max_iter=args.iters, seed=args.seed, front_end=fe,
                                 **SETTINGS[name])
        pipe.stereo()
        for _ in range(2):
            pipe.track()
        ctx.synchronize()
        ctx.profile_enable(True)
        pipe.track()
        ctx.synchronize()
        prof = ctx.profile_read()
        ctx.profile_enable(False)
        by_name = {}
        for label, ms in prof:
            by_name[label] = by_name.get(label, 0.0) + ms
        rec = pipe.results().cpu().numpy()
        solver = sum(ms for label, ms in by_name.items() if "ransac" in label or "refine" in label or "lm_" in label)
        emit({"record": "kernel", "setting": name, "pairs": B, "track_kernels_ms": round(sum(by_name.values()), 4),
              "correspondence_kernels_ms": round(sum(by_name.values()) - solver, 4),
              "by_kernel_ms": {k: round(v, 4) for k, v in sorted(by_name.items())},
              "stereo_points_per_frame": round(float(pipe.frames["M"].float().mean()), 1),
              "correspondences_per_pair": round(float(rec[:, 13].mean()), 1)})
        del pipe


def bench_parent(args, emit):
    """bench.py here and in the parent checkout, alternating; each run is a fresh process."""
    if not args.parent:
        print("bench: skipped (no --parent checkout given)", flush=True)
        return
    for rep in range(args.reps):
        for name, root in (("parent", args.parent), ("this", ROOT)):
            cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup)]
            if args.frames_cache:           # (one rendering serves every run of both trees)
                cmd += ["--frames-cache", os.path.abspath(args.frames_cache)]
            out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, check=True).stdout
            line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
            emit({"record": "bench", "tree": name, "rep": rep, "result": json.loads(line)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--kernel-pairs", type=int, default=256, help="pairs of the profiled tracking step")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--settings", default=",".join(SETTINGS))
    ap.add_argument("--only", default="", choices=("", "six", "kernel", "bench"))
    ap.add_argument("--render-workers", type=int, default=16)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the bench record")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames-cache", default=None, help="bench.py's --frames-cache file, shared by the runs of the bench record")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lk", "bench_lk.jsonl"))
    args = ap.parse_args()
    names = [s for s in args.settings.split(",") if s]
    unknown = [s for s in names if s not in SETTINGS]
    if unknown:
        ap.error("unknown settings %s (have: %s)" % (unknown, ", ".join(SETTINGS)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    if args.only in ("", "bench"):
        bench_parent(args, emit)              # (before this process opens the GPU)
    if args.only in ("", "kernel"):
        bench_kernel(args, emit, names)
    if args.only in ("", "six"):
        bench_six(args, emit, names)


if __name__ == "__main__":
    main()
