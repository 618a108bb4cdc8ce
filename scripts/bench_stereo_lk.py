"""What the sub-pixel static stereo (sosvo_refine_stereo_lk; stereo_refine="lk") gives and costs, measured in ONE process.
Stereo settings: off, lk2 / lk4 / lk10 (the window half-size; max_shift = half, max_iter 30, eps 0.01).  Frame to frame each of
them runs alone (the descriptor matcher), with the ratio rule at r = 48/64 ("+ratio_f2f") and with the Lucas-Kanade tracker at
half 4 and a forward-backward check of 0.5 px ("+f2f_lk4fb").
Records (one JSON line each, appended to --out, default profiles/stereo_lk/bench_stereo_lk.jsonl; no thresholds):
  six        the six rendered pairs of tests/test_gpu_cross_check.py (seed 4100, GFT 1000 features): stereo points per frame,
             the share of bottom keypoints whose tracked position was accepted, inliers / correspondences, mean rotation and
             translation error against the planted motion, per setting
  kernel     one profiled step (front end, stereo, tracking) of --kernel-pairs pairs per stereo setting (HIP events around every
             launch: the sum is kernel time, not wall time): the kernels of the new stage beside all others of the step
  sequence   run_VO(frame_window=32) on the synthetic --frames sequence: frames/s from the median run, per-hop error
  bench      `python bench.py` in this tree and in --parent (a built checkout of the parent commit), alternating, --reps times:
             with the option off nothing changed.  Skipped without --parent.
    python scripts/bench_stereo_lk.py [--only six|kernel|sequence|bench] [--kernel-pairs 256] [--frames 256] [--parent DIR]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT =os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bench_gated_matching as gated  # noqa: E402
from bench_cross_check import _rig  # noqa: E402
from bench_lk import bench_parent  # noqa: E402

STEREO = {"off": None, "lk2": 2, "lk4": 4, "lk10": 10}
F2F = {"": {}, "+ratio_f2f": dict(ratio_f2f=True, ratio=0.75), "+f2f_lk4fb": dict(f2f_tracker="lk", lk=dict(half=4, fb_max=0.5))}
STAGE_KERNELS = ("stereo_lk_gather_kernel", "stereo_lk_accept_kernel", "lk_track_kernel")


def _kw(name):
    """A setting's name (a stereo setting + a frame-to-frame suffix) -> the engines' keyword arguments."""
    stereo = max((s for s in STEREO if name.startswith(s)), key=len)
    half = STEREO[stereo]
    kw = dict(F2F[name[len(stereo):]])
    if half is not None:
        kw.update(stereo_refine="lk", stereo_lk=dict(half=half))
    return kw


def _run_vo_kw(name):
    kw = _kw(name)
    if kw.pop("ratio_f2f", False):
        kw["ratio_test"] = "f2f"
    return kw


def _front_end(B, seed, workers):
    from vo_single_camera_sos_amd import synthetic
    from vo_single_camera_sos_amd.frontend import DeviceImageModel, ImageFrontEnd
    from vo_single_camera_sos_amd.runtime import default_context
    gs, rig_kw = _rig(1200)
    omni, poses = synthetic.make_frame_pairs(gs, B, seed=seed, workers=workers)      # (rendered before the GPU is touched)
    ctx = default_context()
    fe = ImageFrontEnd(ctx, DeviceImageModel(ctx, gs, (480, 640)), 2 * B, detection_method="GFT", num_of_features=1000, kp_cap=512,
                       keep_panoramas=False)
    fe.load_frames(omni)
    return ctx, fe, rig_kw, poses


def bench_six(args, emit, names):
    from vo_single_camera_sos_amd.pipeline import FramePairPipeline, RigConfig
    ctx, fe, rig_kw, poses = _front_end(6, 4100, 1)
    for name in names:
        pipe = FramePairPipeline(ctx, RigConfig(**rig_kw), 6, frame_cap=2048, max_iter=2000, seed=11, front_end=fe, **_kw(name))
        pipe.step()                                  # (the stage moves the front end's keypoints in place: it runs per setting)
        out = {"record": "six_pairs", "setting": name}
        out.update(gated._accuracy(pipe.results().cpu().numpy(), poses, pipe.frames["M"].cpu().numpy()))
        if pipe.stereo_lk is not None:
            # of the bottom keypoints: matched at all / tracked position accepted (the rest: no match, pre-gate, lost, reverted)
            n_bot, st = pipe.n_bot.cpu().numpy(), pipe.s_lk_status.cpu().numpy()
            keys = pipe.s_keys.cpu().numpy().reshape(st.shape)
            live = np.arange(st.shape[1])[None, :] < n_bot[:, None]
            out["bottom_keypoints"] = int(live.sum())
            out["matched_share"] = round(float((live & (keys != 0xFFFFFFFF)).sum()) / max(1, int(live.sum())), 4)
            out["accepted_share"] = round(float((live & (st == 1)).sum()) / max(1, int(live.sum())), 4)
        emit(out)


def bench_kernel(args, emit, names):
    from vo_single_camera_sos_amd.pipeline import FramePairPipeline, RigConfig
    B = args.kernel_pairs
    ctx, fe, rig_kw, poses = _front_end(B, args.seed, args.render_workers)
    for name in names:
        pipe = FramePairPipeline(ctx, RigConfig(**rig_kw), B, frame_cap=2048, max_iter=args.iters, seed=args.seed, front_end=fe,
                                 **_kw(name))
        for _ in range(2):
            pipe.step()
        ctx.synchronize()
        ctx.profile_enable(True)
        pipe.step()
        ctx.synchronize()
        prof = ctx.profile_read()
        ctx.profile_enable(False)
        by_name = {}
        for label, ms in prof:
            by_name[label] = by_name.get(label, 0.0) + ms
        # (lk_track_kernel is the stage's alone here: these settings match frame to frame)
        stage = sum(ms for label, ms in by_name.items() if any(k in label for k in STAGE_KERNELS))
        rec = pipe.results().cpu().numpy()
        emit({"record": "kernel", "setting": name, "pairs": B, "step_kernels_ms": round(sum(by_name.values()), 4),
              "stage_kernels_ms": round(stage, 4), "other_kernels_ms": round(sum(by_name.values()) - stage, 4),
              "by_kernel_ms": {k: round(v, 4) for k, v in sorted(by_name.items())},
              "stereo_points_per_frame": round(float(pipe.frames["M"].float().mean()), 1),
              "correspondences_per_pair": round(float(rec[:, 13].mean()), 1)})
        del pipe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--kernel-pairs", type=int, default=256, help="pairs of the profiled step")
    ap.add_argument("--frames", type=int, default=256, help="frames of the synthetic sequence")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--settings", default=",".join(s + f for f in F2F for s in STEREO), help="for the six pairs")
    ap.add_argument("--only", default="", choices=("", "six", "kernel", "sequence", "bench"))
    ap.add_argument("--render-workers", type=int, default=16)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the bench record")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames-cache", default=None, help="bench.py's --frames-cache file, shared by the runs of the bench record")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stereo_lk", "bench_stereo_lk.jsonl"))
    args = ap.parse_args()
    names = [s for s in args.settings.split(",") if s]
    for s in names:
        try:
            _kw(s)
        except (KeyError, ValueError):
            ap.error("unknown setting %r (a stereo setting of %s with a suffix of %s)" % (s, list(STEREO), list(F2F)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    seq_in = None
    if args.only in ("", "sequence"):            # (rendered before this process opens the GPU)
        from vo_single_camera_sos_amd import synthetic
        seq_in = synthetic.make_sequence(_rig(1200)[0], args.frames, seed=77, max_t=40.0, max_deg=2.0, workers=args.render_workers)
    if args.only in ("", "bench"):
        bench_parent(args, emit)                  # (likewise)
    if args.only in ("", "kernel"):
        bench_kernel(args, emit, list(STEREO))
    if args.only in ("", "six"):
        bench_six(args, emit, names)
    if seq_in:
        gated.bench_sequence(args, emit, list(STEREO), *seq_in, run_vo_kw=_run_vo_kw)


if __name__ == "__main__":
    main()
