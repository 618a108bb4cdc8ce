"""What sub-pixel keypoint refinement (sosvo_refine_subpix, SOSVO_FLAG_SUBPIX) costs and gives, measured in ONE process with the
settings alternating.  Settings:
  off                   no switch
  half2 / half3 / half5 the refinement with that window half-size (max_iter 10, eps 0.01)
  half5+ratio_f2f       half 5 together with the ratio rule frame to frame at r = 48/64 (README's recommended matcher setting)
The records are those of scripts/bench_gated_matching.py (its pairs and sequence benchmarks, given this file's settings), a
six-pairs record of its own (the refinement belongs to the front end, which therefore runs once per setting), and the stage's
kernel time:
  pairs      the headline shape of bench.py, pairs/s from the median of --reps alternating steps, stereo points per frame,
             inliers / correspondences, pose error against the planted motion
  six        the six rendered pairs of tests/test_gpu_cross_check.py: the same accuracy columns, no timing
  sequence   run_VO(frame_window=32) on a synthetic sequence: frames/s from the median run, per-hop error
  kernel     one profiled sosvo_frame_pair_batch step of --kernel-pairs pairs per setting (HIP events around every launch):
             the refinement kernel's time, per keypoint too, against the sum of all kernels of the step
One JSON line per record, appended to --out (default profiles/subpix/bench_subpix.jsonl).
    python scripts/bench_subpix.py [--pairs 768] [--streams 3] [--iters 2000] [--reps 9] [--frames 256] [--only pairs|sequence|six|kernel]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bench_gated_matching as gated  # noqa: E402
from bench_cross_check import _frames, _rig  # noqa: E402

# name -> (window half-size or None, ratio rule frame to frame in 64ths or None)
SETTINGS = {"off": (None, None), "half2": (2, None), "half3": (3, None), "half5": (5, None), "half5+ratio_f2f": (5, 48)}


def _kw(name):
    half, r = SETTINGS[name]
    return dict(subpix=half, ratio_f2f=r is not None, ratio=None if r is None else r / 64.0)


def _run_vo_kw(name):
    half, r = SETTINGS[name]
    return dict(subpix_refine=half is not None, subpix_half=half, ratio_test="f2f" if r is not None else False,
                ratio=None if r is None else r / 64.0)


def bench_six(args, emit, names):
    from vo_single_camera_sos_amd import synthetic
    from vo_single_camera_sos_amd.frontend import DeviceImageModel, ImageFrontEnd
    from vo_single_camera_sos_amd.pipeline import FramePairPipeline, RigConfig
    from vo_single_camera_sos_amd.runtime import default_context
    B = 6
    gs, rig_kw = _rig(1200)
    omni, poses = synthetic.make_frame_pairs(gs, B, seed=4100)
    ctx = default_context()
    fe = ImageFrontEnd(ctx, DeviceImageModel(ctx, gs, (480, 640)), 2 * B, detection_method="GFT", num_of_features=1000, kp_cap=512)
    fe.load_frames(omni)
    fe.run_images()
    for name in names:
        kw = _kw(name)
        fe.subpix = kw.pop("subpix")
        fe.run_features()
        pipe = FramePairPipeline(ctx, RigConfig(**rig_kw), B, frame_cap=2048, max_iter=2000, seed=11, front_end=fe, **kw)
        pipe.stereo()
        pipe.track()
        out = {"record": "six_pairs", "setting": name}
        out.update(gated._accuracy(pipe.results().cpu().numpy(), poses, pipe.frames["M"].cpu().numpy()))
        emit(out)


def bench_kernel(args, emit, names, gs, rig_kw, omni):
    """The stage's own time inside the one-call batch: every launch of one step between HIP events (the events serialise the
    launches, so the sum is kernel time, not the step's wall time)."""
    from vo_single_camera_sos_amd.frontend import DeviceImageModel
    from vo_single_camera_sos_amd.pipeline import FramePairBatch, RigConfig
    from vo_single_camera_sos_amd.runtime import default_context
    ctx = default_context()
    B = min(args.kernel_pairs, omni.shape[0] // 2)
    model = DeviceImageModel(ctx, gs, (480, 640))
    for name in names:
        batch = FramePairBatch(ctx, model, RigConfig(**rig_kw), B, num_of_features=1000, kp_cap=512, frame_cap=2048,
                               max_iter=args.iters, seed=args.seed, **_kw(name))
        batch.load_frames(omni[:2 * B])
        for _ in range(2):
            batch.step()
        ctx.synchronize()
        ctx.profile_enable(True)
        batch.step()
        ctx.synchronize()
        prof = ctx.profile_read()
        ctx.profile_enable(False)
        total = sum(ms for _, ms in prof)
        stage = sum(ms for label, ms in prof if label == "subpix_refine_kernel")
        c = batch.cfg
        n_off = batch.workspace.numel()
        del batch
        out = {"record": "kernel", "setting": name, "pairs": B, "kernels_ms": round(total, 4), "subpix_refine_kernel_ms": round(stage, 4),
               "share_of_kernel_time": round(stage / total, 5) if total else None, "workspace_bytes": int(n_off),
               "problems": int(4 * B * c.nmask), "kp_cap": int(c.kp_cap)}
        emit(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=768)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--pano-width", type=int, default=1440)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9, help="timed steps / runs per setting (the median is reported)")
    ap.add_argument("--frames", type=int, default=256, help="frames of the synthetic sequence")
    ap.add_argument("--kernel-pairs", type=int, default=256, help="pairs of the profiled one-call step")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--settings", default=",".join(SETTINGS))
    ap.add_argument("--only", default="", choices=("", "pairs", "sequence", "six", "kernel"))
    ap.add_argument("--render-workers", type=int, default=16)
    ap.add_argument("--frames-cache", default=None, help="bench.py's --frames-cache file: render once, share")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subpix", "bench_subpix.jsonl"))
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
    # every frame is rendered on the host (forked workers) BEFORE this process touches the GPU
    pairs_in = seq_in = None
    if args.only in ("", "pairs", "kernel"):
        gs, rig_kw = _rig(args.pano_width)
        if args.only == "kernel":
            args.pairs = min(args.pairs, args.kernel_pairs)
        pairs_in = (gs, rig_kw) + _frames(gs, args)
    if args.only in ("", "sequence"):
        from vo_single_camera_sos_amd import synthetic
        seq_in = synthetic.make_sequence(_rig(1200)[0], args.frames, seed=77, max_t=40.0, max_deg=2.0, workers=args.render_workers)
    if pairs_in and args.only in ("", "pairs"):
        gated.bench_pairs(args, emit, names, *pairs_in, kw=_kw)
    if pairs_in and args.only in ("", "kernel"):
        bench_kernel(args, emit, names, pairs_in[0], pairs_in[1], pairs_in[2])
    if args.only in ("", "six"):
        bench_six(args, emit, names)
    if seq_in and args.only in ("", "sequence"):
        gated.bench_sequence(args, emit, names, *seq_in, run_vo_kw=_run_vo_kw)


if __name__ == "__main__":
    main()
