"""What Lowe's ratio rule on the device (sosvo_match_hamming_ratio: the rule fused into the matrix-core matcher) costs and
gives, measured in ONE process with the settings alternating.  Settings:
  off                     no switch
  stereo / f2f / both     the rule at r = 48/64 (the reference's 0.75) in the static-stereo / frame-to-frame / both matchers
  f2f_r51 / f2f_r58       frame to frame at r = 51/64 and 58/64
  gated_f2f               gated frame-to-frame matching alone (the 0.66 inlier share of README's gated-matching table)
  gated_f2f+ratio_f2f     ... with the rule among the admissible candidates
  gated_stereo_cap100     gated static stereo with cap 100 (the gated-matching recommendation) alone
  gated_stereo_cap100+ratio_f2f
The records are those of scripts/bench_gated_matching.py (its three benchmarks, given this file's settings):
  pairs      the headline shape of bench.py, pairs/s from the median of --reps alternating steps, stereo points per frame,
             inliers / correspondences, pose error against the planted motion
  six        the six rendered pairs of tests/test_gpu_cross_check.py: the same accuracy columns, no timing
  sequence   run_VO(frame_window=32) on a synthetic sequence: frames/s from the median run, per-hop error
  window1    run_VO(frame_window=1) on the first --frames1 frames: ms per frame from the median run (the live driver's shape:
             one pair x two views per tracking call, where the train-range split of the ratio kernels matters), each setting
             with the split and, through SOSVO_HINT_MATCH_UNSPLIT, without it
  split      the matching step of ONE tracking call at window 1 (one pair x two views = 2 problems, frame_cap 2048, --split-n
             descriptors per frame), launch to completion, median of 200 after 20 warm-up calls, for: the 1-NN search (split over
             the train range), the 2-NN search sosvo_match_hamming(k = 2) -- the same two-smallest loop WITHOUT the split, what
             the ratio form would be without its atomic merge --, and the ratio form plain and gated (split, merged on two words
             per query, then the elementwise pass)
One JSON line per record, appended to --out (default profiles/ratio_test/bench_ratio_test.jsonl).
    python scripts/bench_ratio_test.py [--pairs 768] [--streams 3] [--iters 2000] [--reps 9] [--frames 256] [--only pairs|sequence|six|window1|split]
    python scripts/bench_ratio_test.py --only pairs --settings both --reps 3     (the run a kernel-trace pass wraps)
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bench_gated_matching as gated  # noqa: E402
from bench_cross_check import _frames, _rig, _summary  # noqa: E402

# name -> (ratio_stereo, ratio_f2f, r in 64ths, gated_stereo, gated_f2f, gated_max_distance)
SETTINGS = {
    "off": (False, False, None, False, False, None),
    "stereo": (True, False, 48, False, False, None),
    "f2f": (False, True, 48, False, False, None),
    "both": (True, True, 48, False, False, None),
    "f2f_r51": (False, True, 51, False, False, None),
    "f2f_r58": (False, True, 58, False, False, None),
    "gated_f2f": (False, False, None, False, True, None),
    "gated_f2f+ratio_f2f": (False, True, 48, False, True, None),
    "gated_stereo_cap100": (False, False, None, True, False, 100),
    "gated_stereo_cap100+ratio_f2f": (False, True, 48, True, False, 100),
}


def _kw(name):
    rs, rf, r, gs, gf, cap = SETTINGS[name]
    return dict(ratio_stereo=rs, ratio_f2f=rf, ratio=None if r is None else r / 64.0, gated_stereo=gs, gated_f2f=gf,
                gated_max_distance=cap)


def _which(stereo, f2f):
    return "both" if stereo and f2f else "stereo" if stereo else "f2f" if f2f else False


def _run_vo_kw(name):
    rs, rf, r, gs, gf, cap = SETTINGS[name]
    return dict(ratio_test=_which(rs, rf), ratio=None if r is None else r / 64.0, gated_matching=_which(gs, gf), gated_max_distance=cap)


def bench_window1(args, emit, names, seq):
    """Sequence mode at window 1: every frame is a front-end call of one frame and a tracking call of one pair.  Every setting
    runs twice in each round: as built, and with SOSVO_HINT_MATCH_UNSPLIT on the engines' context (record field `split`)."""
    import torch
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO
    from vo_single_camera_sos_amd.runtime import default_context
    ctx = default_context()
    models = {name: _rig(1200)[0] for name in names}
    N = min(args.frames1, seq.shape[0])

    def frames(n=N):
        for k in range(n):
            yield k, seq[k], None
    times = {(name, split): [] for name in names for split in (True, False)}
    try:
        with tempfile.TemporaryDirectory() as d, contextlib.redirect_stdout(io.StringIO()):
            for name in names:
                run_VO(None, models[name], results_path=d, _live_frames=lambda: frames(min(N, 4)), frame_window=1, **_run_vo_kw(name))
            torch.cuda.synchronize()
            for _ in range(args.reps):
                for name in names:
                    for split in (True, False):
                        ctx.set_hint_match_unsplit(not split)
                        t0 = time.perf_counter()
                        run_VO(None, models[name], results_path=d, _live_frames=frames, frame_window=1, **_run_vo_kw(name))
                        torch.cuda.synchronize()
                        times[name, split].append(time.perf_counter() - t0)
    finally:
        ctx.set_hint_match_unsplit(False)
    base = _summary(times["off", True])["median"] if "off" in names else None
    for name in names:
        for split in (True, False):
            s = _summary(times[name, split])
            out = {"record": "window1", "setting": name, "split": split, "frames": N, "frame_window": 1, "reps": args.reps,
                   "ms_per_frame": round(1e3 * s["median"] / N, 4), "s_per_run": {k: round(v, 4) for k, v in s.items()}}
            if base is not None:
                out["run_time_vs_off"] = round(s["median"] / base, 4)
            emit(out)


def bench_split(args, emit):
    import numpy as np
    import torch
    from vo_single_camera_sos_amd.runtime import default_context
    ctx = default_context()
    rng = np.random.default_rng(7)
    F, S, n = 2, 2048, args.split_n
    dev = ctx.device
    desc = torch.from_numpy(rng.integers(0, 256, (2 * F, S, 32), dtype=np.uint8)).to(dev)
    pos = torch.from_numpy(np.stack([rng.uniform(0, 1200, (2 * F, S)), rng.uniform(0, 300, (2 * F, S))], -1).astype(np.float32)).to(dev)
    cnt = torch.full((2 * F,), n, dtype=torch.int32, device=dev)
    q_slot = torch.tensor([1, 3], dtype=torch.int32, device=dev)   # current frame, top and bottom view
    t_slot = torch.tensor([0, 2], dtype=torch.int32, device=dev)   # reference frame
    k1 = torch.empty((2, S, 1), dtype=torch.uint32, device=dev)
    k2 = torch.empty((2, S, 2), dtype=torch.uint32, device=dev)
    riv = torch.empty((2, S, 1), dtype=torch.uint32, device=dev)
    sl = dict(q_slot=q_slot, t_slot=t_slot)
    calls = {
        "match_hamming_k1_split": lambda: ctx.match_hamming(desc, desc, cnt, cnt, k=1, keys=k1, **sl),
        "match_hamming_k2_unsplit": lambda: ctx.match_hamming(desc, desc, cnt, cnt, k=2, keys=k2, **sl),
        "ratio_plain_split": lambda: ctx.match_hamming_ratio(desc, desc, cnt, cnt, 48, keys=k1, rivals=riv, **sl),
        "ratio_gated_split": lambda: ctx.match_hamming_ratio(desc, desc, cnt, cnt, 48, q_pos=pos, t_pos=pos, min_dv=-1.0, max_du=90.0,
                                                             keys=k1, rivals=riv, **sl),
    }
    for name, call in calls.items():
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        us = []
        for _ in range(200):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            us.append(1e3 * a.elapsed_time(b))
        us.sort()
        emit({"record": "split", "call": name, "problems": 2, "stride": S, "descriptors": n, "reps": 200,
              "us_median": round(us[100], 2), "us_min": round(us[0], 2), "us_p90": round(us[180], 2)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=768)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--pano-width", type=int, default=1440)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9, help="timed steps / runs per setting (the median is reported)")
    ap.add_argument("--frames", type=int, default=256, help="frames of the synthetic sequence")
    ap.add_argument("--frames1", type=int, default=64, help="frames of the window-1 runs")
    ap.add_argument("--split-n", type=int, default=1500, help="descriptors per frame of the split record")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--settings", default=",".join(SETTINGS))
    ap.add_argument("--only", default="", choices=("", "pairs", "sequence", "six", "window1", "split"))
    ap.add_argument("--render-workers", type=int, default=16)
    ap.add_argument("--frames-cache", default=None, help="bench.py's --frames-cache file: render once, share")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ratio_test", "bench_ratio_test.jsonl"))
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
    if args.only in ("", "pairs"):
        gs, rig_kw = _rig(args.pano_width)
        pairs_in = (gs, rig_kw) + _frames(gs, args)
    if args.only in ("", "sequence", "window1"):
        from vo_single_camera_sos_amd import synthetic
        n = args.frames if args.only != "window1" else args.frames1
        seq_in = synthetic.make_sequence(_rig(1200)[0], n, seed=77, max_t=40.0, max_deg=2.0, workers=args.render_workers)
    if pairs_in:
        gated.bench_pairs(args, emit, names, *pairs_in, kw=_kw)
    if args.only in ("", "six"):
        gated.bench_six(args, emit, names, kw=_kw)
    if seq_in and args.only in ("", "sequence"):
        gated.bench_sequence(args, emit, names, *seq_in, run_vo_kw=_run_vo_kw)
    if seq_in and args.only in ("", "window1"):
        bench_window1(args, emit, names, seq_in[0])
    if args.only in ("", "split"):
        bench_split(args, emit)


if __name__ == "__main__":
    main()
