"""What gated matching (the 1-NN search among the candidates that pass the pixel gates) costs and gives, measured in ONE
process with the settings alternating.  Settings: off, and stereo / f2f / both x cap {none, 100, 64} (named e.g. both_cap64).
  pairs      the headline shape of bench.py (OverlappedFramePairs: --pairs frame pairs over --streams streams, 1440-px
             panoramas, GFT 1000 per mask, kp_cap 512, one-mirror P3P with --iters fixed iterations): every engine is warmed,
             then the settings take turns for --reps rounds of one step each; pairs/s from the median step (host clock around
             a step that ends in a synchronise) with min, max and spread, the step time against off, stereo points per frame,
             inliers / correspondences and the pose error against the planted motion of the last step's records
  sequence   run_VO(frame_window=32) on an in-memory synthetic sequence of --frames frames with the trackers' own settings
             (GP3P, adaptive RANSAC of at most 210 iterations), alternating for --reps runs: frames/s from the median run, GPU
             ms per frame from the window events, and the per-hop pose error against the planted trajectory
  six        the six rendered pairs of tests/test_gpu_cross_check.py (seed 4100, GFT 1000, kp_cap 512, P3P 2000 iterations,
             seed 11), whose GPU records equal the CPU oracle flow: the same accuracy columns, no timing
One JSON line per record, appended to --out (default profiles/gated_matching/bench_gated_matching.jsonl).
    python scripts/bench_gated_matching.py [--pairs 768] [--streams 3] [--iters 2000] [--reps 9] [--frames 256] [--only pairs|sequence|six]
    python scripts/bench_gated_matching.py --only pairs --settings both --reps 3     (the run a kernel-trace pass wraps)
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

from bench_cross_check import _frames, _rig, _summary  # noqa: E402

# name -> (gated_stereo, gated_f2f, gated_max_distance)
SETTINGS = {"off": (False, False, None)}
for _name, (_st, _ff) in (("stereo", (True, False)), ("f2f", (False, True)), ("both", (True, True))):
    for _cap in (None, 100, 64):
        SETTINGS[_name if _cap is None else "%s_cap%d" % (_name, _cap)] = (_st, _ff, _cap)


def _kw(name):
    st, ff, cap = SETTINGS[name]
    return dict(gated_stereo=st, gated_f2f=ff, gated_max_distance=cap)


def _run_vo_kw(name):
    st, ff, cap = SETTINGS[name]
    return dict(gated_matching="both" if st and ff else "stereo" if st else "f2f" if ff else False, gated_max_distance=cap)


def _accuracy(rec, poses, stereo_points):
    import synth
    ok = rec[:, 14] == 0
    rot = [np.degrees(synth.pose_error(rec[i, :12].reshape(3, 4), R, t)[0]) for i, (R, t) in enumerate(poses) if ok[i]]
    tra = [float(np.linalg.norm(rec[i, 3:12:4] - t)) for i, (R, t) in enumerate(poses) if ok[i]]
    return {"tracked": int(ok.sum()), "stereo_points_per_frame": round(float(np.mean(stereo_points)), 1),
            "inliers": int(rec[ok, 12].sum()), "correspondences": int(rec[ok, 13].sum()),
            "inlier_share": round(float(rec[ok, 12].sum() / max(1.0, rec[ok, 13].sum())), 4),
            "mean_rotation_error_deg": round(float(np.mean(rot)), 4), "mean_translation_error_mm": round(float(np.mean(tra)), 3),
            "median_rotation_error_deg": round(float(np.median(rot)), 4),
            "median_translation_error_mm": round(float(np.median(tra)), 3)}


# (kw / run_vo_kw: setting name -> the engines' / run_VO's keyword arguments; other benchmarks reuse these three functions with
# settings of their own)
def bench_pairs(args, emit, names, gs, rig_kw, omni, poses, kw=_kw):
    import torch
    from vo_single_camera_sos_amd.pipeline import OverlappedFramePairs, RigConfig
    engines = {}
    for name in names:
        eng = OverlappedFramePairs(0, gs, (480, 640), RigConfig(**rig_kw), args.pairs, n_streams=args.streams, num_of_features=1000,
                                   kp_cap=512, frame_cap=2048, max_iter=args.iters, adaptive=False, seed=args.seed, **kw(name))
        eng.load_frames(omni)
        engines[name] = eng

    def step(eng):
        eng.step()
        rec = eng.results()
        eng.consumed()
        return rec
    for eng in engines.values():
        for _ in range(args.warmup):
            step(eng)
    torch.cuda.synchronize()
    times = {name: [] for name in names}
    for _ in range(args.reps):                       # the settings take turns: drift of the clocks hits all of them alike
        for name in names:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(engines[name])
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    base = statistics.median(times["off"]) if "off" in times else None
    for name in names:
        rec = engines[name].results().cpu().numpy()
        M = np.concatenate([p.pipe.frames["M"].cpu().numpy() for p in engines[name].parts])
        s = _summary(times[name])
        out = {"record": "pairs", "setting": name, "pairs": args.pairs, "streams": args.streams, "iters": args.iters,
               "pano_width": args.pano_width, "reps": args.reps, "pairs_per_s": round(args.pairs / s["median"], 1),
               "ms_per_step": {k: round(1e3 * v, 3) for k, v in s.items()}}
        out.update(_accuracy(rec, poses, M))
        if base is not None:
            out["step_time_vs_off"] = round(s["median"] / base, 4)
        emit(out)
    for eng in engines.values():
        eng.close()


def bench_six(args, emit, names, kw=_kw):
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
    fe.run()
    for name in names:
        pipe = FramePairPipeline(ctx, RigConfig(**rig_kw), B, frame_cap=2048, max_iter=2000, seed=11, front_end=fe, **kw(name))
        pipe.stereo()
        pipe.track()
        out = {"record": "six_pairs", "setting": name}
        out.update(_accuracy(pipe.results().cpu().numpy(), poses, pipe.frames["M"].cpu().numpy()))
        emit(out)


def bench_sequence(args, emit, names, seq, seq_poses, run_vo_kw=_run_vo_kw):
    import torch
    from vo_single_camera_sos_amd.omnistereo import transformations as tr
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO
    # one camera model per setting: a model keeps ONE engine, so alternating settings on one model would rebuild it every run
    models = {name: _rig(1200)[0] for name in names}
    N = seq.shape[0]

    def frames(n=N):
        for k in range(n):
            yield k, seq[k], None
    times, last = {name: [] for name in names}, {}
    with tempfile.TemporaryDirectory() as d, contextlib.redirect_stdout(io.StringIO()):
        for name in names:                           # engine, scratch, first-use costs: outside the clock
            run_VO(None, models[name], results_path=d, _live_frames=lambda: frames(min(N, 34)), frame_window=32, **run_vo_kw(name))
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for name in names:
                t0 = time.perf_counter()
                last[name] = run_VO(None, models[name], results_path=d, _live_frames=frames, frame_window=32, **run_vo_kw(name))
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
    base = statistics.median(times["off"]) if "off" in times else None
    for name in names:
        r, s = last[name], _summary(times[name])
        rot, tra = [], []
        P = r["poses"]
        for k in range(1, len(P)):
            Tg = [np.identity(4), np.identity(4)]
            for j, q in enumerate((k - 1, k)):
                Tg[j][:3, :3], Tg[j][:3, 3] = seq_poses[q][0], seq_poses[q][1] * 1e-3
            E = tr.rpe(tr.concatenate_matrices(tr.inverse_matrix(Tg[0]), Tg[1]),
                       tr.concatenate_matrices(tr.inverse_matrix(P[k - 1][1]), P[k][1]))
            rot.append(np.degrees(tr.rpe_rotation_metric(E)))
            tra.append(1e3 * tr.rpe_translation_metric(E))
        sm = r.get("sequence_mode", {})
        out = {"record": "sequence", "setting": name, "frames": N, "frame_window": 32, "reps": args.reps,
               "frames_per_s": round(N / s["median"], 1), "s_per_run": {k: round(v, 4) for k, v in s.items()},
               "tracked": int(r["tracked"]), "keyframes": len(r["keyframe_ids"]),
               "per_hop_rotation_error_deg_median": round(float(np.median(rot)), 4),
               "per_hop_translation_error_mm_median": round(float(np.median(tra)), 3),
               "per_hop_rotation_error_deg_mean": round(float(np.mean(rot)), 4),
               "per_hop_translation_error_mm_mean": round(float(np.mean(tra)), 3)}
        hw = sm.get("stage_s")
        if hw:
            gpu_s = hw.get("gpu_windows") or hw.get("wait_and_readback", 0.0)
            out["gpu_ms_per_frame"] = round(1e3 * (gpu_s + hw.get("serial_track", 0.0)) / N, 4)
        if base is not None:
            out["run_time_vs_off"] = round(s["median"] / base, 4)
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
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--settings", default=",".join(SETTINGS))
    ap.add_argument("--only", default="", choices=("", "pairs", "sequence", "six"))
    ap.add_argument("--render-workers", type=int, default=16)
    ap.add_argument("--frames-cache", default=None, help="bench.py's --frames-cache file: render once, share")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gated_matching", "bench_gated_matching.jsonl"))
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
    if args.only in ("", "sequence"):
        from vo_single_camera_sos_amd import synthetic
        seq_in = synthetic.make_sequence(_rig(1200)[0], args.frames, seed=77, max_t=40.0, max_deg=2.0, workers=args.render_workers)
    if pairs_in:
        bench_pairs(args, emit, names, *pairs_in)
    if args.only in ("", "six"):
        bench_six(args, emit, names)
    if seq_in:
        bench_sequence(args, emit, names, *seq_in)


if __name__ == "__main__":
    main()
