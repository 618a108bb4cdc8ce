"""Several sequences through one engine (run_VO_many, pipeline.MultiSequenceEngine / RGBDMultiSequenceEngine) against the
same sequences through back-to-back run_VO(frame_window=W) calls, measured in ONE invocation, the two paths alternating:
for S in --lanes in-memory synthetic sequences (distinct seeds) of --frames frames, SOS and RGB-D,
    total frames/s          host clock around the whole run, which ends in a synchronise
    GPU ms per frame        from the window events (sequence_mode.stage_s.gpu_windows / the engine's gpu_windows counter):
                            upload wait, front end and the two speculative tracking batches of every window / round
    launches, host synchronisations per frame, serial tracking calls
Medians of --reps repetitions (at least seven) with min, max and the spread (max - min) of both paths.  The pose and
keyframe files of both paths are compared at every size that is timed: they have to be identical.
The last record of each kind is the claim "several sequences fill the chip better than one": GPU ms per frame of the lanes
at the largest S below the back-to-back figure by more than the two spreads together -- printed with the figures, next to
the 0.02 ms per frame VERDICT.md guessed for S = 8.
One JSON line per (kind, S), appended to --out (default profiles/multi_sequence/bench_sequences.jsonl).
    python scripts/bench_sequences.py [--lanes 1,2,4,8] [--frames 256] [--window 32] [--reps 7] [--kinds sos,rgbd]
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

FILES = ("estimated_frame_poses_TUM.txt", "gt_associated_frame_poses_TUM.txt", "keyframe_ids.txt")


def _files(d):
    return tuple(open(os.path.join(d, f)).read() for f in FILES)


def _summary(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values), spread=max(values) - min(values))


def _source(kind, data, k):
    if kind == "sos":
        def frames():
            for i in range(data[k].shape[0]):
                yield i, data[k][i], None
    else:
        def frames():
            bgr, depth = data[k]
            for i in range(bgr.shape[0]):
                yield i, bgr[i], depth[i]
    return frames


def render(kind, n_seq, n_frames, workers):
    """n_seq in-memory sequences with distinct seeds (rendered before the GPU is touched: the workers are forked)."""
    from vo_single_camera_sos_amd import synthetic
    if kind == "sos":
        gs = make_model("sos")
        return [synthetic.make_sequence(gs, n_frames, seed=700 + 11 * k, workers=workers)[0] for k in range(n_seq)]
    return [synthetic.make_rgbd_sequence(n_frames, seed=400 + 7 * k, max_t=40.0, max_deg=2.0, depth_is_Z=False,
                                         workers=workers)[:2] for k in range(n_seq)]


def make_model(kind):
    if kind == "sos":
        from vo_single_camera_sos_amd.omnistereo.gum import synthetic_gums
        from vo_single_camera_sos_amd.omnistereo.panorama import Panorama
        gs = synthetic_gums()
        for m in (gs.top_model, gs.bot_model):
            m.panorama = Panorama(m, width=1200)
        gs.make_annulus_masks((480, 640))
        return gs
    from vo_single_camera_sos_amd.omnistereo.camera_models import RGBDCamModel
    return RGBDCamModel(fx=554.256258, fy=554.256258, center_x=319.5, center_y=239.5, scaling_factor=1. / 1000.0,
                        do_undistortion=False, depth_is_Z=False, focal_length_m=1. / 1000.0)


def back_to_back(kind, model, data, S, W, dirs):
    """The yardstick: S run_VO calls one after the other on one camera model (its sequence engine is reused)."""
    import torch
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO
    t0 = time.perf_counter()
    outs = [run_VO(None, model, results_path=dirs[k], _live_frames=_source(kind, data, k), frame_window=W) for k in range(S)]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    sm = [o["sequence_mode"] for o in outs]
    windows, serial = sum(m["windows"] for m in sm), sum(m["serial_tracking_calls"] for m in sm)
    return dict(wall_s=dt, gpu_s=sum(m["stage_s"]["gpu_windows"] for m in sm), tracked=[o["tracked"] for o in outs],
                serial_calls=serial, front_end_launches=windows, tracking_launches_at_most=2 * windows + serial,
                host_syncs=windows + serial, stage_s=[m["stage_s"] for m in sm])


def lanes(kind, model, data, S, W, dirs):
    import torch
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO_many
    t0 = time.perf_counter()
    outs = run_VO_many(model, [dict(results_path=dirs[k], _live_frames=_source(kind, data, k)) for k in range(S)],
                       frame_window=W, lanes=S)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    sm = outs[0]["sequence_mode"]
    return dict(wall_s=dt, gpu_s=sm["gpu_windows"], tracked=[o["tracked"] for o in outs],
                serial_calls=sum(o["sequence_mode"]["serial_tracking_calls"] for o in outs),
                front_end_launches=sm["front_end_launches"],
                tracking_launches=sm["speculative_track_launches"] + sm["serial_track_launches"],
                serial_track_launches=sm["serial_track_launches"], max_serial_pairs=sm["max_serial_pairs"],
                copy_launches=sm["copy_launches"], host_syncs=sm["host_syncs"], rounds=sm["rounds"],
                stage_s=[o["sequence_mode"]["stage_s"] for o in outs])


def bench_kind(kind, data, args, out_file):
    sizes = sorted(int(v) for v in args.lanes.split(","))
    records = []
    for S in sizes:
        frames = S * args.frames
        with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
            d_solo = [os.path.join(tmp, "solo_%d" % k) for k in range(S)]
            d_many = [os.path.join(tmp, "many_%d" % k) for k in range(S)]
            m_solo, m_many = make_model(kind), make_model(kind)
            back_to_back(kind, m_solo, data, S, args.window, d_solo)        # first-use costs outside the clock
            lanes(kind, m_many, data, S, args.window, d_many)
            runs = {"back_to_back": [], "lanes": []}
            for _ in range(args.reps):                                       # alternating
                runs["back_to_back"].append(back_to_back(kind, m_solo, data, S, args.window, d_solo))
                runs["lanes"].append(lanes(kind, m_many, data, S, args.window, d_many))
            identical = all(_files(a) == _files(b) for a, b in zip(d_solo, d_many))
        rec = {"kind": kind, "lanes": S, "frames_per_sequence": args.frames, "frames": frames, "window": args.window,
               "repetitions": args.reps, "outputs_identical": identical}
        for name, rr in runs.items():
            last = rr[-1]
            rec[name] = {"frames_per_s": _summary([frames / r["wall_s"] for r in rr]),
                         "gpu_ms_per_frame": _summary([1e3 * r["gpu_s"] / frames for r in rr]),
                         "tracked": last["tracked"], "serial_tracking_calls": last["serial_calls"],
                         "host_syncs_per_frame": last["host_syncs"] / frames,
                         "front_end_launches": last["front_end_launches"],
                         "launches_per_frame": (last["front_end_launches"] + last.get("tracking_launches", last.get(
                             "tracking_launches_at_most", 0)) + last.get("copy_launches", 0)) / frames,
                         # where the host's time goes, per lane / per run, seconds of the last repetition
                         "stage_s": [{k: round(v, 5) for k, v in st.items()} for st in last["stage_s"]]}
            for key in ("serial_track_launches", "max_serial_pairs", "copy_launches", "rounds"):
                if key in last:
                    rec[name][key] = last[key]
        line = json.dumps(rec)
        print(line, flush=True)
        out_file.write(line + "\n")
        out_file.flush()
        records.append(rec)
    big, one = records[-1], records[0]
    a, b = big["lanes"]["gpu_ms_per_frame"], big["back_to_back"]["gpu_ms_per_frame"]
    wall_a, wall_b = big["lanes"]["frames_per_s"]["median"], big["back_to_back"]["frames_per_s"]["median"]
    claim = {"kind": kind, "lanes": big["frames"] // args.frames,
             "claim": "GPU ms per frame of the lanes below back-to-back run_VO by more than the two spreads together",
             "lanes_gpu_ms_per_frame": a, "back_to_back_gpu_ms_per_frame": b,
             "single_sequence_gpu_ms_per_frame": one["back_to_back"]["gpu_ms_per_frame"],
             "holds": bool(b["median"] - a["median"] > a["spread"] + b["spread"]),
             "verdict_guess_ms_per_frame": 0.02, "verdict_guess_met": bool(a["median"] <= 0.02),
             "outputs_identical_at_every_size": all(r["outputs_identical"] for r in records),
             "wall_frames_per_s": {"lanes": wall_a, "back_to_back": wall_b, "lanes_below_back_to_back": bool(wall_a < wall_b)}}
    line = json.dumps(claim)
    print(line, flush=True)
    out_file.write(line + "\n")
    out_file.flush()
    return records, claim


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", default="1,2,4,8")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kinds", default="sos,rgbd")
    ap.add_argument("--workers", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "8")))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_sequence", "bench_sequences.jsonl"))
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("--reps: at least seven repetitions")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    ok = True
    kinds = args.kinds.split(",")
    n_seq = max(int(v) for v in args.lanes.split(","))
    data = {kind: render(kind, n_seq, args.frames, args.workers) for kind in kinds}    # (all of it before the first GPU call)
    with open(args.out, "a") as out_file:
        for kind in kinds:
            records, claim = bench_kind(kind, data.pop(kind), args, out_file)
            ok = ok and claim["outputs_identical_at_every_size"] and claim["holds"]
    if not ok:
        sys.exit("bench_sequences: the lanes' files differ from the back-to-back runs', or their GPU time per frame is not "
                 "below the back-to-back figure by more than the two spreads (see the records)")


if __name__ == "__main__":
    main()
