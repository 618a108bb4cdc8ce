"""What cyclic panorama columns give and cost, measured in ONE process with the two forms alternating:
the pair pipeline's accuracy with and without the option, and the kernel times of the cyclic stages (sosvo_gray_pyramid_cyclic,
sosvo_track_lk with SOSVO_LK_CYCLIC_COLUMNS, the cyclic |du| gate of the gated matcher) beside their plain forms -- HIP events
around each call (the context's timer): kernel time on the stream, not wall time.  Records (one JSON line each, appended to --out,
default profiles/cyclic/bench_cyclic.jsonl; no thresholds):
  pyramid    the levels 1 .. 2 of the 4 * pairs panoramas of --pairs frame pairs (two views, two frames), rows x cols each
  tracker    --points points per problem, 2 * pairs problems, half 4 and half 10, 3 levels, max_iter 30, eps 0.01, with and
             without the forward-backward check; the starts lie on a grid around the whole circle, the seam's columns included
  matcher    sosvo_match_hamming_gated (du side only) and sosvo_match_hamming_gated_cyclic on 2 * pairs problems of --points
             queries and trains, max_du = cols / 16
  accuracy   FramePairPipeline with and without cyclic_columns, per setting (the matcher; LK half 4 and half 10, 3 levels,
             max_iter 30, forward-backward 0.5 px) and per set of rendered pairs at 1200 columns, GFT 1000 features, one-mirror
             P3P with 2000 iterations: `six` = the six pairs of tests/test_gpu_cross_check.py (seed 4100, no deliberate yaw),
             `yaw5` / `yaw10` / `yaw20` = six rooms each, the second frame turned by +/- that angle about the vertical axis
             and moved by up to 40 mm: correspondences, inlier share, mean rotation / translation error
Each time is the median of --reps calls after one warm-up call; the cyclic / plain ratio is printed beside it.
    python scripts/bench_cyclic.py [--only kernel|accuracy] [--pairs 256] [--rows 300] [--cols 1440] [--points 1000] [--reps 7] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

FB = 0.5
SETTINGS = {"match": {}, "lk4+fb": dict(f2f_tracker="lk", lk=dict(half=4, fb_max=FB)), "lk10+fb": dict(f2f_tracker="lk", lk=dict(half=10, fb_max=FB))}


def _yaw_pairs(gs, yaw_deg, n, seed):
    """n rooms; pair i = the room from the identity pose and from a pose turned by +/- yaw_deg about the vertical axis and moved
    by 10 .. 40 mm -> (omni [2 n, H, W, 3], poses)."""
    from vo_single_camera_sos_amd import synthetic
    omni, poses = [], []
    for i in range(n):
        rng = np.random.default_rng(seed + i)
        room = synthetic.Room(seed=seed + i)
        a = np.deg2rad(yaw_deg if i % 2 else -yaw_deg)
        R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        t = rng.normal(size=3)
        t = t / np.linalg.norm(t) * rng.uniform(10.0, 40.0)
        omni += [synthetic.render_omni(gs, room, np.eye(3), np.zeros(3), 2.0, rng), synthetic.render_omni(gs, room, R, t, 2.0, rng)]
        poses.append((R, t))
    return np.stack(omni), poses


def bench_accuracy(emit):
    import bench_gated_matching as gated
    from bench_cross_check import _rig
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
    for name, (omni, poses) in sets.items():
        B = len(poses)
        fe = ImageFrontEnd(ctx, model, 2 * B, detection_method="GFT", num_of_features=1000, kp_cap=512, keep_panoramas=False)
        fe.load_frames(omni)
        fe.run()
        for setting, kw in SETTINGS.items():
            for cyclic in (False, True):
                pipe = FramePairPipeline(ctx, RigConfig(**rig_kw), B, frame_cap=2048, max_iter=2000, seed=11, front_end=fe,
                                         cyclic_columns=cyclic, **kw)
                pipe.stereo()
                pipe.track()
                out = {"record": "accuracy", "pairs_set": name, "setting": setting, "cyclic_columns": cyclic}
                out.update(gated._accuracy(pipe.results().cpu().numpy(), poses, pipe.frames["M"].cpu().numpy()))
                emit(out)


def _timed(ctx, fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ctx.timer_stop()
        ms.append(ctx.timer_elapsed_ms())
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--rows", type=int, default=300)
    ap.add_argument("--cols", type=int, default=1440)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default=None, choices=["kernel", "accuracy"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cyclic", "bench_cyclic.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.only != "kernel":
        with open(args.out, "a") as f:
            def emit_line(rec):
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
            bench_accuracy(emit_line)
    if args.only == "accuracy":
        return
    import torch
    import reflk_cyclic as rc
    from vo_single_camera_sos_amd.runtime import default_context
    B, rows, cols, cap = args.pairs, args.rows, args.cols, args.points
    # four distinct panoramas (view x frame; the second frame is the first moved by a few pixels around the circle), rendered
    # before the GPU is touched, then repeated per pair on the device: image v * 2 B + 2 i + f is view v, pair i, frame f
    base = np.stack([rc.texture(21, rows, cols), rc.texture(21, rows, cols, (5.3, -1.6)), rc.texture(22, rows, cols),
                     rc.texture(22, rows, cols, (-5.3, 1.6))])
    ys, xs = np.meshgrid(np.linspace(30, rows - 31, 25), np.arange(0, cols, cols / 40.0), indexing="ij")
    grid = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)[:cap]
    ctx = default_context()
    dev = ctx.device
    gray = torch.from_numpy(base).to(dev).view(2, 1, 2, rows, cols).expand(2, B, 2, rows, cols).reshape(4 * B, rows, cols).contiguous()
    prev_img = torch.arange(0, 4 * B, 2, dtype=torch.int32, device=dev)
    next_img = prev_img + 1
    pts = torch.from_numpy(grid).to(dev).view(1, -1, 2).expand(2 * B, len(grid), 2).contiguous()
    n = torch.full((2 * B,), len(grid), dtype=torch.int32, device=dev)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    out = open(args.out, "a")
    shape = dict(pairs=B, rows=rows, cols=cols, points=len(grid), reps=args.reps)

    def emit(rec, plain, cyc):
        rec.update(shape, plain_ms=round(plain, 4), cyclic_ms=round(cyc, 4), cyclic_over_plain=round(cyc / plain, 4))
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    pyr = {False: ctx.gray_pyramid(gray, 3), True: ctx.gray_pyramid_cyclic(gray, 3)}
    t = {c: _timed(ctx, lambda c=c: (ctx.gray_pyramid_cyclic if c else ctx.gray_pyramid)(gray, 3, out=pyr[c]), args.reps) for c in (False, True, False, True)}
    emit(dict(record="pyramid", levels=3), t[False], t[True])
    for half in (4, 10):
        for fb in (None, 0.5):
            bufs = {c: tuple(b.clone() for b in ctx.track_lk(pyr[c], prev_img, next_img, pts, n, half=half, fb_max=0.5)) for c in (False, True)}
            t = {c: _timed(ctx, lambda c=c: ctx.track_lk(pyr[c], prev_img, next_img, pts, n, half=half, fb_max=fb, out=bufs[c]), args.reps)
                 for c in (False, True, False, True)}
            st = {c: float(bufs[c][1].float().mean().item()) for c in (False, True)}
            emit(dict(record="tracker", half=half, levels=3, fb_max=fb, tracked_plain=round(st[False], 4), tracked_cyclic=round(st[True], 4)),
                 t[False], t[True])
    # the gated matcher on random descriptors with positions all around the circle
    g = torch.Generator(device="cpu").manual_seed(5)
    desc = torch.randint(0, 256, (4 * B, cap, 32), dtype=torch.uint8, generator=g).to(dev)
    pos = torch.stack([torch.rand((4 * B, cap), generator=g) * cols, torch.rand((4 * B, cap), generator=g) * rows], -1).to(dev)
    cnt = torch.full((4 * B,), cap, dtype=torch.int32, device=dev)
    keys = torch.empty((2 * B, cap, 1), dtype=torch.uint32, device=dev)
    du = cols / 16.0
    t = {False: _timed(ctx, lambda: ctx.match_hamming_gated(desc, desc, pos, pos, cnt, cnt, -1.0, du, keys=keys, q_slot=next_img, t_slot=prev_img), args.reps),
         True: _timed(ctx, lambda: ctx.match_hamming_gated_cyclic(desc, desc, pos, pos, cnt, cnt, du, cols, keys=keys, q_slot=next_img, t_slot=prev_img), args.reps)}
    emit(dict(record="matcher", max_du=du), t[False], t[True])
    out.close()


if __name__ == "__main__":
    main()
