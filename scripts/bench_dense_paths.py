"""What the four diagonal aggregation paths of the dense stage (paths = 8) cost and give, at the headline
panorama size (--cols 1440: 146 rows), default options with min_disparity 0.
Records (one JSON line each, appended to --out, default profiles/dense_paths/bench_dense_paths.jsonl; no thresholds):
  kernels    DenseOmniStereo(paths=...).step() of n = 1 and n = 64 rendered frames under the library's per-kernel event profile
             (sosvo_profile_*), paths 4 and 8 alternating in one process: milliseconds per dense kernel, their sum, the four
             diagonal launches and their sum beside the up pass; median of --reps steps after one warm-up
  accuracy   the device's map of one frame rendered at pose t = (200, -300, 0) in Room(seed=3) against ray-cast truth, for 4 and
             for 8 paths: the three figures of tests/test_dense_reference.py
On a tree without the `paths` keyword (the parent commit) only the four-path records are made, labelled paths_keyword false, so
that the four-path figures of two trees can be put side by side in one session.
    python scripts/bench_dense_paths.py [--cols 1440] [--reps 9] [--only kernels|accuracy] [--label TEXT] [--out FILE]
"""
import argparse
import inspect
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

POSE_T = (200.0, -300.0, 0.0)


def _rig(cols):
    from vo_single_camera_sos_amd.omnistereo.gum import synthetic_gums
    from vo_single_camera_sos_amd.omnistereo.panorama import Panorama
    gs = synthetic_gums()
    for m in (gs.top_model, gs.bot_model):
        m.panorama = Panorama(m, width=cols)
    gs.make_annulus_masks((480, 640))
    pano = gs.top_model.panorama
    geo = (pano.cols, pano.rows, pano.pixel_size, pano.cyl_height_max)
    return gs, dict(pano_top=geo, pano_bot=geo, F_top=gs.top_model.F[:3, 0], F_bot=gs.bot_model.F[:3, 0], min_range=500.0,
                    max_range=7000.0)


def one_step(ctx, call):
    """-> {kernel label: summed milliseconds of one call}."""
    ctx.profile_enable(True)
    call()
    ctx.synchronize()
    sums = {}
    for name, ms in ctx.profile_read():
        sums[name] = sums.get(name, 0.0) + ms
    ctx.profile_enable(False)
    return sums


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", type=int, default=1440)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default=None, choices=["kernels", "accuracy"])
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_paths", "bench_dense_paths.jsonl"))
    args = ap.parse_args()
    import torch
    import refdense
    from vo_single_camera_sos_amd import synthetic
    from vo_single_camera_sos_amd._lib import DenseOptions
    from vo_single_camera_sos_amd.frontend import DeviceImageModel
    from vo_single_camera_sos_amd.pipeline import DenseOmniStereo, RigConfig
    from vo_single_camera_sos_amd.runtime import default_context
    keyword = "paths" in inspect.signature(DenseOmniStereo.__init__).parameters
    all_paths = (4, 8) if keyword else (4,)
    gs, rig_kw = _rig(args.cols)
    room = synthetic.Room(seed=3)
    frame = synthetic.render_omni(gs, room, np.eye(3), np.array(POSE_T), 2.0, np.random.default_rng(1))   # (before the GPU is touched)
    pair, _ = synthetic.make_frame_pairs(gs, 1, seed=7)
    ctx = default_context()
    model = DeviceImageModel(ctx, gs, (480, 640))
    rows, cols = model.rows, model.cols
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    f = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    def engine(n, paths):
        kw = dict(paths=paths) if keyword else {}
        return DenseOmniStereo(ctx, model, RigConfig(**rig_kw), n, options=opts, **kw)

    opts = DenseOptions(min_disparity=0)
    if args.only in (None, "kernels"):
        for n in (1, 64):
            frames = np.concatenate([frame[None], pair] * ((n + 2) // 3))[:n]
            engines = {p: engine(n, p) for p in all_paths}
            for eng in engines.values():
                eng.load_frames(frames)
                eng.step()                       # warm-up
            ctx.synchronize()
            per = {p: {} for p in all_paths}
            for _ in range(args.reps):           # alternating: neither form has the warmer chip
                for p in all_paths:
                    for k, v in one_step(ctx, engines[p].step).items():
                        per[p].setdefault(k, []).append(v)
            for p in all_paths:
                med = {k: float(np.median(v)) for k, v in per[p].items() if k.startswith("dense_") and "triangulate" not in k}
                diag = {k: v for k, v in med.items() if "diag" in k}
                rec = dict(record="kernels", label=args.label, paths_keyword=keyword, paths=p, n=n, rows=rows, cols=cols, reps=args.reps,
                           options=opts._asdict(), dense_kernel_ms={k: round(v, 4) for k, v in sorted(med.items(), key=lambda kv: -kv[1])},
                           dense_stereo_ms=round(sum(med.values()), 4), up_pass_ms=round(med["dense_path_kernel_up"], 4))
                if diag:
                    rec.update(diagonal_ms=round(sum(diag.values()), 4),
                               diagonal_over_up_pass=round(sum(diag.values()) / (4 * med["dense_path_kernel_up"]), 4))
                emit(rec)
            del engines

    if args.only in (None, "accuracy"):
        white = np.full_like(frame, 255)
        g = ctx.unwrap_median_gray(torch.from_numpy(white[None]).to(ctx.device), model.unwrap_table, 0)
        ctx.synchronize()
        valid = g.cpu().numpy() == 255
        true = refdense.true_disparity(gs, room, POSE_T)
        rec = dict(record="accuracy", label=args.label, paths_keyword=keyword, rows=rows, cols=cols, room="Room(seed=3)", pose_t=POSE_T,
                   ksize=0, options=opts._asdict())
        for p in all_paths:
            one = engine(1, p)
            one.load_frames(frame[None])
            d16, _ = one.step()
            ctx.synchronize()
            comparable, share, within, med = refdense.accuracy(d16.cpu().numpy()[0], true, valid[0], valid[1])
            rec["paths_%d" % p] = dict(comparable=comparable, valid=round(share, 4), within_1_row=round(within, 4),
                                       median_error_rows=round(med, 4))
        emit(rec)


if __name__ == "__main__":
    main()
