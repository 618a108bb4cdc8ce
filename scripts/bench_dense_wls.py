"""What the WLS filter of the dense disparity map costs and gives, at the headline panorama size
(--cols 1440: 146 rows), at the reference's defaults (lambda 8000, sigma 1, 3 iterations, radius 3, roll-off 1000 ppm).
Records (one JSON line each, appended to --out, default profiles/dense_wls/bench_dense_wls.jsonl; no thresholds):
  kernels    DenseOmniStereo(wls=...).step() of n = 1 and n = 64 rendered frames, clamped and cyclic, under the library's
             per-kernel event profile (sosvo_profile_*): milliseconds per kernel of the filter summed over the iterations, the
             same per iteration for the solve kernels (four, and the cyclic form's correction), their total, the sosvo_dense_stereo total of the same steps and the
             ratio of the two; median of --reps steps after one warm-up
  accuracy   the device's map of one frame rendered at pose t = (200, -300, 0) in Room(seed=3) against ray-cast truth, before and
             after the filter: the figures of tests/test_dense_reference.py and the product that counts once holes are filled
    python scripts/bench_dense_wls.py [--cols 1440] [--reps 9] [--only kernels|accuracy] [--out FILE]
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

SOLVES = ("wls_rows_forward_kernel", "wls_rows_backward_kernel", "wls_cols_forward_kernel", "wls_cols_backward_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", type=int, default=1440)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default=None, choices=["kernels", "accuracy"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_wls", "bench_dense_wls.jsonl"))
    args = ap.parse_args()
    import torch
    import refdense
    from bench_dense_speckle import POSE_T, _rig, profiled
    from vo_single_camera_sos_amd import dense_filter, synthetic
    from vo_single_camera_sos_amd._lib import DenseOptions, WlsOptions
    from vo_single_camera_sos_amd.frontend import DeviceImageModel
    from vo_single_camera_sos_amd.pipeline import DenseOmniStereo, RigConfig
    from vo_single_camera_sos_amd.runtime import default_context
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

    opts = DenseOptions(min_disparity=0)
    if args.only in (None, "kernels"):
        for n in (1, 64):
            for cyclic in (False, True):
                w = WlsOptions(cyclic=cyclic)
                eng = DenseOmniStereo(ctx, model, RigConfig(**rig_kw), n, options=opts, wls=w)
                eng.load_frames(np.concatenate([frame[None], pair] * ((n + 2) // 3))[:n])
                med = profiled(ctx, eng.step, args.reps)
                wls = {k: v for k, v in med.items() if k.startswith("wls_")}
                stereo = sum(v for k, v in med.items() if k.startswith("dense_") and "triangulate" not in k)
                total = sum(wls.values())
                emit(dict(record="kernels", n=n, rows=rows, cols=cols, reps=args.reps, wls=w._asdict(), options=opts._asdict(),
                          input="the device's own map of rendered frames",
                          wls_kernel_ms={k: round(v, 4) for k, v in sorted(wls.items(), key=lambda kv: -kv[1])},
                          solve_ms_per_iteration={k: round(wls[k] / w.iters, 4) for k in SOLVES + ("wls_rows_correct_kernel",) if k in wls},
                          row_waves=-(-n * rows // 64), column_waves=-(-n * cols // 64),
                          wls_ms=round(total, 4), wls_us_per_frame=round(total * 1e3 / n, 2), dense_stereo_ms=round(stereo, 4),
                          wls_over_stereo=round(total / stereo, 4), scratch_bytes_per_pixel=round(48 + 16 / cols, 3) if cyclic else 40))
                del eng

    if args.only in (None, "accuracy"):
        w = WlsOptions()
        one = DenseOmniStereo(ctx, model, RigConfig(**rig_kw), 1, options=opts)
        one.load_frames(frame[None])
        d16, _ = one.step()
        conf = dense_filter.dense_confidence(ctx, d16, options=w)
        filtered = dense_filter.dense_wls(ctx, d16, one.gray[:1], options=w, conf=conf, mask=one.mask)
        white = np.full_like(frame, 255)
        g = ctx.unwrap_median_gray(torch.from_numpy(white[None]).to(ctx.device), model.unwrap_table, 0)
        ctx.synchronize()
        valid = g.cpu().numpy() == 255
        true = refdense.true_disparity(gs, room, POSE_T)
        rec = dict(record="accuracy", rows=rows, cols=cols, room="Room(seed=3)", pose_t=POSE_T, ksize=0, options=opts._asdict(),
                   wls=w._asdict(), mean_confidence_of_valid=round(float(conf[d16 >= 0].float().mean().item()), 2))
        for key, m in (("without", d16.cpu().numpy()[0]), ("with", filtered.cpu().numpy()[0])):
            comparable, share, within, med = refdense.accuracy(m, true, valid[0], valid[1])
            rec[key] = dict(comparable=comparable, valid=round(share, 4), within_1_row=round(within, 4),
                            valid_and_within_1_row=round(share * within, 4), median_error_rows=round(med, 4))
        emit(rec)


if __name__ == "__main__":
    main()
