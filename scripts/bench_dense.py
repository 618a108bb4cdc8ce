"""What dense omnistereo costs and gives, at the headline panorama size (--cols 1440: 146 rows).
Records (one JSON line each, appended to --out, default profiles/dense/bench_dense.jsonl; no thresholds):
  kernels    DenseOmniStereo.step() of n = 1 and n = 64 frames under the library's per-kernel event profile (sosvo_profile_*):
             milliseconds per kernel label (census of both views summed, each aggregation pass, select, left-right,
             triangulate; the unwrap is listed too), median of --reps steps after one warm-up, and the scratch bytes
  accuracy   the device's disparity map of one frame rendered at pose t = (200, -300, 0) in Room(seed=3) against ray-cast truth:
             the three figures of tests/test_dense_reference.py
  points     cloud points per frame (finite X) beside the sparse path's stereo points per frame (GFT, 1000 features per mask)
  cpu        tests/refdense.py on the same gray panoramas, one frame, one core (a plain numpy baseline), and whether its map
             equals the device's
    python scripts/bench_dense.py [--cols 1440] [--reps 9] [--only kernels|accuracy|points|cpu] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

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


def scratch_bytes(n, rows, cols, lr=True):
    """sosvo_dense_stereo's scratch for S_out = NULL: census words of both views, C, S, k*, the left-right keys (256-byte aligned)."""
    total = n * rows * cols
    al = lambda b: (b + 255) & ~255   # noqa: E731
    return 2 * al(total * 8) + al(total * 64) + al(total * 128) + al(total) + (al(total * 4) if lr else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", type=int, default=1440)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default=None, choices=["kernels", "accuracy", "points", "cpu"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense", "bench_dense.jsonl"))
    args = ap.parse_args()
    import refdense
    from vo_single_camera_sos_amd import synthetic
    from vo_single_camera_sos_amd._lib import DenseOptions
    from vo_single_camera_sos_amd.frontend import DeviceImageModel, ImageFrontEnd
    from vo_single_camera_sos_amd.pipeline import DenseOmniStereo, FramePairPipeline, RigConfig, dense_mask
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
    one = DenseOmniStereo(ctx, model, RigConfig(**rig_kw), 1, options=opts)
    one.load_frames(frame[None])
    d16, X = one.step()
    ctx.synchronize()
    d16_h, X_h, gray_h = d16.cpu().numpy()[0], X.cpu().numpy()[0], one.gray.cpu().numpy()
    mask_top = dense_mask(ctx, model).cpu().numpy()

    if args.only in (None, "kernels"):
        for n in (1, 64):
            eng = DenseOmniStereo(ctx, model, RigConfig(**rig_kw), n, options=opts)
            eng.load_frames(np.concatenate([frame[None], pair] * ((n + 2) // 3))[:n])
            eng.step()
            ctx.synchronize()
            per = {}
            for _ in range(args.reps):
                ctx.profile_enable(True)
                eng.step()
                ctx.synchronize()
                sums = {}
                for name, ms in ctx.profile_read():
                    sums[name] = sums.get(name, 0.0) + ms
                ctx.profile_enable(False)
                for k, v in sums.items():
                    per.setdefault(k, []).append(v)
            med = {k: float(np.median(v)) for k, v in per.items()}
            dense = sum(v for k, v in med.items() if k.startswith("dense_") and "triangulate" not in k)
            emit(dict(record="kernels", n=n, rows=rows, cols=cols, reps=args.reps, options=opts._asdict(),
                      kernel_ms={k: round(v, 4) for k, v in sorted(med.items(), key=lambda kv: -kv[1])},
                      dense_stereo_ms=round(dense, 4), dense_stereo_us_per_frame=round(dense * 1e3 / n, 1),
                      scratch_bytes=scratch_bytes(n, rows, cols), scratch_bytes_per_pixel=round(scratch_bytes(n, rows, cols) / (n * rows * cols), 1)))
            del eng

    if args.only in (None, "accuracy"):
        white = np.full_like(frame, 255)
        import torch
        g = ctx.unwrap_median_gray(torch.from_numpy(white[None]).to(ctx.device), model.unwrap_table, 0)
        ctx.synchronize()
        valid = g.cpu().numpy() == 255
        true = refdense.true_disparity(gs, room, POSE_T)
        comparable, share, within, med = refdense.accuracy(d16_h, true, valid[0], valid[1])
        emit(dict(record="accuracy", rows=rows, cols=cols, room="Room(seed=3)", pose_t=POSE_T, ksize=0, options=opts._asdict(),
                  comparable=comparable, valid=round(share, 4), within_1_row=round(within, 4), median_error_rows=round(med, 4),
                  true_rows=[round(float(true[valid[0]].min()), 2), round(float(true[valid[0]].max()), 2)]))

    if args.only in (None, "points"):
        fe = ImageFrontEnd(ctx, model, 2, detection_method="GFT", num_of_features=1000, kp_cap=512, keep_panoramas=False)
        fe.load_frames(pair)
        rig = RigConfig(**rig_kw, stereo_min_disp=1.0, stereo_max_hdiff=2.5)
        pipe = FramePairPipeline(ctx, rig, 1, frame_cap=2048, max_iter=200, seed=5, front_end=fe)
        pipe.step()
        two = DenseOmniStereo(ctx, model, RigConfig(**rig_kw), 2, median_win_size=11, options=DenseOptions())
        two.load_frames(pair)
        _, X2 = two.step()
        ctx.synchronize()
        emit(dict(record="points", rows=rows, cols=cols, median_win_size=11, options=DenseOptions()._asdict(),
                  sparse_stereo_points_per_frame=[int(v) for v in pipe.frames["M"].cpu().numpy()],
                  dense_cloud_points_per_frame=[int(v) for v in (~np.isnan(X2.cpu().numpy()[..., 0])).sum(axis=(1, 2))],
                  pixels_inside_the_top_mask=int((mask_top != 0).sum())))

    if args.only in (None, "cpu"):
        t0 = time.perf_counter()
        want = refdense.dense_stereo(gray_h[0], gray_h[1], mask_top, min_disparity=0)
        emit(dict(record="cpu", rows=rows, cols=cols, refdense_seconds_per_frame=round(time.perf_counter() - t0, 2),
                  equals_the_device=bool(np.array_equal(want, d16_h)), cloud_points=int((~np.isnan(X_h[..., 0])).sum())))


if __name__ == "__main__":
    main()
