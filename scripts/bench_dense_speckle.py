"""What the speckle filter of the dense disparity map costs and gives, at the headline panorama size
(--cols 1440: 146 rows), max_size 100, max_diff 16, cyclic.
Records (one JSON line each, appended to --out, default profiles/dense_speckle/bench_dense_speckle.jsonl; no thresholds):
  kernels    DenseOmniStereo(speckle=...).step() of n = 1 and n = 64 rendered frames under the library's per-kernel event profile
             (sosvo_profile_*): milliseconds per speckle kernel, their sum, the sosvo_dense_stereo total of the same steps and the
             ratio of the two; median of --reps steps after one warm-up
  worst      Context.dense_speckle alone on n = 1 and n = 64 copies of one serpentine corridor covering the frame (one component,
             the longest chains), beside the stereo total of the `kernels` record of that n
  accuracy   the device's map of one frame rendered at pose t = (200, -300, 0) in Room(seed=3) against ray-cast truth, with and
             without the filter: the three figures of tests/test_dense_reference.py, the pixels removed and how many of the
             comparable ones were wrong by more than one row
  points     cloud points per frame (finite X) with and without the filter, two rendered frames, median window 11
    python scripts/bench_dense_speckle.py [--cols 1440] [--reps 9] [--only kernels|worst|accuracy|points] [--out FILE]
"""
import argparse
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


def serpentine(rows, cols):
    """A corridor one pixel wide covering the frame (tests/speckle_cases.py's): one component."""
    rr, cc = np.mgrid[0:rows, 0:cols]
    link = np.where((rr % 4) == 1, cc == cols - 1, cc == 0)
    return np.where(((rr & 1) == 0) | link, 300 + (rr & 3), -1).astype(np.int16)


def profiled(ctx, call, reps):
    """-> {kernel label: median over reps of the summed milliseconds of one call}, after one warm-up call."""
    call()
    ctx.synchronize()
    per = {}
    for _ in range(reps):
        ctx.profile_enable(True)
        call()
        ctx.synchronize()
        sums = {}
        for name, ms in ctx.profile_read():
            sums[name] = sums.get(name, 0.0) + ms
        ctx.profile_enable(False)
        for k, v in sums.items():
            per.setdefault(k, []).append(v)
    return {k: float(np.median(v)) for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", type=int, default=1440)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default=None, choices=["kernels", "worst", "accuracy", "points"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_speckle", "bench_dense_speckle.jsonl"))
    args = ap.parse_args()
    import torch
    import refdense
    from vo_single_camera_sos_amd import synthetic
    from vo_single_camera_sos_amd._lib import DenseOptions, SpeckleOptions
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

    opts, sp = DenseOptions(min_disparity=0), SpeckleOptions(max_size=100, max_diff=16, cyclic=True)
    stereo_ms = {}

    def split(med):
        speckle = {k: v for k, v in med.items() if k.startswith("speckle_")}
        stereo = sum(v for k, v in med.items() if k.startswith("dense_") and "triangulate" not in k)
        return speckle, stereo

    if args.only in (None, "kernels", "worst"):
        for n in (1, 64):
            eng = DenseOmniStereo(ctx, model, RigConfig(**rig_kw), n, options=opts, speckle=sp)
            eng.load_frames(np.concatenate([frame[None], pair] * ((n + 2) // 3))[:n])
            speckle, stereo = split(profiled(ctx, eng.step, args.reps))
            stereo_ms[n] = stereo
            total = sum(speckle.values())
            if args.only in (None, "kernels"):
                emit(dict(record="kernels", n=n, rows=rows, cols=cols, reps=args.reps, speckle=sp._asdict(), options=opts._asdict(),
                          input="the device's own map of rendered frames",
                          speckle_kernel_ms={k: round(v, 4) for k, v in sorted(speckle.items(), key=lambda kv: -kv[1])},
                          speckle_ms=round(total, 4), speckle_us_per_frame=round(total * 1e3 / n, 2),
                          dense_stereo_ms=round(stereo, 4), speckle_over_stereo=round(total / stereo, 4),
                          scratch_bytes_per_pixel=8))
            del eng

    if args.only in (None, "worst"):
        for n in (1, 64):
            d = torch.from_numpy(np.repeat(serpentine(rows, cols)[None], n, axis=0)).to(ctx.device)
            out = torch.empty_like(d)
            speckle, _ = split(profiled(ctx, lambda: ctx.dense_speckle(d, options=sp, out=out), args.reps))
            total = sum(speckle.values())
            kept = bool((out == d).all().item())          # (one component of far more than 100 pixels: nothing goes)
            emit(dict(record="worst", n=n, rows=rows, cols=cols, reps=args.reps, speckle=sp._asdict(),
                      input="one serpentine corridor covering the frame, %d pixels in one component" % int((serpentine(rows, cols) >= 0).sum()),
                      speckle_kernel_ms={k: round(v, 4) for k, v in sorted(speckle.items(), key=lambda kv: -kv[1])},
                      speckle_ms=round(total, 4), speckle_us_per_frame=round(total * 1e3 / n, 2),
                      dense_stereo_ms_of_the_rendered_frames=round(stereo_ms[n], 4), speckle_over_stereo=round(total / stereo_ms[n], 4),
                      map_unchanged=kept))

    if args.only in (None, "accuracy"):
        one = DenseOmniStereo(ctx, model, RigConfig(**rig_kw), 1, options=opts)
        one.load_frames(frame[None])
        d16, _ = one.step()
        filtered = ctx.dense_speckle(d16, options=sp)
        white = np.full_like(frame, 255)
        g = ctx.unwrap_median_gray(torch.from_numpy(white[None]).to(ctx.device), model.unwrap_table, 0)
        ctx.synchronize()
        valid = g.cpu().numpy() == 255
        true = refdense.true_disparity(gs, room, POSE_T)
        before, after = d16.cpu().numpy()[0], filtered.cpu().numpy()[0]
        rec = dict(record="accuracy", rows=rows, cols=cols, room="Room(seed=3)", pose_t=POSE_T, ksize=0, options=opts._asdict(),
                   speckle=sp._asdict())
        for key, m in (("without", before), ("with", after)):
            comparable, share, within, med = refdense.accuracy(m, true, valid[0], valid[1])
            rec[key] = dict(comparable=comparable, valid=round(share, 4), within_1_row=round(within, 4), median_error_rows=round(med, 4))
        rr, cc = np.mgrid[0:rows, 0:cols]
        rb = np.clip(np.rint(rr - true).astype(np.int64), 0, rows - 1)
        comp = (valid[0] != 0) & (valid[1][rb, cc] != 0) & (rr - true >= 0) & (true < 63)       # (refdense.accuracy's comparable pixels)
        gone = (before >= 0) & (after < 0)
        wrong = np.abs(before[gone & comp] / 16.0 - true[gone & comp]) > 1.0
        rec.update(pixels_removed=int(gone.sum()), comparable_pixels_removed=int((gone & comp).sum()),
                   of_those_wrong_by_more_than_1_row=int(wrong.sum()))
        emit(rec)

    if args.only in (None, "points"):
        counts = {}
        for key, speckle in (("without", None), ("with", sp)):
            two = DenseOmniStereo(ctx, model, RigConfig(**rig_kw), 2, median_win_size=11, options=DenseOptions(), speckle=speckle)
            two.load_frames(pair)
            _, X2 = two.step()
            ctx.synchronize()
            counts[key] = [int(v) for v in (~np.isnan(X2.cpu().numpy()[..., 0])).sum(axis=(1, 2))]
        emit(dict(record="points", rows=rows, cols=cols, median_win_size=11, options=DenseOptions()._asdict(), speckle=sp._asdict(),
                  dense_cloud_points_per_frame=counts))


if __name__ == "__main__":
    main()
