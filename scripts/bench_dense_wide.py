"""What the number of disparities of the dense stage (disparities = 16 .. 256) costs and gives.
Records (one JSON line each, appended to --out, default profiles/dense_wide/bench_dense_wide.jsonl; no thresholds):
  kernels    the stereo call on the device's gray panoramas of n = 1 and n = 64 rendered frames at the headline panorama size
             (--cols 1440: 146 rows) under the library's per-kernel event profile (sosvo_profile_*); D = 16, 32, 64 through the
             existing kernels (Context.dense_stereo: the yardstick), 64 through the new kernels (the hook
             dense_wide.debug_dense_stereo_wide_kernels), 128 and 256 alternating in one process: milliseconds per dense
             kernel and their sum, each pass relative to the existing D = 64 pass of the same run beside D / 64, and the scratch in
             bytes per pixel; default options with min_disparity 0, four paths; median of --reps calls after one warm-up
  large      the same at --large-cols 2880 (292 rows), D = 64 (existing) and 256, with the largest n <= 64 whose D = 256 scratch
             fits in half of the free device memory; the record states n and the scratch
  accuracy   the device's maps of the near room of tests/dense_wide_scenes.py (walls at 0.25 to 0.4 m, 1440 columns) against
             ray-cast truth for D = 64, 128 and 256: the figures of tests/test_dense_wide_reference.py on the truth bands
             [65, 127) and [0, 63)
    python scripts/bench_dense_wide.py [--reps 9] [--only kernels|large|accuracy] [--label TEXT] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PASSES = ("down", "path_kernel_up", "path_kernel_lr", "path_kernel_rl", "select", "left_right")
EXISTING_64, WIDE_64 = "64", "64_wide_kernels"


def _rig(cols):
    from vo_single_camera_sos_amd.omnistereo.gum import synthetic_gums
    from vo_single_camera_sos_amd.omnistereo.panorama import Panorama
    gs = synthetic_gums()
    for m in (gs.top_model, gs.bot_model):
        m.panorama = Panorama(m, width=cols)
    gs.make_annulus_masks((480, 640))
    pano = gs.top_model.panorama
    geo = (pano.cols, pano.rows, pano.pixel_size, pano.cyl_height_max)
    return gs, dict(pano_top=geo, pano_bot=geo, F_top=gs.top_model.F[:3, 0], F_bot=gs.bot_model.F[:3, 0], min_range=0.0, max_range=0.0)


def one_call(ctx, call):
    """-> {kernel label: summed milliseconds of one call}."""
    ctx.profile_enable(True)
    call()
    ctx.synchronize()
    sums = {}
    for name, ms in ctx.profile_read():
        sums[name] = sums.get(name, 0.0) + ms
    ctx.profile_enable(False)
    return sums


def _pass_of(label):
    """A kernel label of either family -> its pass, or None (the census)."""
    for p in PASSES:
        if label in ("dense_%s_kernel" % p, "dense_wide_%s_kernel" % p, "dense_" + p, "dense_wide_" + p):
            return p
    return None


def _stereo(ctx, kind, top, bot, mask, opts):
    from vo_single_camera_sos_amd import dense_wide
    if kind == EXISTING_64:
        return ctx.dense_stereo(top, bot, mask, options=opts)
    if kind == WIDE_64:
        return dense_wide.debug_dense_stereo_wide_kernels(ctx, top, bot, mask, options=opts, disparities=64)
    return dense_wide.dense_stereo(ctx, top, bot, mask, options=opts, disparities=int(kind))


def kernel_records(ctx, emit, label, record, cols, n, kinds, reps):
    """n = None: the largest n <= 64 whose scratch at the largest D fits in half of the free device memory."""
    import torch
    from vo_single_camera_sos_amd import synthetic
    from vo_single_camera_sos_amd._lib import DenseOptions
    from vo_single_camera_sos_amd.frontend import DeviceImageModel
    from vo_single_camera_sos_amd.pipeline import dense_mask
    gs, _ = _rig(cols)
    model = DeviceImageModel(ctx, gs, (480, 640))
    mask = dense_mask(ctx, model)
    rows = model.rows
    widest = max(22 + 3 * int(k) for k in kinds if k not in (EXISTING_64, WIDE_64))
    extra = {}
    if n is None:
        free, _ = torch.cuda.mem_get_info()
        n = int(max(1, min(64, (free // 2) // (widest * rows * model.cols))))
        extra = dict(free_device_bytes=int(free), scratch_bytes=widest * rows * model.cols * n)
    pair, _ = synthetic.make_frame_pairs(gs, 1, seed=7)
    frames = np.concatenate([pair] * ((n + 1) // 2))[:n]
    gray = ctx.unwrap_median_gray(torch.from_numpy(np.ascontiguousarray(frames)).to(ctx.device), model.unwrap_table, 0)
    top, bot = gray[:n].contiguous(), gray[n:].contiguous()
    opts = DenseOptions(min_disparity=0)
    for kind in kinds:
        _stereo(ctx, kind, top, bot, mask, opts)    # warm-up (the scratch grows to the largest D here, not inside a timed call)
    ctx.synchronize()
    per = {kind: {} for kind in kinds}
    for _ in range(reps):                # alternating: no D has the warmer chip
        for kind in kinds:
            for k, v in one_call(ctx, lambda: _stereo(ctx, kind, top, bot, mask, opts)).items():
                per[kind].setdefault(k, []).append(v)
    base = None
    for kind in sorted(kinds, key=lambda k: k != EXISTING_64):      # the existing 64 first: the yardstick of the others
        D = 64 if kind in (EXISTING_64, WIDE_64) else int(kind)
        med = {k: float(np.median(v)) for k, v in per[kind].items() if k.startswith("dense_")}
        passes = {_pass_of(k): v for k, v in med.items() if _pass_of(k)}
        if kind == EXISTING_64:
            base = passes
        rec = dict(record=record, label=label, disparities=D, kernels="existing" if kind == EXISTING_64 else "wide", n=n, rows=rows,
                   cols=model.cols, reps=reps, options=opts._asdict(), scratch_bytes_per_pixel=213 if kind == EXISTING_64 else 22 + 3 * D,
                   dense_kernel_ms={k: round(v, 4) for k, v in sorted(med.items(), key=lambda kv: -kv[1])},
                   dense_stereo_ms=round(sum(med.values()), 4), passes_ms=round(sum(passes.values()), 4), bytes_ratio=round(D / 64.0, 4))
        rec.update(extra)
        if base:
            rec["pass_over_64"] = {p: round(passes[p] / base[p], 4) for p in PASSES if p in passes and p in base}
            rec["passes_over_64"] = round(sum(passes.values()) / sum(base.values()), 4)
        emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", type=int, default=1440)
    ap.add_argument("--large-cols", type=int, default=2880)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default=None, choices=["kernels", "large", "accuracy"])
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_wide", "bench_dense_wide.jsonl"))
    args = ap.parse_args()
    from vo_single_camera_sos_amd._lib import DenseOptions
    from vo_single_camera_sos_amd.frontend import DeviceImageModel
    from vo_single_camera_sos_amd.pipeline import DenseOmniStereo, RigConfig
    from vo_single_camera_sos_amd.runtime import default_context
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    f = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    scene = None
    if args.only in (None, "accuracy"):
        import dense_wide_scenes
        scene = dense_wide_scenes.near_room_scene()         # (rendered before the GPU is touched)
    ctx = default_context()
    if args.only in (None, "kernels"):
        for n in (1, 64):
            kernel_records(ctx, emit, args.label, "kernels", args.cols, n, ("16", "32", EXISTING_64, WIDE_64, "128", "256"), args.reps)
    if args.only in (None, "large"):
        kernel_records(ctx, emit, args.label, "large", args.large_cols, None, (EXISTING_64, "256"), args.reps)
    if scene is not None:
        import refdense_wide
        gs, omni, _, valid, true = scene
        model = DeviceImageModel(ctx, gs, (480, 640))
        _, rig_kw = _rig(1440)
        opts = DenseOptions(min_disparity=0)
        rec = dict(record="accuracy", label=args.label, rows=model.rows, cols=model.cols, pose_t=(0.0, 0.0, 0.0), ksize=0,
                   room="Room(seed=3, half_x=(250, 400), half_y=(300, 1000), cells=(60, 15))", options=opts._asdict())
        for D in (64, 128, 256):
            one = DenseOmniStereo(ctx, model, RigConfig(**rig_kw), 1, options=opts, min_disparity=0.0, disparities=D)
            one.load_frames(omni[None])
            d16, _ = one.step()
            ctx.synchronize()
            d16 = d16.cpu().numpy()[0]
            for name, lo, hi in (("truth_65_127", 65.0, 127.0), ("truth_below_63", 0.0, 63.0)):
                comparable, share, both, within, med = refdense_wide.accuracy(d16, true, valid[0], valid[1], lo, hi)
                rec["D%d_%s" % (D, name)] = dict(comparable=comparable, valid=round(share, 4), valid_and_within_1_row=round(both, 4),
                                                 within_1_row_of_the_valid=round(within, 4), median_error_rows=round(med, 4))
        emit(rec)


if __name__ == "__main__":
    main()
