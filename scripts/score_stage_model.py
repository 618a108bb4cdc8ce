"""The staged RANSAC scoring flow as a CPU model on the bench's first frame pairs: which share of
the (solved hypothesis, set of 64 points) evaluations is still scored under a plan.  Host only (the oracle, no GPU):

    python scripts/score_stage_model.py [--pairs 8] [--iters 2000] [--plans 4,16:4,8,16:4,8,12,16]

Renders the pairs as bench.py does (seed 1234, 1440-column panoramas, GFT with 1000 features per mask), runs the
reference's flow on the oracle up to the correspondences (tests/refflow.py), builds the inlier matrix of every
hypothesis (oracle.hypothesis_once, oracle.score_points) and prints, per plan: mean / min / max of the share over the
pairs and the survivors after each stage for pair 0.  "wf" is the worst-first order of the device (set_at in
tests/test_ransac_stage_rule.py, score_set_at in csrc/ransac.hip), "b2f" plain back to front, "today" the flow of
section 17 (the first four sets as one probe).  A plan a,b,c prunes after the positions [0, a), [a, b), [b, c) and scores
the rest for the last survivors; "each" prunes after every set."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle  # noqa: E402
import refflow  # noqa: E402
from test_ransac_prune_rule import prune_model  # noqa: E402
from test_ransac_stage_rule import stage_model  # noqa: E402
from vo_single_camera_sos_amd import orb_pattern, synthetic  # noqa: E402
from vo_single_camera_sos_amd.omnistereo.gum import synthetic_gums  # noqa: E402
from vo_single_camera_sos_amd.omnistereo.panorama import Panorama  # noqa: E402


def bench_correspondences(n_pairs, seed, pano_width=1440, features=1000):
    """-> (list of refflow.track_inputs dicts, cam_off, cam_rot, thr) for the bench's first pairs."""
    gs = synthetic_gums()
    for m in (gs.top_model, gs.bot_model):
        m.panorama = Panorama(m, width=pano_width)
    gs.make_annulus_masks((480, 640))
    bits = []
    for m in (gs.top_model, gs.bot_model):
        mx, my = m.panorama.float32_maps()
        m.panorama.generate_azimuthal_masks(
            30, 0, elev_mask_padding=10, stand_masks_azimuth_coord_in_degrees_list=[50, 170, 290],
            stand_masks_width_in_degrees=10, omni_shape=(480, 640),
            unwrap_fn=lambda om, mx=mx, my=my: oracle.unwrap(np.repeat(om[..., None], 3, 2), None, mx, my)[..., 0])
        bits.append(m.panorama.mask_bits())
    maps = [m.panorama.float32_maps() for m in (gs.top_model, gs.bot_model)]
    pano = gs.top_model.panorama
    geo = (pano.cols, pano.rows, pano.pixel_size, pano.cyl_height_max)
    rp = refflow.RigParams(pano_top=geo, pano_bot=geo, F_top=gs.top_model.F[:3, 0], F_bot=gs.bot_model.F[:3, 0],
                           min_range=500.0, max_range=7000.0, stereo_min_disp=1.0, stereo_max_hdiff=2.5,
                           f2f_max_hdiff=0.125 * 0.5 * pano.cols, pct_good_matches=1.0)
    ca, sa = orb_pattern.angle_cos_sin(-1.0)
    im = refflow.ImageModel(np.stack([maps[0][0], maps[1][0]]), np.stack([maps[0][1], maps[1][1]]),
                            np.stack([gs.top_model.mask, gs.bot_model.mask]),
                            np.ascontiguousarray(np.stack(bits), dtype=np.uint32),
                            max(1, len(gs.top_model.panorama.azimuthal_masks)), features, orb_pattern.orb_pattern(), ca, sa,
                            kp_cap=512)
    omni, _ = synthetic.make_frame_pairs(gs, n_pairs, seed=seed, workers=max(1, min(8, os.cpu_count() or 1)))
    corr = [refflow.track_inputs(rp, refflow.frame_from_image(rp, im, omni[2 * i]), refflow.frame_from_image(rp, im, omni[2 * i + 1]))
            for i in range(n_pairs)]
    return corr, np.stack([rp.F_top, rp.F_bot]), np.stack([np.eye(3), np.eye(3)]), 1.0 - np.cos(np.deg2rad(5.0))


def inlier_matrix(c, cam_off, cam_rot, thr, iters, seed):
    kw = dict(cam=c["cam"], cam_off=cam_off, cam_rot=cam_rot)
    n = c["f"].shape[0]
    solved, inl = np.zeros(iters, bool), np.zeros((iters, n), bool)
    for it in range(iters):
        ok, T, _ = oracle.hypothesis_once(c["f"], c["p"], seed, it, **kw)
        solved[it] = ok
        if ok:
            inl[it] = oracle.score_points(c["f"], c["p"], T, **kw) < thr
    return solved, inl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--plans", default="4,16:4,8,16:4,8,12,16", help="plans separated by ':', boundaries by ','")
    args = ap.parse_args()
    plans = [tuple(int(k) for k in pl.split(",")) for pl in args.plans.split(":")]
    corr, cam_off, cam_rot, thr = bench_correspondences(args.pairs, args.seed)
    rows = {}   # label -> list of (share, survivors per stage)
    for i, c in enumerate(corr):
        n, split = c["f"].shape[0], c["n_top"]
        E = (n + 63) // 64
        solved, inl = inlier_matrix(c, cam_off, cam_rot, thr, args.iters, args.seed + i)
        ns = int(solved.sum())
        full = np.where(solved, inl.sum(axis=1), -1)
        best = int(np.argmax(full))
        misses = [int((~inl[best, 64 * s: 64 * s + 64]).sum()) for s in range(E)]
        print("pair %d: n = %d, %d top, %d solved, best count %d, its misses per set %s" % (i, n, split, ns, full.max(), misses))
        m = prune_model(solved, inl)
        rows.setdefault("today: first 4, rest", []).append(((4 * ns + int(m["alive"].sum()) * (E - 4)) / (ns * E), [int(m["alive"].sum())]))
        cases = [("wf " + ",".join(map(str, pl)) + ",rest", split, pl) for pl in plans]
        cases += [("wf, pruning after every set", split, tuple(range(1, E))),
                  ("b2f 4,8,12,16,rest", 0, (4, 8, 12, 16)), ("b2f: last 4 sets as one probe, rest", 0, (4,))]
        for label, sp, pl in cases:
            m = stage_model(solved, inl, sp, pl)
            assert m["best_iter"] == best
            rows.setdefault(label, []).append((m["scored"] / (ns * E), m["alive_after"]))
    print("\n| plan | mean | min | max | alive after each stage, pair 0 |\n|---|---|---|---|---|")
    for label, r in rows.items():
        sh = np.array([x[0] for x in r])
        alive = "" if "every set" in label else ", ".join(map(str, r[0][1]))
        print("| %s | %.3f | %.3f | %.3f | %s |" % (label, sh.mean(), sh.min(), sh.max(), alive))


if __name__ == "__main__":
    main()
