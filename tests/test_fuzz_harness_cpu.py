"""CPU: the generators of scripts/fuzz_parity.py (the stages themselves need the GPU: tests/test_gpu_fuzz_script.py) -- the
harness must import without touching the GPU, and its inputs must cover what its docstring promises."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _harness():
    spec = importlib.util.spec_from_file_location("fuzz_parity_module", os.path.join(ROOT, "scripts", "fuzz_parity.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generators_cover_the_promised_input_kinds():
    fp = _harness()
    assert set(fp.STAGES) >= {"median", "gft", "fast", "agast", "match", "radius", "orb", "unwrap", "ransac", "describe", "relpose",
                              "l2sort", "pipeline", "rgbd"}
    rng = np.random.default_rng(1)
    kinds = [fp._image(rng, 20, 30, k) for k in range(4)]
    assert all(im.shape == (20, 30) and im.dtype == np.uint8 for im in kinds)
    assert np.unique(kinds[0]).size > 100 and np.unique(kinds[3]).size == 1          # noise ... constant
    seen_empty = seen_full = False
    for _ in range(60):
        bits = fp._masks(rng, 20, 30, 3)
        assert bits.dtype == np.uint32 and bits.max() < 8
        seen_empty |= any(((bits >> m) & 1).sum() == 0 for m in range(3))
        seen_full |= bool((bits == 7).all())
    assert seen_empty and seen_full
    nq, nt = np.array([5, 0, 9], np.int32), np.array([7, 3, 0], np.int32)
    ties = False
    for _ in range(40):
        q, t = fp._descriptors(rng, 3, 9, 7, nq, nt)
        assert q.shape == (3, 9, 32) and t.shape == (3, 7, 32)
        ties |= bool((t[0, 0] == t[0, 1]).all())
    assert ties                                                                       # duplicate train rows occur


def test_batch_and_rgbd_draws_cover_every_detector_and_stay_legal():
    """The `batch` (omni one-call batch from images) and `rgbd` stages draw their configurations without a GPU: over many
    draws every detector and median window appears, both sides of the RGB-D kp_cap 1024 switch appear (for every detector
    but FAST / AGAST, whose capacity is only a cut), capacities that truncate appear, and every draw is a configuration the
    entry points accept (detector_ok, the median set, the ranges of include/sosvo.h)."""
    fp = _harness()
    assert {"batch", "rgbd"} <= set(fp.STAGES)
    rng = np.random.default_rng(7)
    seen = dict(det=set(), median=set(), streams=set(), pairs=set(), pattern=set(), solver=set(), masks=set(), kinds=set())
    orb_2048 = gft_small = cap_below_corners = cap_above_corners = False
    for _ in range(400):
        d = fp.draw_batch(rng)
        det, cap = d["detector"], d["kp_cap"]
        assert det in ("GFT", "ORB", "FAST", "AGAST") and 0 < cap <= (2048 if det == "ORB" else 4096), d
        assert d["median"] in (0, 1, 3, 5, 11) and 1 <= d["n_pairs"] <= 5 and 1 <= d["n_streams"] <= min(4, d["n_pairs"]), d
        assert 0 < d["frame_cap"] <= 16384 and d["max_iter"] <= 400 and 360 <= d["width"] <= 1200, d
        assert 360.0 / d["azimuth"] <= 32 and len(d["frames"]) == d["n_pairs"], d
        if det == "GFT":
            assert 0 < d["quality"] < 1 and 0 < d["max_corners"] <= 1000 and d["min_distance"] < 30, d
        seen["det"].add(det)
        seen["median"].add(d["median"])
        seen["streams"].add(d["n_streams"])
        seen["pairs"].add(d["n_pairs"])
        seen["pattern"].add(d["pattern"])
        seen["solver"].add(d["solver"])
        seen["masks"].add(int(round(360.0 / d["azimuth"])))
        seen["kinds"] |= {k for _, k, _ in d["frames"]}
        orb_2048 |= det == "ORB" and cap == 2048
        gft_small |= det == "GFT" and cap <= 64
        cap_below_corners |= cap < d["max_corners"]
        cap_above_corners |= cap > d["max_corners"]
    assert seen["det"] == {"GFT", "ORB", "FAST", "AGAST"} and seen["median"] == {0, 1, 3, 5, 11}, seen
    assert seen["streams"] == {1, 2, 3, 4} and seen["pairs"] == {1, 2, 3, 4, 5} and seen["pattern"] == {"opencv", "seeded"}
    assert seen["solver"] == {"P3P", "GP3P"} and max(seen["masks"]) == 32 and seen["kinds"] == {0, 1, 2, 3, 4}, seen
    assert orb_2048 and gft_small and cap_below_corners and cap_above_corners
    sides = {}
    algos, meds, cut = set(), set(), False
    for _ in range(400):
        d = fp.draw_rgbd(rng)
        det, cap = d["detector"], d["kp_cap"]
        assert det in ("GFT", "ORB", "FAST", "AGAST") and 0 < cap <= (2048 if det == "ORB" else 4096), d
        assert d["ksize"] in (0, 1, 3, 5, 11) and 0 < d["frame_cap"] <= 16384 and 1 <= d["B"] <= 3, d
        assert det != "GFT" or d["nfeat"] <= 1000, d
        sides.setdefault(det, set()).add(cap > 1024)
        algos.add(d["algo"])
        meds.add(d["ksize"])
        cut |= d["frame_cap"] < cap
    assert set(sides) == {"GFT", "ORB", "FAST", "AGAST"} and all(v == {False, True} for v in sides.values()), sides
    assert algos == {"EPNP", "KNEIP", "GP3P", "TWOPT"} and meds == {0, 1, 3, 5, 11} and cut


def test_rgbd_frames_have_depth_inside_the_range_gates():
    """The rgbd stage's depth maps are in the units of its 0.8 .. 7 range gates: most readings pass them (so frames keep
    keypoints and pairs track), some fall outside, and holes (0 / NaN) occur."""
    fp = _harness()
    rng = np.random.default_rng(3)
    inside = outside = holes = 0
    for _ in range(12):
        bgr, depth = fp.rgbd_frames(rng, 2, 40, 60)
        assert bgr.shape == (4, 40, 60, 3) and bgr.dtype == np.uint8 and depth.shape == (4, 40, 60) and depth.dtype == np.float32
        ok = np.isfinite(depth) & (depth != 0)
        inside += int(((depth >= 0.8) & (depth <= 7.0) & ok).sum())
        outside += int((~((depth >= 0.8) & (depth <= 7.0)) & ok).sum())
        holes += int((~ok).sum())
    assert inside > 2 * outside > 0 and holes > 0, (inside, outside, holes)
