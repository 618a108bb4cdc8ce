"""CPU: tests/refwls.py -- the numpy statement of the WLS disparity filter -- pinned against outside
truth: numpy.linalg.solve of the explicitly built systems, exact invariants (constants, hard guide edges, the rolled seam), a
per-pixel loop for the confidence, and the ray-cast disparities of tests/test_dense_reference.py; and WlsOptions.  The
thresholds are conditions on the reference alone; the measured values stand beside them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refdense  # noqa: E402
import refwls  # noqa: E402
import test_dense_reference as dense_cases  # noqa: E402


def _guides(rng, n):
    return {"random": rng.integers(0, 256, n).astype(np.uint8), "constant": np.full(n, 77, np.uint8),
            "striped": ((np.arange(n) & 1) * 255).astype(np.uint8)}


@pytest.mark.parametrize("cyclic", (False, True), ids=("clamped", "cyclic"))
@pytest.mark.parametrize("n", (1, 2, 3, 7, 40))
def test_line_solve_against_a_dense_solve(n, cyclic):
    """Every line solve against numpy.linalg.solve of the matrix built entry by entry (corner entries included for the cyclic
    form).  Required: relative agreement 1e-9 (the condition number is at most 1 + 4 lam_t, about 3e4, so rounding allows about
    1e-11).  Measured worst case over all cases: 1.3e-12 (cyclic, 3 elements)."""
    rng = np.random.default_rng(100 * n + cyclic)
    worst = 0.0
    for sigma in (1.0, 8.0):
        w = refwls.weight_table(sigma)
        for lam_t in (0.0, 0.37, 50.0, 8000.0):
            for name, g in _guides(rng, n).items():
                fs = [rng.random(n) * 30000.0, rng.random(n) * 255.0]
                us = refwls.solve_lines(fs, g, lam_t, w, cyclic)
                M = refwls.line_matrix(g, lam_t, w, cyclic)
                for f, u in zip(fs, us):
                    x = np.linalg.solve(M, f)
                    rel = np.abs(u - x).max() / np.abs(x).max()
                    worst = max(worst, rel)
                    assert rel <= 1e-9, (name, sigma, lam_t, rel)
    print("line solve n = %d %s: worst relative difference %.3g" % (n, "cyclic" if cyclic else "clamped", worst))


def test_hard_guide_edge_keeps_the_two_sides_apart():
    """Guide 0 | 255 with sigma = 1 (affinity exp(-255) across the edge), maps 160 | 480, a hole that straddles the edge and
    one more elsewhere: every pixel comes out exactly 160 or 480 on its own side, the holes filled."""
    rows, cols, edge = 12, 20, 9
    guide = np.zeros((rows, cols), np.uint8)
    guide[:, edge:] = 255
    d16 = np.where(guide == 0, 160, 480).astype(np.int16)
    d16[4:7, edge - 2:edge + 3] = -1
    d16[9:11, 1:4] = -1
    for cyclic in (False, True):
        out, _ = refwls.wls(d16, guide, cyclic=cyclic)
        assert np.array_equal(out, np.where(guide == 0, 160, 480))


@pytest.mark.parametrize("cyclic", (False, True), ids=("clamped", "cyclic"))
def test_constant_map_stays_constant(cyclic):
    """333 with 30 % holes under a random guide: every valid output is exactly 333 (the rows of I + lam A sum to 1)."""
    rng = np.random.default_rng(5)
    d16 = np.where(rng.random((17, 23)) < 0.3, -1, 333).astype(np.int16)
    guide = rng.integers(0, 256, d16.shape).astype(np.uint8)
    for sigma in (1.0, 8.0):
        out, _ = refwls.wls(d16, guide, weights=refwls.weight_table(sigma), cyclic=cyclic)
        assert (out >= 0).any() and np.all(out[out >= 0] == 333)


def test_cyclic_form_rolls_with_its_input_and_differs_from_the_clamped_one():
    """Rolling d16, guide and conf by 7 columns rolls the cyclic result exactly; the cyclic and the clamped results differ
    (confidences drawn from 1 .. 255, lambda = 50, sigma = 8, a guide of gray values 0 .. 15 so that the seam couples strongly).
    Measured: see the print; required: more than a quarter of the 6 x 30 map."""
    rng = np.random.default_rng(11)
    d16 = rng.integers(0, 1000, (6, 30)).astype(np.int16)
    d16[rng.random(d16.shape) < 0.2] = -1
    guide = rng.integers(0, 16, d16.shape).astype(np.uint8)
    conf = rng.integers(1, 256, d16.shape).astype(np.uint8)
    kw = dict(lam=50.0, weights=refwls.weight_table(8.0))
    cyc, planes = refwls.wls(d16, guide, conf, cyclic=True, **kw)
    rolled, rolled_planes = refwls.wls(np.roll(d16, 7, 1), np.roll(guide, 7, 1), np.roll(conf, 7, 1), cyclic=True, **kw)
    assert np.array_equal(np.roll(cyc, 7, 1), rolled)
    assert np.allclose(np.roll(planes, 7, 2), rolled_planes, rtol=1e-12, atol=0)
    clamped, _ = refwls.wls(d16, guide, conf, cyclic=False, **kw)
    differ = int((cyc != clamped).sum())
    print("cyclic against clamped: %d of %d pixels differ" % (differ, d16.size))
    assert differ > d16.size // 4
    narrow = rng.integers(0, 1000, (5, 2)).astype(np.int16)        # cols < 3: the flag changes nothing
    g2 = rng.integers(0, 256, narrow.shape).astype(np.uint8)
    assert np.array_equal(refwls.wls(narrow, g2, cyclic=True, **kw)[0], refwls.wls(narrow, g2, cyclic=False, **kw)[0])


def _confidence_loop(d16, radius, roll_ppm, cyclic):
    rows, cols = d16.shape
    out = np.zeros((rows, cols), np.uint8)
    for r in range(rows):
        for c in range(cols):
            if d16[r, c] < 0:
                continue
            m = s1 = s2 = 0
            for dy in range(-radius, radius + 1):
                for dx in range(-radius, radius + 1):
                    rr, cc = r + dy, c + dx
                    if rr < 0 or rr >= rows:
                        continue
                    if cyclic:
                        cc %= cols
                    elif cc < 0 or cc >= cols:
                        continue
                    v = int(d16[rr, cc])
                    if v >= 0:
                        m, s1, s2 = m + 1, s1 + v, s2 + v * v
            V = (m * s2 - s1 * s1) // (m * m)
            out[r, c] = max(0, 255 - (255 * roll_ppm * V) // 1000000)
    return out


@pytest.mark.parametrize("cyclic", (False, True), ids=("clamped", "cyclic"))
@pytest.mark.parametrize("radius", (0, 1, 3, 7))
def test_confidence_against_a_per_pixel_loop(radius, cyclic):
    rng = np.random.default_rng(radius)
    rows, cols = 11, 9
    d16 = (200 + 16 * (np.arange(cols)[None, :] // 4) + rng.integers(0, 6, (rows, cols))).astype(np.int16)
    d16[:, 6:] += 160                                  # a ten-row step
    d16[rng.random(d16.shape) < 0.15] = -1
    for roll_ppm in (1000, 40, 1000000):
        conf = refwls.confidence(d16, radius, roll_ppm, cyclic)
        assert np.array_equal(conf, _confidence_loop(d16, radius, roll_ppm, cyclic))
    if radius == 3 and not cyclic:
        assert conf.dtype == np.uint8
        smooth = refwls.confidence(np.full((9, 9), 500, np.int16))
        assert np.all(smooth == 255)
        step = np.full((9, 12), 320, np.int16)
        step[:, 6:] += 16
        assert refwls.confidence(step)[4, 5] in (239, 240)  # a one-row step: 255 - 255 * 0.001 * 256 * 12 / 49
        step[:, 6:] += 144
        assert refwls.confidence(step)[4, 5] == 0          # a ten-row step: 0


def test_denominators_underflow_gradually_to_zero():
    """A 1 x 64 guide of alternating 0 and 255 (affinity exp(-255) = 1.8e-111 per step) and a single valid pixel: the
    denominators fall through a subnormal to 0, exactly one output pixel is valid, nothing is NaN."""
    guide = ((np.arange(64) & 1) * 255).astype(np.uint8)[None, :]
    d16 = np.full((1, 64), -1, np.int16)
    d16[0, 20] = 640
    out, planes = refwls.wls(d16, guide)
    assert not np.isnan(planes).any()
    D = planes[1, 0]
    tiny = np.finfo(np.float64).tiny
    assert ((D > 0) & (D < tiny)).any() and (D == 0).any()
    print("denominators right of the pixel:", D[20:25])
    assert int((out >= 0).sum()) == 1 and out[0, 20] == 640


def _filtered_case(width, room, ksize):
    """dense_cases._ray_cast_case (imported, not copied) and the WLS filter at its defaults on the case's own map, guided by the
    top gray panorama the stereo read (caught on its way into refdense.dense_stereo) under the top view's mask."""
    caught = {}
    inner = refdense.dense_stereo

    def catching(top, bot, mask=None, **kw):
        caught["top"], caught["mask"] = top, mask
        return inner(top, bot, mask, **kw)
    dense_cases.refdense.dense_stereo = catching
    try:
        d16, true, valid = dense_cases._ray_cast_case(width, room, ksize)
    finally:
        dense_cases.refdense.dense_stereo = inner
    from vo_single_camera_sos_amd._lib import WlsOptions
    o = WlsOptions()
    conf = refwls.confidence(d16, o.radius, o.roll_ppm, o.cyclic)
    out, _ = refwls.wls(d16, caught["top"], conf, caught["mask"], o.lam, o.weight_table(), o.iters, o.min_weight, o.cyclic)
    figures = []
    for name, m in (("raw map", d16), ("filtered", out)):
        comparable, share, within, med = refdense.accuracy(m, true, valid[0], valid[1])
        print("%-8s: %d comparable, %.4f valid, %.4f within 1 row, %.4f valid and within 1 row, median %.4f"
              % (name, comparable, share, within, share * within, med))
        figures.append(share * within)
    return figures


def test_ray_cast_truth_of_the_default_room():
    """Required: valid and within 1 row >= 0.98 of the comparable pixels, and no lower than the raw map's.  Measured: raw 0.9830
    valid, 0.9902 within 1 row, 0.9734 both, median 0.1808; filtered 0.9991, 0.9909, 0.9900, 0.1405."""
    from vo_single_camera_sos_amd import synthetic
    raw, filtered = _filtered_case(480, synthetic.Room(seed=3), 0)
    assert filtered >= 0.98 and filtered >= raw


def test_ray_cast_truth_of_a_near_room():
    """Required: valid and within 1 row >= 0.88, and no lower than the raw map's.  Measured: raw 0.9024 valid, 0.9056 within 1
    row, 0.8171 both, median 0.3000; filtered 1.0000, 0.8988, 0.8988, 0.2746."""
    from vo_single_camera_sos_amd import synthetic
    raw, filtered = _filtered_case(640, synthetic.Room(seed=3, half_x=(500.0, 1500.0), half_y=(400.0, 2500.0)), 11)
    assert filtered >= 0.88 and filtered >= raw


def test_wls_options_refuse_every_bad_value():
    from vo_single_camera_sos_amd._lib import DenseOptions, StepOptions, WlsOptions
    o = WlsOptions()
    assert tuple(o) == (8000.0, 1.0, 3, 3, 1000, 2.0 ** -20, False) and o.flags == 0 and WlsOptions(cyclic=True).flags == 1
    assert WlsOptions.of(None) is None and WlsOptions.of(o) is o and WlsOptions.of(dict(lam=50, sigma=8)).sigma == 8.0
    assert hash(o) == hash(WlsOptions())
    assert WlsOptions(lam=0, iters=8, radius=0, roll_ppm=0).lam == 0.0 and WlsOptions(lam=1e6, radius=7, roll_ppm=10 ** 6).radius == 7
    table = o.weight_table()
    assert len(table) == 256 and table[0] == 1.0 and np.array_equal(np.array(table), refwls.weight_table(1.0))
    assert np.array_equal(np.array(WlsOptions(sigma=8).weight_table()), refwls.weight_table(8.0))
    nan, inf = float("nan"), float("inf")
    bad = [dict(lam=-1), dict(lam=1e6 + 1), dict(lam=nan), dict(lam=inf), dict(lam="8000"), dict(lam=None), dict(lam=True),
           dict(sigma=0), dict(sigma=-1.0), dict(sigma=nan), dict(sigma=inf), dict(sigma=None), dict(iters=0), dict(iters=9),
           dict(iters=2.5), dict(iters=True), dict(radius=-1), dict(radius=8), dict(radius=1.5), dict(radius=None),
           dict(roll_ppm=-1), dict(roll_ppm=10 ** 6 + 1), dict(roll_ppm=0.5), dict(min_weight=0), dict(min_weight=-1.0),
           dict(min_weight=nan), dict(min_weight=inf), dict(cyclic=2), dict(cyclic="yes")]
    for kw in bad:
        with pytest.raises(ValueError):
            WlsOptions(**kw)
    with pytest.raises(ValueError):
        WlsOptions.of(dict(lamda=3))
    with pytest.raises(ValueError):
        WlsOptions.of(7)
    assert "wls" not in StepOptions._fields and "wls" not in DenseOptions._fields
    # the reference's three controls
    assert WlsOptions.from_tuner(False, 8000, 100) is None
    assert WlsOptions.from_tuner(True, 8000, 100) == WlsOptions()
    assert WlsOptions.from_tuner(1, 500, 150, cyclic=True) == WlsOptions(lam=500.0, sigma=1.5, cyclic=True)
    for args in ((True, -1, 100), (True, 8000, 0), (True, 8000, None), (2, 8000, 100), (False, 8000, 0)):
        with pytest.raises(ValueError):
            WlsOptions.from_tuner(*args)
