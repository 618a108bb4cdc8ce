"""CPU: the sub-pixel refinement rule as tests/refsubpix.py states it -- accuracy on rendered X-corners, the edge cases, the
exactness bound of the integer sums, the library's weight table, and the reach of the stage against the rows
sosvo_describe_orb_rows guarantees around a keypoint."""
import ctypes
import math

import numpy as np
import pytest

import refsubpix
from cfg_fakes import lib_or_skip
from vo_single_camera_sos_amd import _lib, orb_pattern

N_CASES = 100


@pytest.fixture(scope="module")
def corners():
    """The 100 seeded scenes, rendered once: (image as nested lists, true corner)."""
    lib_or_skip()
    return [(img.tolist(), true) for img, true in (refsubpix.render_corner(seed) for seed in range(N_CASES))]


def _run(corners, half, start):
    errs, iters, reverted = [], [], 0
    for img, (tx, ty) in corners:
        st = {}
        x, y = refsubpix.refine(img, np.float32(start[0]), np.float32(start[1]), half, stats=st)
        errs.append(math.hypot(float(x) - tx, float(y) - ty))
        iters.append(st["iterations"])
        reverted += st["reverted"]
    return np.array(errs), np.array(iters), reverted


def test_rendered_corners_are_found_to_a_few_hundredths_of_a_pixel(corners):
    """100 seeded 64 x 64 X-corners at (31 + U(-.5, .5), 31 + U(-.5, .5)), each started at (31, 31).  Bounds: those of the
    rule's prototype times two (half 5: mean <= 0.06, max <= 0.15 px; half 3: mean <= 0.10 px); no case may revert.
    This rendering of the scene (numpy's default_rng) gives, iterations mean / max and error mean / max, reference only:
        half 2: 6.7 / 9, 0.120 / 0.338 px     half 3: 4.3 / 6, 0.054 / 0.138 px     half 5: 3.0 / 3, 0.031 / 0.100 px
        integer start: 0.369 / 0.620 px
    (the prototype: half 2 6.8 / 9, 0.102 / 0.255; half 3 4.3 / 5, 0.050 / 0.120; half 5 3.0 / 3, 0.032 / 0.082; start
    0.387 / 0.671 -- another noise generator; the bounds are the prototype's, which are the tighter ones)."""
    start = np.array([math.hypot(31 - tx, 31 - ty) for _, (tx, ty) in corners])
    print("integer start: mean %.3f max %.3f px" % (start.mean(), start.max()))
    got = {}
    for half in (2, 3, 5):
        errs, iters, reverted = got[half] = _run(corners, half, (31, 31))
        print("half %d: iterations %.1f / %d, error mean %.3f max %.3f px, %d reverted"
              % (half, iters.mean(), iters.max(), errs.mean(), errs.max(), reverted))
    assert got[5][2] == 0 and got[3][2] == 0 and got[2][2] == 0
    assert got[5][0].mean() <= 0.06 and got[5][0].max() <= 0.15
    assert got[3][0].mean() <= 0.10
    assert got[5][0].mean() < 0.25 * start.mean()


def test_a_start_two_pixels_off_reaches_the_same_accuracy(corners):
    """(33, 30) is 2.2 px from the corner; half 5.  Reference, this rendering: iterations 3.9 / 5, error 0.031 / 0.100 px (the
    prototype: 0.033 / 0.082)."""
    errs, iters, reverted = _run(corners, 5, (33, 30))
    print("start (33, 30): iterations %.1f / %d, error mean %.3f max %.3f px" % (iters.mean(), iters.max(), errs.mean(), errs.max()))
    assert reverted == 0 and errs.mean() <= 0.06 and errs.max() <= 0.15


def test_flat_nan_and_noise():
    lib_or_skip()
    flat = [[77] * 40 for _ in range(40)]
    for half in (2, 3, 4, 5):
        st = {}
        out = refsubpix.refine(flat, np.float32(20.25), np.float32(19.5), half, stats=st)
        assert out == (np.float32(20.25), np.float32(19.5)) and st["iterations"] == 0 and not st["reverted"]
    nan = np.float32("nan")
    for x0, y0 in ((nan, np.float32(3)), (np.float32(3), nan), (np.float32("inf"), np.float32(3)), (np.float32(3), np.float32("-inf"))):
        out = refsubpix.refine(flat, x0, y0, 5)
        assert [np.float32(v).tobytes() for v in out] == [x0.tobytes(), y0.tobytes()]
    rng = np.random.default_rng(5)
    noise = (rng.integers(0, 2, (48, 48)) * 255).astype(np.uint8).tolist()
    moved = 0
    for half in (2, 5):
        for _ in range(40):
            x0, y0 = (np.float32(v) for v in rng.uniform(-3, 51, 2))
            st = {}
            x, y = refsubpix.refine(noise, x0, y0, half, stats=st)
            if st["reverted"]:
                assert (x, y) == (x0, y0)
            else:
                assert abs(float(x) - float(x0)) <= half + 1e-6 and abs(float(y) - float(y0)) <= half + 1e-6
            moved += (x, y) != (x0, y0)
    assert moved > 0


def test_the_sums_stay_far_below_int64():
    """A 0 / 255 checker has the largest differences an u8 image can have.  Analytic bound per sum: (2 half + 1)^2 elements of
    gx gy m (|px| + |py|) <= 121 * (255 * 1024)^2 * 256 * 10 < 2^55."""
    lib_or_skip()
    g = 255 * 1024
    assert 121 * g * g * 256 * 10 < 2 ** 55
    for half in (2, 3, 4, 5):
        w = refsubpix.weights(half)
        assert max(w) == 256 and ((2 * half + 1) ** 2) * g * g * ((max(w) * max(w)) >> 8) * 2 * half < 2 ** 55
    yy, xx = np.mgrid[0:40, 0:40]
    seen = 0
    for cell in (1, 2, 3):
        checker = ((((xx // cell) + (yy // cell)) & 1) * 255).astype(np.uint8).tolist()
        for half in (2, 5):
            for x0, y0 in ((20.0, 20.0), (20.5, 20.5), (19.75, 20.25), (0.0, 0.0), (39.0, 39.0)):
                st = {}
                refsubpix.refine(checker, np.float32(x0), np.float32(y0), half, stats=st)
                seen = max(seen, st["max_sum"])
    print("largest |sum| on the checkers: 2^%.1f" % math.log2(seen))
    assert 0 < seen < 2 ** 55 < 2 ** 63


def test_row_range_clamps_like_an_image_cut_to_those_rows():
    lib_or_skip()
    img, _ = refsubpix.render_corner(3)
    cut = img[20:50].tolist()
    for x0, y0 in ((31.0, 31.0), (31.0, 21.0), (30.5, 48.0)):
        a = refsubpix.refine(img.tolist(), np.float32(x0), np.float32(y0), 5, row_range=(20, 50))
        b = refsubpix.refine(cut, np.float32(x0), np.float32(y0 - 20), 5)
        assert abs(float(a[0]) - float(b[0])) < 1e-5 and abs(float(a[1]) - 20 - float(b[1])) < 1e-5
    assert refsubpix.cut_rows(64, (0, 0)) == (0, 1) and refsubpix.cut_rows(64, (70, 90)) == (63, 64)
    assert refsubpix.cut_rows(64, (-4, 200)) == (0, 64) and refsubpix.cut_rows(64, None) == (0, 64)


def test_the_library_hands_out_the_weight_table():
    lib = lib_or_skip()
    for half in (2, 3, 4, 5):
        want = [int(math.floor(256 * math.exp(-((k - half) / half) ** 2) + 0.5)) for k in range(2 * half + 1)]
        assert _lib.subpix_weights(half) == want and want[half] == 256 and want == want[::-1]
        buf = (ctypes.c_int32 * 13)(*([-7] * 13))
        assert lib.sosvo_subpix_weights(None, half, buf) == 0
        assert list(buf)[:2 * half + 1] == want and list(buf)[2 * half + 1:] == [-7] * (12 - 2 * half)   # nothing beyond
    buf = (ctypes.c_int32 * 13)()
    for bad in (1, 6, 0, -2, 100):
        assert lib.sosvo_subpix_weights(None, bad, buf) == -1
        with pytest.raises(_lib.SosvoError):
            _lib.subpix_weights(bad)
    assert lib.sosvo_subpix_weights(None, 5, None) == -1


def _pattern_radius(pattern, cos_a, sin_a):
    """R of the descriptor stage: the largest |offset| of a test point rotated by the angle and rounded."""
    p = pattern.astype(np.float32)
    rx = np.rint(p[:, 0] * np.float32(cos_a) - p[:, 1] * np.float32(sin_a))
    ry = np.rint(p[:, 0] * np.float32(sin_a) + p[:, 1] * np.float32(cos_a))
    return int(max(np.abs(rx).max(), np.abs(ry).max()))


def test_the_rows_the_descriptor_stage_guarantees_cover_the_reach():
    """sosvo_describe_orb_rows keeps a keypoint only if the rows y - R .. y + R (R: the rotated pattern's radius) lie at
    least 3 rows inside its view's range, so R + 3 rows on either side of y hold computed gray values.  The refinement
    reads within 2 half + 2 rows of y: for half <= 5 the clamp to row_range never acts on the pipeline's keypoints."""
    cos_a, sin_a = orb_pattern.angle_cos_sin(orb_pattern.GFT_KEYPOINT_ANGLE)
    for pattern in (orb_pattern.opencv_pattern(), orb_pattern.seeded_pattern()):
        R = _pattern_radius(pattern, cos_a, sin_a)
        print("pattern radius %d: %d rows guaranteed, reach %d" % (R, R + 3, 2 * 5 + 2))
        for half in (2, 3, 4, 5):
            assert R + 3 >= 2 * half + 2, (R, half)
