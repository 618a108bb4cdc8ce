"""CPU: the pyramidal Lucas-Kanade rule as tests/reflk.py states it (the reference the device stages equal bit for bit,
tests/test_gpu_lk.py): the pyramid's sizes and arithmetic, the bounds that make the integer sums exact, and what the rule
recovers on images that ARE shifted copies of each other (reflk.texture: sinusoids evaluated analytically, quantised to u8).

The tolerances are measured, not chosen: RECOVERED_* below are twice the largest error of this reference on these scenes
(the 1/32-px grid alone puts a floor near 1/64 px, the u8 quantisation adds to it)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import reflk  # noqa: E402

ROWS, COLS, SEED, MAX_ITER = 96, 128, 11, 10
SMALL_SHIFT, LARGE_SHIFT = (0.37, -0.21), (5.3, -3.6)
# largest |error| (either axis) of reflk.track on the scene (SEED, 96 x 128, the 60 grid points below, max_iter 10, eps 0.01):
#   shift (0.37, -0.21), half 4, 1 level:  0.06100 px     shift (5.3, -3.6), half 4, 3 levels:  0.06960 px
# (half 10: 0.0203 / 0.0278 px; half 2, 1 level: 0.153 px -- a 5 x 5 window is a poor estimator, not a wrong one)
MEASURED_SMALL, MEASURED_LARGE = 0.06100, 0.06960
RECOVERED_SMALL, RECOVERED_LARGE = 2 * MEASURED_SMALL, 2 * MEASURED_LARGE


@pytest.fixture(scope="module")
def first():
    return reflk.texture(SEED, ROWS, COLS)


def _points():
    return reflk.grid_points(ROWS, COLS, 24, 8)


def _errors(a, b, shift, half, levels, **kw):
    pa, pb = reflk.pyramid(a, levels), reflk.pyramid(b, levels)
    out = []
    for x, y in _points():
        nx, ny, st, _ = reflk.track(pa, pb, x, y, half, max_iter=MAX_ITER, **kw)
        out.append((st, max(abs(float(nx) - float(x) - shift[0]), abs(float(ny) - float(y) - shift[1]))))
    return np.array([s for s, _ in out]), np.array([e for _, e in out])


def test_pyramid_sizes_and_a_constant_image():
    assert reflk.level_sizes(96, 128, 4) == [(96, 128), (48, 64), (24, 32), (12, 16)]
    assert reflk.level_sizes(95, 127, 4) == [(95, 127), (48, 64), (24, 32), (12, 16)]
    assert reflk.level_sizes(1, 3, 3) == [(1, 3), (1, 2), (1, 1)]
    for value in (0, 1, 77, 255):          # the kernel sums to 256: a constant stays what it is, at the borders too
        lv, rr = reflk.pyramid(np.full((37, 53), value, np.uint8), 4)
        assert [l.shape for l in lv] == [(37, 53), (19, 27), (10, 14), (5, 7)]
        assert all((l == value).all() for l in lv)
        assert rr == [(0, 37), (0, 19), (0, 10), (0, 5)]


def test_row_ranges_of_the_levels():
    lv, rr = reflk.pyramid(np.zeros((96, 128), np.uint8), 4, row_range=(21, 70))
    assert rr == [(21, 70), (11, 35), (6, 18), (3, 9)]
    # cut to the image, at least one row, on every level; a range on the last row of an even level stays inside the next
    assert reflk.pyramid(np.zeros((96, 8), np.uint8), 3, row_range=(95, 400))[1] == [(95, 96), (47, 48), (23, 24)]
    assert reflk.pyramid(np.zeros((96, 8), np.uint8), 3, row_range=(-5, 0))[1] == [(0, 1), (0, 1), (0, 1)]
    # rows outside the range do not reach the result: noise there, same levels inside the ranges
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (96, 128), dtype=np.uint8)
    noisy = img.copy()
    noisy[:21], noisy[70:] = rng.integers(0, 256, (21, 128)), rng.integers(0, 256, (26, 128))
    a, ra = reflk.pyramid(img, 4, row_range=(21, 70))
    b, _ = reflk.pyramid(noisy, 4, row_range=(21, 70))
    for l in range(1, 4):
        assert np.array_equal(a[l][ra[l][0]:ra[l][1]], b[l][ra[l][0]:ra[l][1]])
        assert not a[l][:ra[l][0]].any() and not a[l][ra[l][1]:].any()       # (not written)


def test_sums_stay_exact_at_the_largest_window():
    """Every integer sum of the rule stays below 2^53 (so its conversion to double is exact) at half 10 on the image that
    makes them largest: pixels 0 / 255 at random."""
    rng = np.random.default_rng(5)
    a = (rng.integers(0, 2, (64, 64)) * 255).astype(np.uint8)
    b = (rng.integers(0, 2, (64, 64)) * 255).astype(np.uint8)
    pa, pb = reflk.pyramid(a, 1), reflk.pyramid(b, 1)
    stats = {}
    for x, y in ((20.0, 20.0), (31.5, 33.25), (40.03, 22.97)):
        reflk.track(pa, pb, np.float32(x), np.float32(y), 10, max_iter=3, min_eig=0.0, stats=stats)
    assert 2 ** 40 < stats["max_sum"] < 2 ** 53
    assert 441 * (16 * 255 * 1024) ** 2 < 2 ** 53      # the bound itself: N |g|^2


def test_a_flat_image_loses_every_point():
    flat = np.full((ROWS, COLS), 93, np.uint8)
    for levels in (1, 3):
        p = reflk.pyramid(flat, levels)
        for x, y in _points():
            nx, ny, st, err = reflk.track(p, p, x, y, 4, max_iter=MAX_ITER)
            assert st == 0 and err == 0 and (nx, ny) == (x, y)


def test_a_small_planted_shift_is_recovered_at_one_level(first):
    """Largest error of the reference: 0.06100 px (half 4, 1 level, shift (0.37, -0.21)); the bound is twice that."""
    st, err = _errors(first, reflk.texture(SEED, ROWS, COLS, SMALL_SHIFT), SMALL_SHIFT, 4, 1)
    print("small shift: largest error %.5f px" % err.max())
    assert st.all() and err.max() <= RECOVERED_SMALL
    assert abs(err.max() - MEASURED_SMALL) < 5e-4       # the figure the bound was derived from is still the figure


def test_a_large_planted_shift_needs_the_pyramid(first):
    """Largest error of the reference with 3 levels: 0.06960 px (half 4, shift (5.3, -3.6)); the bound is twice that.  With one
    level a 9 x 9 window cannot see a 6.4-px motion: points end up tens of pixels away (largest error 30.9 px)."""
    second = reflk.texture(SEED, ROWS, COLS, LARGE_SHIFT)
    st, err = _errors(first, second, LARGE_SHIFT, 4, 3)
    print("large shift, 3 levels: largest error %.5f px" % err.max())
    assert st.all() and err.max() <= RECOVERED_LARGE
    assert abs(err.max() - MEASURED_LARGE) < 5e-4
    st1, err1 = _errors(first, second, LARGE_SHIFT, 4, 1)
    print("large shift, 1 level: largest error %.3f px, %d of %d within the bound" % (err1.max(), (err1 <= RECOVERED_LARGE).sum(), len(err1)))
    assert err1.max() > 1.0 and not (err1[st1 == 1] <= RECOVERED_LARGE).all()


def test_the_initial_flow_at_the_truth_converges_in_one_iteration(first):
    """An integer shift makes the second image the first one moved, pixel for pixel: from the true position J equals T, the
    first step is exactly zero and the residual is zero.  Without the guess the same point needs several iterations."""
    shift = (3.0, -2.0)
    pa, pb = reflk.pyramid(first, 1), reflk.pyramid(reflk.texture(SEED, ROWS, COLS, shift), 1)
    for x, y in _points()[::7]:
        stats = {}
        guess = (np.float32(x + shift[0]), np.float32(y + shift[1]))
        nx, ny, st, err = reflk.track(pa, pb, x, y, 4, max_iter=MAX_ITER, guess=guess, stats=stats)
        assert st == 1 and stats["iterations"] == [1] and (nx, ny) == guess and err == 0
        stats = {}
        reflk.track(pa, pb, x, y, 4, max_iter=MAX_ITER, stats=stats)
        assert stats["iterations"][0] > 1


def test_the_forward_backward_check_rejects_a_replaced_patch(first):
    """The second image is the first moved by (1.3, -0.8) with a 40 x 50 patch replaced by another texture.  fb_max = 0.25 px:
    a genuine track errs by at most 0.07 px each way (above), so its round trip stays below 0.14 px.  Without the check every
    point inside or outside the patch has status 1.  With it every point whose window lies outside the patch is kept; at half 10 (cv2's window) every point
    whose window lies inside is rejected.  At half 4 a 9 x 9 window can find a false match that is itself consistent both ways,
    which no such check can reject (measured: 1 of 20); the test asks for the majority."""
    shift = (1.3, -0.8)
    second = reflk.texture(SEED, ROWS, COLS, shift).copy()
    second[30:70, 40:90] = reflk.texture(99, ROWS, COLS)[30:70, 40:90]
    pts = reflk.grid_points(ROWS, COLS, 16, 6)
    for half, levels in ((10, 3), (4, 1)):
        pyr = [reflk.pyramid(first, levels), reflk.pyramid(second, levels)]
        m = half + 4          # the window, its gradient halo and the motion
        inside = (pts[:, 0] >= 40 + m) & (pts[:, 0] < 90 - m) & (pts[:, 1] >= 30 + m) & (pts[:, 1] < 70 - m)
        outside = (pts[:, 0] < 40 - m) | (pts[:, 0] >= 90 + m) | (pts[:, 1] < 30 - m) | (pts[:, 1] >= 70 + m)
        assert inside.sum() >= 4 and outside.sum() >= 30
        _, st0, _ = reflk.track_problems(pyr, [0], [1], pts[None], [len(pts)], half, max_iter=MAX_ITER)
        nx, st, _, back = reflk.track_problems(pyr, [0], [1], pts[None], [len(pts)], half, max_iter=MAX_ITER, fb_max=0.25)
        assert st0[0][inside].all() and st0[0][outside].all()
        assert st[0][outside].all()
        assert np.abs(back[0][outside] - pts[outside]).max() < 0.25
        rejected = int((st[0][inside] == 0).sum())
        print("half %d: %d of %d points inside the patch rejected" % (half, rejected, inside.sum()))
        assert rejected == inside.sum() if half == 10 else 2 * rejected > inside.sum()
