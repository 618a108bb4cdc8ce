"""CPU: the cyclic-column rule of tests/reflk_cyclic.py on its own -- what the device is then compared
with bit for bit in tests/test_gpu_cyclic.py.  The pyramid's exact roll invariance; the tracker on the periodic shifted
texture (nothing is lost, the planted shift is recovered, today's clamped rule loses or misplaces points on the same scene),
bit equality with tests/reflk.py away from the seam, the near-invariance under rolls, the forward-backward check across the
seam, results written inside [0, W); and the cyclic |du| gate on hand-made pairs."""
import numpy as np
import pytest

import reflk
import reflk_cyclic as rc

ROWS, W, MAX_ITER = 96, 128, 10
# (half, levels, shift, the reference's worst error in px on the 256 grid points: measured once, recorded in DESIGN.md)
SETTINGS = [(4, 1, (0.37, -0.21), 0.07905), (4, 3, (5.3, -3.6), 0.06545), (4, 3, (-5.3, 3.6), 0.07495),
            (10, 3, (5.3, -3.6), 0.02941), (2, 1, (0.37, -0.21), 0.22131)]
ROLL_MEASURED = 0.01468           # the largest move of a result under the rolls below (the rule is not exactly invariant)


def _bits(res):
    x, y, s, e = res
    return (np.float32(x).tobytes(), np.float32(y).tobytes(), int(s), np.float32(e).tobytes())


@pytest.fixture(scope="module")
def scene():
    """The first image, the grid, and per (levels, shift) both pyramids under both rules: built once, never written."""
    s = dict(a=rc.texture(7, ROWS, W), pts=rc.seam_grid(ROWS, W), cache={})

    def pyrs(levels, shift, cyclic=True):
        key = (levels, shift, cyclic)
        if key not in s["cache"]:
            mod = rc if cyclic else reflk
            s["cache"][key] = (mod.pyramid(s["a"], levels), mod.pyramid(rc.texture(7, ROWS, W, shift), levels))
        return s["cache"][key]
    s["pyrs"] = pyrs
    return s


# ---- the texture and the pyramid ----------------------------------------------------------------------------------------------
def test_the_texture_is_periodic_and_its_shift_goes_round():
    a = rc.texture(7, ROWS, W)
    assert a.shape == (ROWS, W) and a.dtype == np.uint8 and a.std() > 20
    assert np.array_equal(rc.texture(7, ROWS, W, (float(W), 0.0)), a)            # one turn
    assert np.array_equal(rc.texture(7, ROWS, W, (5.0, 0.0)), np.roll(a, 5, 1))  # whole columns: a roll
    assert len(rc.seam_grid(ROWS, W)) == 256


@pytest.mark.parametrize("levels,k", [(2, 2), (3, 4), (3, 36), (4, 8), (4, 120)])
def test_pyramid_rolls_with_its_input_byte_for_byte(levels, k):
    rng = np.random.default_rng(levels * 100 + k)
    img = rng.integers(0, 256, (45, W), dtype=np.uint8)
    for row_range in (None, (7, 40)):
        base, rr = rc.pyramid(img, levels, row_range)
        rolled, rr2 = rc.pyramid(np.roll(img, k, 1), levels, row_range)
        assert rr == rr2
        for l in range(levels):
            assert base[l].shape[1] == W >> l
            assert np.array_equal(rolled[l], np.roll(base[l], k >> l, 1)), (l, row_range)
    plain, cyc = reflk.pyramid(img, levels)[0], rc.pyramid(img, levels)[0]     # the two rules differ at the borders only
    assert not np.array_equal(plain[1], cyc[1]) and np.array_equal(plain[1][:, 2:-2], cyc[1][:, 2:-2])


def test_pyramid_refuses_a_width_that_is_no_multiple():
    img = np.zeros((8, 127), np.uint8)
    with pytest.raises(ValueError):
        rc.pyramid(img, 2)
    with pytest.raises(ValueError):
        rc.pyramid(np.zeros((8, 20), np.uint8), 4)        # 20 = 4 * 5: three levels, not four
    assert len(rc.pyramid(np.zeros((8, 20), np.uint8), 3)[0]) == 3
    assert len(rc.pyramid(img, 1)[0]) == 1
    with pytest.raises(ValueError):                       # 5 columns on the top level, the template needs 2 * 2 + 3
        rc.track(rc.pyramid(np.zeros((8, 20), np.uint8), 3), rc.pyramid(np.zeros((8, 20), np.uint8), 3), 1.0, 1.0, 2)


# ---- the tracker ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half,levels,shift,measured", SETTINGS)
def test_no_point_is_lost_and_the_shift_is_recovered_around_the_circle(scene, half, levels, shift, measured):
    pa, pb = scene["pyrs"](levels, shift)
    qa, qb = scene["pyrs"](levels, shift, cyclic=False)
    worst, crossed, plain_bad = 0.0, 0, 0
    for p in scene["pts"]:
        x, y, st, _ = rc.track(pa, pb, p[0], p[1], half, MAX_ITER)
        assert st == 1, p
        assert 0.0 <= float(x) < W
        ex = rc.cyclic_distance(x, (float(p[0]) + shift[0]) % W, W)
        worst = max(worst, float(np.hypot(ex, float(y) - float(p[1]) - shift[1])))
        crossed += abs(float(x) - float(p[0])) > W / 2
        x, y, st, _ = reflk.track(qa, qb, p[0], p[1], half, MAX_ITER)
        plain_bad += (not st) or np.hypot(float(x) - float(p[0]) - shift[0], float(y) - float(p[1]) - shift[1]) > 0.15
    print("half %d, %d levels, shift %s: worst error %.5f px (measured %.5f), %d crossed the seam; clamped rule: %d lost or "
          "beyond 0.15 px" % (half, levels, shift, worst, measured, crossed, plain_bad))
    assert worst <= 2.0 * measured
    assert plain_bad >= 1                                  # today's rule loses or misplaces some of the same points
    if abs(shift[0]) > 4:
        assert crossed >= 8                                # the columns within |shift| of the seam, 8 rows each


def test_interior_points_equal_the_plain_rule_bit_for_bit(scene):
    """x = 40 .. 88 at width 128, half 4, 3 levels: no window touches a border on any level, so the clamp and the wrap never
    act and the two rules are the same arithmetic."""
    pa, pb = scene["pyrs"](3, (5.3, -3.6))
    qa, qb = scene["pyrs"](3, (5.3, -3.6), cyclic=False)
    inner = [p for p in scene["pts"] if 40 <= p[0] <= 88]
    assert len(inner) == 13 * 8
    for p in inner:
        assert _bits(rc.track(pa, pb, p[0], p[1], 4, MAX_ITER)) == _bits(reflk.track(qa, qb, p[0], p[1], 4, MAX_ITER)), p


@pytest.mark.parametrize("k", [1, 37, 64, 127])
def test_rolling_both_images_changes_no_status_and_barely_a_result(scene, k):
    """Not exact: gq / 32 + dx rounds differently for a wrapped and an unwrapped gq."""
    a, shift = scene["a"], (5.3, -3.6)
    pa, pb = scene["pyrs"](3, shift)
    ra, rb = rc.pyramid(np.roll(a, k, 1), 3), rc.pyramid(np.roll(rc.texture(7, ROWS, W, shift), k, 1), 3)
    worst = 0.0
    for p in scene["pts"][::2]:
        x, y, st, _ = rc.track(pa, pb, p[0], p[1], 4, MAX_ITER)
        x2, y2, st2, _ = rc.track(ra, rb, np.float32((float(p[0]) + k) % W), p[1], 4, MAX_ITER)
        assert st == st2 == 1
        worst = max(worst, rc.cyclic_distance(x2, (float(x) + k) % W, W), abs(float(y2) - float(y)))
    print("roll %d: largest move %.5f px (measured over all rolls and points: %.5f)" % (k, worst, ROLL_MEASURED))
    assert worst <= 2.0 * ROLL_MEASURED


@pytest.mark.parametrize("half,levels,shift", [s[:3] for s in SETTINGS[:3]])
def test_forward_backward_check_keeps_the_points_at_the_seam(scene, half, levels, shift):
    near = np.array([p for p in scene["pts"] if p[0] < 12 or p[0] >= W - 12], np.float32)
    assert len(near) == 48
    nx, st, _, bk = rc.track_problems(list(scene["pyrs"](levels, shift)), [0], [1], near[None], [len(near)], half, MAX_ITER,
                                      fb_max=0.25)
    assert st.all()
    back = [np.hypot(rc.cyclic_distance(bk[0, i, 0], near[i, 0], W), float(bk[0, i, 1]) - float(near[i, 1])) for i in range(48)]
    print("way back, half %d, %d levels, shift %s: largest distance %.4f px" % (half, levels, shift, max(back)))
    assert max(back) <= 0.25
    if abs(shift[0]) > 4:                                  # (some of them did cross)
        assert (np.abs(nx[0, :, 0].astype(np.float64) - near[:, 0]) > W / 2).any()


def test_results_are_written_inside_the_period(scene):
    a = scene["a"]
    same = rc.pyramid(a, 1)
    x, y, st, err = rc.track(same, same, np.float32(W - 1 / 64), np.float32(40), 4, MAX_ITER)
    assert st == 1 and float(x) == 0.0 and float(y) == 40.0 and float(err) == 0.0     # rounds to column W: written as 0
    assert float(rc.wrap_x(-1e-12, W)) == 0.0              # W - 1e-12 rounds to W in float32
    assert float(rc.wrap_x(127.99999999, W)) == 0.0
    assert float(rc.wrap_x(float(W), W)) == 0.0 and float(rc.wrap_x(-0.25, W)) == 127.75
    assert float(rc.wrap_x(3.0 * W + 5.5, W)) == 5.5 and float(rc.wrap_x(127.99999, W)) == float(np.float32(127.99999))
    # a start beyond the period is a position on the circle; a LOST point's guess is written inside it as well
    flat = rc.pyramid(np.full((ROWS, W), 9, np.uint8), 1)
    x, y, st, _ = rc.track(flat, flat, np.float32(W + 3.5), np.float32(40), 4, MAX_ITER)
    assert st == 0 and float(x) == 3.5                     # no texture: lost with its guess, wrapped
    moved = rc.pyramid(rc.texture(7, ROWS, W, (0.37, -0.21)), 1)
    assert _bits(rc.track(same, moved, np.float32(W + 3.5), np.float32(40), 4, MAX_ITER)) == \
        _bits(rc.track(same, moved, np.float32(3.5), np.float32(40), 4, MAX_ITER))
    for bad in (np.float32(2.0 ** 36), np.float32(-2.0 ** 36)):   # |32 x + 0.5| >= 2^40: no position at all
        assert rc.track(same, same, bad, np.float32(40), 4, MAX_ITER)[2] == 0
    assert rc.track(same, same, np.float32(5), np.float32(-3), 4, MAX_ITER)[2] == 0    # the rows still have an edge


# ---- the gate -------------------------------------------------------------------------------------------------------------------
def test_cyclic_gate_on_hand_made_pairs():
    Wp, g = 1440, 90.0
    a = np.array([10.0, 1435.0, 1400.0, 0.0, 90.0, 0.0, 1350.0, 1349.96875, 700.0, 700.0, 50.0], np.float32)
    b = np.array([1430.0, 3.0, 20.0, 90.0, 0.0, 1350.0, 0.0, 0.0, 790.03125, 100.0, 1400.03125], np.float32)
    #             straddle  straddle  straddle  d = g  d = g  W - d = g  same    just out   just out  far  W - d just in
    want = np.array([1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1], bool)
    assert np.array_equal(rc.du_gate(a, b, g, Wp), want)
    assert np.array_equal(rc.du_gate(b, a, g, Wp), want)                      # symmetric
    plain = rc.du_gate_plain(a, b, g)
    assert np.array_equal(plain, np.array([0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0], bool))
    assert (rc.du_gate(a, b, g, Wp) | ~plain).all()                            # the cyclic gate only adds
    for off in (0.0, -1.0):                                                    # the disabled gate passes everything
        assert rc.du_gate(a, b, off, Wp).all() and rc.du_gate_plain(a, b, off).all()
    # exact at the boundaries for a fractional bound: one float32 step beyond is out
    g2 = 37.5
    u = np.float32(1000.0)
    assert rc.du_gate([u], [np.float32(1037.5)], g2, Wp)[0] and not rc.du_gate([u], [np.nextafter(np.float32(1037.5), np.float32(2000))], g2, Wp)[0]
    assert rc.du_gate([np.float32(1420.0)], [np.float32(17.5)], g2, Wp)[0]     # W - d = 37.5
    assert not rc.du_gate([np.float32(1420.0)], [np.nextafter(np.float32(17.5), np.float32(100))], g2, Wp)[0]
