"""CPU: tests/refdense_wide.py -- the numpy statement of dense omnistereo with D = 16 .. 256 disparities
-- pinned from outside: at D = 64 it is refdense / refdense8; planted integer shifts beyond 63 rows, the winner k* = 255 among
them; ray-cast truth of a room whose walls stand nearer than 64 disparities reach; the sign bit of S; and the host-side pieces
that need no GPU (the scratch layout, _lib.dense_disparities).  The thresholds are conditions on the reference alone; the
measured values stand beside them.  The scenes are shared with tests/test_gpu_dense_wide.py, computed once per session."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refdense  # noqa: E402
import refdense8  # noqa: E402
import refdense_wide  # noqa: E402
from dense_wide_scenes import near_room_scene  # noqa: E402
from test_gpu_dense import _frames, _texture  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vo_single_camera_sos_amd", "csrc")
OPTS = dict(P1=8, P2=48, uniqueness=15, lr_max=1)
# (D, shift, min_disparity) at 300 x 24: the issue's table, then its case with k* = 255
PLANTED = [(128, 64, 1), (128, 100, 1), (128, 127, 1), (256, 100, 1), (256, 200, 1), (256, 254, 1), (256, 255, 1), (240, 239, 1),
           (16, 15, 1), (256, 255, 0)]
_CACHE = {}


@pytest.mark.parametrize("shape", ((12, 9), (70, 5)), ids=lambda s: "%dx%d" % s)
def test_sixty_four_disparities_are_refdense_and_refdense8(shape):
    top, bot = _frames(*shape)
    for cyclic in (False, True):
        for t, b in zip(top, bot):
            ct, cb = refdense.census(t, cyclic), refdense.census(b, cyclic)
            C = refdense_wide.cost_volume(ct, cb, 1, 64)
            assert np.array_equal(C, refdense.cost_volume(ct, cb, 1))
            for paths in (4, 8):
                S = refdense_wide.aggregate(C, 8, 48, paths, cyclic)
                assert np.array_equal(S, refdense8.aggregate(C, 8, 48, paths, cyclic))
                assert np.array_equal(refdense_wide.select(S, 1, 15, 1), refdense.select(S, 1, 15, 1))
                assert np.array_equal(refdense_wide.select(S, 1, 0, -1), refdense.select(S, 1, 0, -1))
            want4 = refdense.dense_stereo(t, b, None, min_disparity=0, cyclic=cyclic, want_volume=True, **OPTS)
            want8 = refdense8.dense_stereo(t, b, None, min_disparity=0, cyclic=cyclic, want_volume=True, paths=8, **OPTS)
            for paths, want in ((4, want4), (8, want8)):
                got = refdense_wide.dense_stereo(t, b, None, min_disparity=0, cyclic=cyclic, want_volume=True, paths=paths, **OPTS)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    with pytest.raises(ValueError):
        refdense_wide.cost_volume(ct, cb, 0, 72)


def planted(shift, rows=300, cols=24):
    """Section 37's construction: top = img[: rows], bot = img[shift : shift + rows] of one texture seeded from rows + shift."""
    img = _texture(np.random.default_rng(rows + shift), rows + shift, cols)
    return np.ascontiguousarray(img[:rows]), np.ascontiguousarray(img[shift:shift + rows])


def planted_share(d16, shift):
    """The share of the reachable pixels (r >= shift) within half a row of 16 * shift."""
    return float((np.abs(d16[shift:].astype(np.int32) - 16 * shift) <= 8).mean())


@pytest.mark.parametrize("case", PLANTED, ids=lambda c: "D%d_shift%d_d%d" % c)
def test_planted_integer_shift_beyond_63_rows_is_found(case):
    """At least 0.97 of the reachable pixels lie within half a row of the planted shift.  Measured, in PLANTED's order:
    0.9966, 0.9973, 0.9983 (D = 128); 0.9973, 0.9958, 0.9918, 0.9917 (D = 256); 0.9939 (D = 240, shift 239); 0.9988 (D = 16,
    shift 15); 0.9926 (D = 256, shift 255, min_disparity 0: 1 072 of the 7 200 pixels are kept with k* = 255)."""
    D, shift, d0 = case
    top, bot = planted(shift)
    d16, S = refdense_wide.dense_stereo(top, bot, None, min_disparity=d0, disparities=D, want_volume=True, **OPTS)
    share = planted_share(d16, shift)
    print("planted shift %d, D %d, min_disparity %d: %.4f" % (shift, D, d0, share))
    assert share >= 0.97
    if shift - d0 == 255:
        kept = int((refdense_wide.winners(S, d0, 15, 1) == 255).sum())
        print("kept with k* = 255: %d" % kept)
        assert kept >= 500


@pytest.mark.parametrize("shift", (100, 127, 200, 254, 255))
def test_sixty_four_disparities_find_none_of_the_far_shifts(shift):
    top, bot = planted(shift)
    assert planted_share(refdense_wide.dense_stereo(top, bot, None, min_disparity=1, disparities=64, **OPTS), shift) == 0.0
    assert planted_share(refdense.dense_stereo(top, bot, None, min_disparity=1, **OPTS), shift) == 0.0


def near_room_map(D):
    """refdense_wide's d16 of the scene: min_disparity 0, the default options, four paths, under the top view's mask."""
    if ("map", D) not in _CACHE:
        _, _, gray, valid, _ = near_room_scene()
        _CACHE["map", D] = refdense_wide.dense_stereo(gray[0], gray[1], valid[0].astype(np.uint8), min_disparity=0, disparities=D, **OPTS)
    return _CACHE["map", D]


# refdense_wide's share "valid and within one row" at D = 128 on the comparable pixels with truth in [65, 127), as measured
NEAR_SHARE_128 = 0.3239


def test_ray_cast_truth_of_a_room_nearer_than_64_disparities():
    """The walls stand 0.25 to 0.4 m away; at 1440 columns 64 disparities end at 0.36 m.  Comparable pixels with truth in
    [65, 127): D = 64 has none valid and within one row of the truth (its largest value is 63.0 rows), D = 128 at least its
    measured share less the project's margin of 0.03 for these scenes.  On the pixels with truth below 63, D = 128 loses at
    most 0.02 of D = 64's valid share and 0.01 of its share within one row.
    Measured: 39 852 comparable pixels in [65, 127): D = 64 valid 0.4235, valid and within one row 0.0000 (median error 46.4
    rows); D = 128 valid 0.5584, valid and within one row 0.3239 (0.5801 of the valid, median error 0.8134 row).  Truth below
    63 (80 185 pixels): D = 64 valid 0.7773, of those within one row 0.7068, median 0.6047; D = 128 valid 0.7690, within one
    row 0.7066, median 0.6047.  The absolute figures are low: the 640 x 480 frames
    are oversampled at this width and the walls are slanted steeply; the contrast is what the test is for."""
    _, _, _, valid, true = near_room_scene()
    assert true.shape == (146, 1440)
    fig = {}
    for D in (64, 128):
        d16 = near_room_map(D)
        fig[D] = (refdense_wide.accuracy(d16, true, valid[0], valid[1], 65.0, 127.0), refdense_wide.accuracy(d16, true, valid[0], valid[1], 0.0, 63.0))
        print("D %d: truth in [65, 127): %d comparable, %.4f valid, %.4f valid and within 1 row, %.4f of the valid, median %.4f" % ((D,) + fig[D][0]))
        print("D %d: truth below 63: %d comparable, %.4f valid, %.4f valid and within 1 row, %.4f of the valid, median %.4f" % ((D,) + fig[D][1]))
    assert fig[64][0][0] == fig[128][0][0] > 30000
    assert fig[64][0][2] == 0.0 and fig[64][0][1] > 0.2            # confident wrong depth, not missing depth
    assert fig[128][0][2] >= NEAR_SHARE_128 - 0.03
    assert fig[128][1][1] >= fig[64][1][1] - 0.02 and fig[128][1][3] >= fig[64][1][3] - 0.01
    low = refdense.accuracy(near_room_map(64), true, valid[0], valid[1])      # refdense's own figures of the same map
    assert low[0] == fig[64][1][0] and low[1] == fig[64][1][1] and low[2] == fig[64][1][3]


def sign_bit_volume(cyclic):
    """(img, (d16, S [300, 300, 128])) of the sign-bit case (also tests/test_gpu_dense_wide.py): top = bot = a 300 x 300
    texture, min_disparity 0, P1 = P2 = 8127, eight paths, D = 128."""
    if ("sign", cyclic) not in _CACHE:
        img = _texture(np.random.default_rng(5), 300, 300)
        _CACHE["sign", cyclic] = (img, refdense_wide.dense_stereo(img, img, None, min_disparity=0, P1=8127, P2=8127, cyclic=cyclic,
                                                                  want_volume=True, paths=8, disparities=128))
    return _CACHE["sign", cyclic]


@pytest.mark.parametrize("cyclic", (False, True), ids=("clamped", "cyclic"))
def test_S_uses_its_sign_bit_and_stays_16_bits(cyclic):
    """S above 32767 on at least 0.4 of the volume clamped, 0.9 cyclic, and never above 65528.  Measured: 0.618 and 0.984 of the
    volume, maxima 56104 and 57943."""
    _, (_, S) = sign_bit_volume(cyclic)
    share = (S > 32767).mean()
    print("cyclic %d: share above 32767 %.3f, max %d" % (cyclic, share, S.max()))
    assert S.dtype == np.uint16 and S.shape == (300, 300, 128) and S.max() <= 65528
    assert share >= (0.9 if cyclic else 0.4)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_the_scratch_layout_is_the_documented_one(tmp_path):
    """csrc/dense_wide_scratch.h (the function dense_wide.hip calls), built by the host compiler: tests/dense_wide_scratch_check.cpp
    places it at n = 2, rows = 3, cols = 5, D = 48 against offsets worked out by hand, and checks the 22 + 3 D bytes per pixel
    that include/sosvo_dense_wide.h documents at the working size."""
    exe = str(tmp_path / "dense_wide_scratch_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, "-o", exe,
                           os.path.join(HERE, "dense_wide_scratch_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


def test_dense_disparities_refuses_every_bad_value():
    from vo_single_camera_sos_amd import _lib
    from vo_single_camera_sos_amd._lib import DenseOptions, dense_disparities
    assert [dense_disparities(D) for D in range(16, 257, 16)] == list(range(16, 257, 16)) == list(refdense_wide.DISPARITIES)
    assert dense_disparities(240, 8, DenseOptions(P2=8127)) == 240 and dense_disparities(64, 4, DenseOptions(P2=8191)) == 64
    assert (_lib.DENSE_WIDE_MIN_DISPARITIES, _lib.DENSE_WIDE_MAX_DISPARITIES, _lib.DENSE_DISPARITIES) == (16, 256, 64)
    for D in (0, 8, 15, 17, 24, 63, 65, 100, 255, 257, 272, 512, -16, -64, 64.0, "64", None, True, False, (64,)):
        with pytest.raises(ValueError):
            dense_disparities(D)
    for kw in (dict(paths=6), dict(paths=8, options=DenseOptions(P1=0, P2=8128)), dict(paths=8, options=dict(P2=8191)), dict(paths="4")):
        with pytest.raises(ValueError):
            dense_disparities(128, **kw)
    assert DenseOptions._fields == ("min_disparity", "P1", "P2", "uniqueness", "lr_max", "cyclic")
