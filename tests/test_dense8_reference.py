"""CPU: tests/refdense8.py -- the numpy statement of eight-path aggregation -- pinned from outside: the
skewed-line form against a per-pixel loop over predecessors, the one-column cases, planted integer shifts, ray-cast truth next
to the four-path figures of the same run, the sign bit of S, and that the GPU tests' inputs can tell the forms apart.  The
thresholds are conditions on the reference alone; the measured values stand beside them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refdense  # noqa: E402
import refdense8  # noqa: E402
from test_gpu_dense import _frames, _texture  # noqa: E402

OPTS = dict(P1=8, P2=48, uniqueness=15, lr_max=1)


def _naive_diagonal(C, P1, P2, dr, dc, cyclic):
    """The definition of include/sosvo.h pixel by pixel: the predecessor of (r, c) is (r - dr, c - dc); the path starts where
    r - dr leaves [0, rows), clamped also where c - dc leaves [0, cols); cyclic the predecessor's column is (c - dc) mod cols."""
    rows, cols = C.shape[:2]
    C = C.astype(np.int64)
    L = np.zeros_like(C)
    for r in (range(rows) if dr > 0 else range(rows - 1, -1, -1)):
        for c in range(cols):
            pr, pc = r - dr, c - dc
            if not 0 <= pr < rows or (not cyclic and not 0 <= pc < cols):
                L[r, c] = C[r, c]
                continue
            Lp = L[pr, pc % cols]
            m = Lp.min()
            for k in range(refdense.D):
                best = min(Lp[k], m + P2)
                if k > 0:
                    best = min(best, Lp[k - 1] + P1)
                if k < refdense.D - 1:
                    best = min(best, Lp[k + 1] + P1)
                L[r, c, k] = C[r, c, k] + best - m
    return L


def _random_volume(seed, rows, cols):
    return np.random.default_rng(seed).integers(0, 65, (rows, cols, refdense.D)).astype(np.uint8)


@pytest.mark.parametrize("P", ((8, 48), (0, 0)), ids=lambda p: "P%d_%d" % p)
@pytest.mark.parametrize("shape", ((7, 5), (5, 7)), ids=lambda s: "%dx%d" % s)
def test_skewed_lines_equal_the_per_pixel_definition(shape, P):
    C = _random_volume(shape[0], *shape)
    for dr, dc in refdense8.DIAGONALS:
        for cyclic in (False, True):
            got, want = refdense8.diagonal(C, P[0], P[1], dr, dc, cyclic), _naive_diagonal(C, P[0], P[1], dr, dc, cyclic)
            assert np.array_equal(got, want), (dr, dc, cyclic, np.argwhere(got != want)[:5])


def test_one_column_cyclic_is_vertical_and_clamped_is_the_cost():
    C = _random_volume(3, 9, 1)
    Ci = C.astype(np.int32)
    down, up = refdense._path(Ci, 8, 48), refdense._path(Ci[::-1], 8, 48)[::-1]
    assert not np.array_equal(down, Ci) and not np.array_equal(down, up)
    for dr, dc in refdense8.DIAGONALS:
        assert np.array_equal(refdense8.diagonal(C, 8, 48, dr, dc, True), down if dr > 0 else up)
        assert np.array_equal(refdense8.diagonal(C, 8, 48, dr, dc, False), Ci)


def test_four_paths_are_refdense():
    C = _random_volume(4, 12, 9)
    for cyclic in (False, True):
        assert np.array_equal(refdense8.aggregate(C, 8, 48, paths=4, cyclic=cyclic), refdense.aggregate(C, 8, 48))
    img = _texture(np.random.default_rng(9), 40, 12)
    assert np.array_equal(refdense8.dense_stereo(img[:30], img[10:], **OPTS), refdense.dense_stereo(img[:30], img[10:], **OPTS))
    with pytest.raises(ValueError):
        refdense8.aggregate(C, 8, 48, paths=6)


@pytest.mark.parametrize("k", (1, 5, 40, 63))
@pytest.mark.parametrize("shape", ((96, 40), (130, 33)), ids=lambda s: "%dx%d" % s)
def test_planted_integer_shift_is_found_with_eight_paths(shape, k):
    """The construction of test_dense_reference.test_planted_integer_shift_is_found; at least 0.97 of the reachable pixels
    within half a row of 16 k, clamped and cyclic.  Measured (k = 1, 5, 40, 63):
    96 x 40 clamped 1.0000, 0.9975, 0.9888, 0.9894; cyclic 1.0000, 0.9975, 0.9888, 0.9886;
    130 x 33 clamped 1.0000, 0.9990, 0.9926, 0.9882; cyclic 1.0000, 0.9990, 0.9916, 0.9900.
    (Cyclic here is the flag as the device has it: census taps and diagonal predecessors both wrap.  With clamped taps and
    wrapped predecessors the cyclic figures are 0.9884, 0.9879 at 96 x 40 and 0.9988, 0.9916, 0.9878 at 130 x 33.)"""
    rows, cols = shape
    img = _texture(np.random.default_rng(rows + k), rows + k, cols)
    for cyclic in (False, True):
        d16 = refdense8.dense_stereo(img[:rows], img[k:k + rows], None, min_disparity=1, cyclic=cyclic, paths=8, **OPTS)
        share = (np.abs(d16[k:].astype(np.int32) - 16 * k) <= 8).mean()
        print("planted shift %d at %dx%d, cyclic %d: %.4f" % (k, rows, cols, cyclic, share))
        assert share >= 0.97


def _ray_cast_figures(width, room, ksize):
    """The scene and the call of test_dense_reference._ray_cast_case (one frame at t = (200, -300, 0), noise 2, the CPU oracle's
    unwrap and median, min_disparity 0, clamped) -> {paths: refdense.accuracy's four figures} for 4 and 8 paths."""
    import oracle
    from vo_single_camera_sos_amd import synthetic
    from vo_single_camera_sos_amd.omnistereo.gum import synthetic_gums
    from vo_single_camera_sos_amd.omnistereo.panorama import Panorama
    gs = synthetic_gums()
    for m in (gs.top_model, gs.bot_model):
        m.panorama = Panorama(m, width=width)
    gs.make_annulus_masks((480, 640))
    t = np.array([200.0, -300.0, 0.0])
    omni = synthetic.render_omni(gs, room, np.eye(3), t, 2.0, np.random.default_rng(1))
    white = np.full_like(omni, 255)
    gray, valid = [], []
    for m in (gs.top_model, gs.bot_model):
        mx, my = m.panorama.float32_maps()
        gray.append(oracle.median_gray(oracle.unwrap(omni, m.mask, mx, my), ksize))
        valid.append(oracle.median_gray(oracle.unwrap(white, m.mask, mx, my), 0) == 255)
    true = refdense.true_disparity(gs, room, t)
    out = {}
    for paths in (4, 8):
        d16 = refdense8.dense_stereo(gray[0], gray[1], valid[0].astype(np.uint8), min_disparity=0, paths=paths, **OPTS)
        out[paths] = refdense.accuracy(d16, true, valid[0], valid[1])
        print("%d paths: %d comparable, %.4f valid, %.4f within 1 row, median %.4f" % ((paths,) + out[paths]))
    return out


def test_ray_cast_truth_of_the_default_room_with_eight_paths():
    """Panorama(width=480), Room(seed=3), ksize 0: the four-path conditions, >= 0.95 valid, >= 0.97 within 1 row, median <= 0.25.
    Measured: 0.9831 / 0.9908 / 0.1747 (four paths in the same run: 0.9830 / 0.9902 / 0.1808)."""
    from vo_single_camera_sos_amd import synthetic
    fig = _ray_cast_figures(480, synthetic.Room(seed=3), 0)
    _, share, within, med = fig[8]
    assert fig[8][0] == fig[4][0] == 21675
    assert share >= 0.95 and within >= 0.97 and med <= 0.25


def test_ray_cast_truth_of_a_near_room_gains_from_eight_paths():
    """Room(seed=3, half_x=(500, 1500), half_y=(400, 2500)) at width 640, ksize 11, where the four-path map is weakest: the share
    within 1 row at least the four-path share of the same run + 0.005, the median no larger, the valid share no more than
    0.005 lower.  Measured: four paths 0.9024 / 0.9056 / 0.3000, eight paths 0.9016 / 0.9162 / 0.2822."""
    from vo_single_camera_sos_amd import synthetic
    fig = _ray_cast_figures(640, synthetic.Room(seed=3, half_x=(500.0, 1500.0), half_y=(400.0, 2500.0)), 11)
    (_, share4, within4, med4), (_, share8, within8, med8) = fig[4], fig[8]
    assert within8 >= within4 + 0.005 and med8 <= med4 and share8 >= share4 - 0.005


def sign_bit_volume(cyclic):
    """S [300, 300, 64] of the sign-bit case (also tests/test_gpu_dense8.py): top = bot = a 300 x 300 texture, min_disparity 0,
    P1 = P2 = 8127."""
    img = _texture(np.random.default_rng(5), 300, 300)
    return img, refdense8.dense_stereo(img, img, None, min_disparity=0, P1=8127, P2=8127, cyclic=cyclic, want_volume=True, paths=8)


@pytest.mark.parametrize("cyclic", (False, True), ids=("clamped", "cyclic"))
def test_S_uses_its_sign_bit_and_stays_16_bits(cyclic):
    """S above 32767 (what a signed 16-bit load would turn negative) on at least 0.4 of the volume clamped, 0.9 cyclic, and never
    above 65528.  Measured: 0.507 and 0.969 of the volume, maxima 45863 and 51638."""
    _, (_, S) = sign_bit_volume(cyclic)
    share = (S > 32767).mean()
    print("cyclic %d: share above 32767 %.3f, max %d" % (cyclic, share, S.max()))
    assert S.dtype == np.uint16 and S.max() <= 65528
    assert share >= (0.9 if cyclic else 0.4)


@pytest.mark.parametrize("shape", ((12, 9), (70, 5), (5, 70)), ids=lambda s: "%dx%d" % s)
def test_the_gpu_inputs_tell_the_forms_apart(shape):
    """On the frames of test_gpu_dense._frames, min_disparity 0: a device that ran the four paths twice, took the wrong column
    form or selected from the four-path volume would differ from refdense8.  Asserted: the eight-path S differs from twice the
    four-path S on more than half the volume, clamped and cyclic, under the option set (8127, 8127, 99, 63) of the GPU test
    (measured 0.986 to 0.994); under the default set (8, 48, 15, 1) clamped and cyclic S differ (0.06 to 0.77) and d16 differs
    between 4 and 8 paths (0.12 to 0.23).  Under the default set the first share is 0.530 / 0.496 at 12 x 9, 0.772 / 0.745 at
    70 x 5 and 0.711 / 0.700 at 5 x 70 (clamped / cyclic; the constant frame, 0.39 at 12 x 9, pulls it down): printed
    only.  With P1 = P2 = 0 every L is C and S8 = 2 S4 exactly, so that set tells nothing here."""
    top, bot = _frames(*shape)

    def run(paths, cyclic, P1, P2, uniq, lr_max):
        got = [refdense8.dense_stereo(t, b, None, 0, P1, P2, uniq, lr_max, cyclic, True, paths) for t, b in zip(top, bot)]
        return np.stack([g[0] for g in got]), np.stack([g[1] for g in got]).astype(np.int64)
    S8 = {}
    for cyclic in (False, True):
        stiff = (run(8, cyclic, 8127, 8127, 99, 63)[1] != 2 * run(4, cyclic, 8127, 8127, 99, 63)[1]).mean()
        (d4, S4), (d8, S8[cyclic]) = run(4, cyclic, 8, 48, 15, 1), run(8, cyclic, 8, 48, 15, 1)
        doubled, maps = (S8[cyclic] != 2 * S4).mean(), (d8 != d4).mean()
        print("%dx%d cyclic %d: S8 != 2 S4 on %.3f (P 8127) and %.3f (P 8, 48), d16 differs on %.3f" % (shape + (cyclic, stiff, doubled, maps)))
        assert stiff > 0.5 and maps > 0
    forms = (S8[False] != S8[True]).mean()
    print("%dx%d: clamped != cyclic on %.3f" % (shape + (forms,)))
    assert forms > 0
