"""CPU: the seam-free front end's rule on the CPU oracle -- the plain stages on host-padded arrays plus
the unpad (tests/refseam.py).  The numbers below were measured with the oracle; they are conditions, the device's results are
compared against them (tests/test_gpu_seam_free.py), never the other way round."""
import numpy as np
import pytest

import refseam

W = 256


@pytest.fixture(scope="module")
def results():
    P, bits = refseam.fixture()
    return dict(P=P, bits=bits, plain=refseam.front_end(P, bits), seam_free=refseam.front_end(P, bits, seam_free=True))


def _bands(kp):
    """-> (in the left 31-column band, in the right one, within 5 columns of the seam)."""
    x = kp[:, 0]
    return int((x < 31).sum()), int((x >= W - 31).sum()), int(((x < 5) | (x >= W - 5)).sum())


def test_fixture_bytes():
    P, bits = refseam.fixture()
    assert P.shape == (96, 256, 3) and bits.shape == (96, 256)
    assert [int((bits == 1 << k).sum()) for k in range(4)] == [80 * 64] * 4


def test_the_table_of_counts(results):
    plain, sf = results["plain"], results["seam_free"]
    assert [len(k) for k, _ in plain] == [15, 37, 37, 20]
    assert [len(k) for k, _ in sf] == [33, 37, 37, 35]
    all_plain, all_sf = np.concatenate([k for k, _ in plain]), np.concatenate([k for k, _ in sf])
    assert len(all_plain) == 109 and len(all_sf) == 142
    assert _bands(all_plain) == (0, 0, 0)
    assert _bands(all_sf) == (18, 15, 8)
    assert all_sf[:, 0].min() >= 0 and all_sf[:, 0].max() < W


def test_every_plain_keypoint_is_kept_with_its_descriptor(results):
    for (kp, desc), (kp_sf, desc_sf) in zip(results["plain"], results["seam_free"]):
        where = {tuple(p): i for i, p in enumerate(kp_sf.tolist())}
        for p, d in zip(kp.tolist(), desc):
            assert tuple(p) in where
            assert np.array_equal(desc_sf[where[tuple(p)]], d)


@pytest.mark.parametrize("shift", [64, 128, 192])
def test_a_roll_by_whole_sectors_rolls_the_result(results, shift):
    """Rolling P and the masks by k sectors gives, mask for mask, the same keypoints shifted mod 256 in the same order with
    the same descriptors: mask m of the rolled input is mask m - k of the original."""
    P, bits = np.roll(results["P"], shift, axis=1), refseam.sector_masks(96, W)      # (the rolled sectors are sectors again)
    rolled = refseam.front_end(P, bits, seam_free=True)
    for m in range(4):
        kp, desc = results["seam_free"][(m - shift // 64) % 4]
        want = kp.copy()
        want[:, 0] = (want[:, 0] + shift) % W
        assert np.array_equal(rolled[m][0], want)
        assert np.array_equal(rolled[m][1], desc)


def test_a_mask_that_straddles_the_seam_is_the_documented_limit(results):
    """A roll by 37 columns: the masks roll with the image, so mask 3 then covers [229, 256) and [0, 37).  In padded
    coordinates its two pieces lie W apart, so its greedy minimum distance and its maximum are those of two pieces: that mask,
    and only it, may differ from the rolled result."""
    P, bits = np.roll(results["P"], 37, axis=1), refseam.sector_masks(96, W, shift=37)
    rolled = refseam.front_end(P, bits, seam_free=True)
    same = []
    for m in range(4):
        kp, desc = results["seam_free"][m]
        want = kp.copy()
        want[:, 0] = (want[:, 0] + 37) % W
        same.append(np.array_equal(rolled[m][0], want) and np.array_equal(rolled[m][1], desc))
    assert same == [True, True, True, False]


def test_unpad_on_hand_made_values():
    x = np.array([39.5, 40.0, W + 39.96875, W + 40.0, 40.0 - 2.0 ** -10, 41.25, 79.0], np.float32)
    want = np.array([W - 0.5, 0.0, W - 0.03125, 0.0, W - 2.0 ** -10, 1.25, 39.0], np.float32)
    got = refseam.unpad(x, W)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    # a sub-pixel value so close below the halo that + W rounds up to W itself: written as 0
    assert refseam.unpad(np.nextafter(np.float32(40.0), np.float32(0.0)), W) == 0.0


def test_unpad_is_exact_on_the_detectors_grid():
    """Every multiple of 1/32 below W + 80 at W = 1440: the float32 subtraction and the wrap are exact."""
    period = 1440
    k = np.arange((period + 2 * refseam.HALO) * 32, dtype=np.int64)
    x = (k / 32.0).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * 32, k)       # (the inputs are on the grid)
    exact = ((k - refseam.HALO * 32) % (period * 32)) / 32.0
    got = refseam.unpad(x, period)
    assert np.array_equal(got.astype(np.float64), exact)
    assert got.min() == 0.0 and got.max() == period - 1 / 32.0


def test_pad_and_pad0():
    a = np.arange(2 * 50 * 3).reshape(2, 50, 3)
    p = refseam.pad(a)
    assert p.shape == (2, 130, 3)
    assert np.array_equal(p[:, 40:90], a) and np.array_equal(p[:, :40], a[:, 10:]) and np.array_equal(p[:, 90:], a[:, :40])
    b = refseam.pad0(np.ones((2, 3, 50), np.uint32))
    assert b.shape == (2, 3, 130) and b[..., :40].sum() == 0 and b[..., 90:].sum() == 0 and b[..., 40:90].all()
