"""CPU: tests/refdense.py -- the numpy statement of the dense stereo algorithm -- pinned against outside
truth: planted integer shifts and ray-cast disparities of synthetic.Room; and the host-side pieces that need no GPU
(DenseOptions, the reference's zero-is-invalid map, the .pcd writer).  The thresholds are conditions on the reference alone;
the measured values stand beside them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refdense  # noqa: E402

OPTS = dict(P1=8, P2=48, uniqueness=15, lr_max=1)


def _texture(rng, rows, cols):
    a = rng.integers(0, 256, (rows + 2, cols + 2)).astype(np.float64)
    return ((a[:-2, 1:-1] + a[2:, 1:-1] + a[1:-1, :-2] + a[1:-1, 2:] + 2 * a[1:-1, 1:-1]) / 6.0).astype(np.uint8)


@pytest.mark.parametrize("k", (1, 5, 40, 63))
@pytest.mark.parametrize("shape", ((96, 40), (130, 33)), ids=lambda s: "%dx%d" % s)
def test_planted_integer_shift_is_found(shape, k):
    """bot = img[k : k + rows], top = img[: rows]: among the reachable pixels (r >= k) at least 0.97 lie within half a row of
    16 k (the parabola moves an exact integer match by up to half a row unless k* is 0 or 63).
    Measured: 96 x 40: 1.0000, 0.9973, 0.9920, 0.9894; 130 x 33: 1.0000, 0.9995, 0.9939, 0.9896 (k = 1, 5, 40, 63)."""
    rows, cols = shape
    img = _texture(np.random.default_rng(rows + k), rows + k, cols)
    d16 = refdense.dense_stereo(img[:rows], img[k:k + rows], None, min_disparity=1, **OPTS)
    share = (np.abs(d16[k:].astype(np.int32) - 16 * k) <= 8).mean()
    print("planted shift %d at %dx%d: %.4f" % (k, rows, cols, share))
    assert share >= 0.97


def _ray_cast_case(width, room, ksize):
    """-> (d16, true disparity, the two views' masks) of one frame rendered at pose t = (200, -300, 0), noise 2, through the CPU
    oracle's unwrap and median; true disparity = baseline / (rho * pixel_size) with rho from Room.cast along the top bearings."""
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
    d16 = refdense.dense_stereo(gray[0], gray[1], valid[0].astype(np.uint8), min_disparity=0, **OPTS)
    return d16, refdense.true_disparity(gs, room, t), valid


def test_ray_cast_truth_of_the_default_room():
    """Panorama(width=480) (49 rows), Room(seed=3), ksize 0.  Required: >= 0.95 of the comparable pixels valid, >= 0.97 of those
    within 1 row of the truth, median error <= 0.25 row.  Measured: 21 675 comparable pixels (true disparities 1.7 to 3.0 rows),
    0.9830 valid, 0.9902 within 1 row, median 0.1808."""
    from vo_single_camera_sos_amd import synthetic
    d16, true, valid = _ray_cast_case(480, synthetic.Room(seed=3), 0)
    assert d16.shape == (49, 480)
    comparable, share, within, med = refdense.accuracy(d16, true, valid[0], valid[1])
    print("default room: %d comparable, %.4f valid, %.4f within 1 row, median %.4f"
          % (comparable, share, within, med))
    assert share >= 0.95 and within >= 0.97 and med <= 0.25


def test_ray_cast_truth_of_a_near_room():
    """The harder case for the record: Room(seed=3, half_x=(500, 1500), half_y=(400, 2500)) at width 640 (65 rows), ksize 11;
    occlusions and the floor's slant lower the figures.  Asserted with the issue's 0.03 margins below its prototype's 0.902 valid and
    0.906 within 1 row; the median is printed only.  Measured: 33 431 comparable pixels (true disparities 4.9 to 19.0 rows), 0.9024
    valid, 0.9056 within 1 row, median 0.3000."""
    from vo_single_camera_sos_amd import synthetic
    d16, true, valid = _ray_cast_case(640, synthetic.Room(seed=3, half_x=(500.0, 1500.0), half_y=(400.0, 2500.0)), 11)
    assert d16.shape == (65, 640)
    comparable, share, within, med = refdense.accuracy(d16, true, valid[0], valid[1])
    print("near room: %d comparable, %.4f valid, %.4f within 1 row, median %.4f"
          % (comparable, share, within, med))
    assert share >= 0.902 - 0.03 and within >= 0.906 - 0.03


def test_dense_options_refuse_every_bad_value():
    from vo_single_camera_sos_amd._lib import DenseOptions
    o = DenseOptions()
    assert tuple(o) == (1, 8, 48, 15, 1, False) and o.flags == 0 and DenseOptions(cyclic=True).flags == 1
    assert DenseOptions(P1=0, P2=0) == (1, 0, 0, 15, 1, False)          # the reference's tuner: no smoothness
    assert DenseOptions(min_disparity=1024, P1=8191, P2=8191, uniqueness=99, lr_max=-1).lr_max == -1
    assert DenseOptions.of(None) == o and DenseOptions.of(dict(P2=100)).P2 == 100 and DenseOptions.of(o) is o
    assert hash(o) == hash(DenseOptions())
    bad = [dict(min_disparity=-1), dict(min_disparity=1025), dict(min_disparity=1.5), dict(min_disparity=None), dict(P1=-1),
           dict(P1=49), dict(P2=8192), dict(P1=9000, P2=9000), dict(P1="8"), dict(P2=float("nan")), dict(uniqueness=-1),
           dict(uniqueness=100), dict(uniqueness=15.5), dict(uniqueness=True), dict(lr_max=0.5), dict(lr_max=None),
           dict(lr_max=1 << 31)]
    for kw in bad:
        with pytest.raises(ValueError):
            DenseOptions(**kw)
    with pytest.raises(ValueError):
        DenseOptions.of(dict(p1=3))
    with pytest.raises(ValueError):
        DenseOptions.of(7)
    from vo_single_camera_sos_amd._lib import StepOptions
    assert "dense" not in StepOptions._fields


def test_zero_is_invalid_exactly_where_d16_is_minus_one():
    """The host mirror's map (d16 / 16, 0 where invalid) under the default options: min_disparity 1 keeps every valid d16 >= 8."""
    rng = np.random.default_rng(2)
    img = _texture(rng, 80, 24)
    d16 = refdense.dense_stereo(img[:70], img[10:80], (rng.random((70, 24)) < 0.9).astype(np.uint8))
    assert (d16 == -1).any() and (d16 >= 0).any() and d16[d16 >= 0].min() >= 8
    dmap = np.where(d16 >= 0, d16 / 16.0, 0.0)
    assert np.array_equal(dmap == 0, d16 == -1)


def test_pcd_writer_header_and_point_count(tmp_path):
    from vo_single_camera_sos_amd.omnistereo.gum import write_pcd_ascii
    xyz = np.random.default_rng(0).normal(size=(7, 3)) * 1000
    lines = open(write_pcd_ascii(str(tmp_path / "XYZ.pcd"), xyz)).read().splitlines()
    assert lines[:11] == ["# .PCD v0.7 - Point Cloud Data file format", "VERSION 0.7", "FIELDS x y z", "SIZE 4 4 4", "TYPE F F F",
                          "COUNT 1 1 1", "WIDTH 7", "HEIGHT 1", "VIEWPOINT 0 0 0 1 0 0 0", "POINTS 7", "DATA ascii"]
    assert len(lines) == 11 + 7
    assert np.array_equal(np.array([l.split() for l in lines[11:]], dtype=np.float32), xyz.astype(np.float32))
    assert len(open(write_pcd_ascii(str(tmp_path / "empty.pcd"), np.zeros((0, 3)))).read().splitlines()) == 11
