"""CPU: the host-side mirror of the reference's model classes against golden vectors captured from the
reference (tests/golden/geometry_c2.npz).  The unwrap LUT is built with the same numpy float32/float64
operations as the reference, so it is compared BIT-EXACT."""
import os

import numpy as np
import pytest

from vo_single_camera_sos_amd.omnistereo.gum import synthetic_gums
from vo_single_camera_sos_amd.omnistereo.panorama import Panorama

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "geometry_c2.npz"))


def _rig():
    gs = synthetic_gums()
    gs.top_model.panorama = Panorama(gs.top_model, width=1200)
    gs.bot_model.panorama = Panorama(gs.bot_model, width=1200)
    return gs


def test_panorama_dimensions_and_lut_bit_exact():
    gs = _rig()
    for name, m in (("top", gs.top_model), ("bot", gs.bot_model)):
        pn = m.panorama
        rows, cols, px, hmax, hmin, circ = G[name + "_pano"]
        assert (pn.rows, pn.cols) == (int(rows), int(cols))
        assert pn.pixel_size == px and pn.cyl_height_max == hmax and pn.z_height_min == hmin
        assert pn.cyl_circumference == circ
        sel = G[name + "_lut_rows"]
        assert np.array_equal(pn.world2cam_LUT_map_x[sel], G[name + "_lut_x"], equal_nan=True)
        assert np.array_equal(pn.world2cam_LUT_map_y[sel], G[name + "_lut_y"], equal_nan=True)
        assert int(np.isnan(pn.world2cam_LUT_map_x).sum()) == int(G[name + "_lut_nan_count"][0])
        assert np.array_equal(m.T_model_wrt_C, G[name + "_T_model_wrt_C"])
        assert np.array_equal(m.F[:3, 0], G[name + "_F"])


def test_pixel_to_angles_bearings_and_projection():
    gs = _rig()
    for name, m in (("top", gs.top_model), ("bot", gs.bot_model)):
        mm = G["m_" + name]
        az, el = m.panorama.get_direction_angles_from_pixel_pano(mm, use_LUTs=False)
        assert np.array_equal(az, G["az_" + name], equal_nan=True)
        assert np.array_equal(el, G["el_" + name], equal_nan=True)
        b = m.get_3D_point_from_angles_wrt_focus(azimuth=az, elevation=el)[0]
        assert np.array_equal(b, G["bearing_" + name], equal_nan=True)
    Pw = np.array([[[2000.0, 500.0, 300.0, 1.0]]])
    u_t, v_t, _ = gs.top_model.get_pixel_from_3D_point_wrt_C(Pw)
    u_b, v_b, _ = gs.bot_model.get_pixel_from_3D_point_wrt_C(Pw)
    assert np.allclose([u_t.item(), v_t.item(), u_b.item(), v_b.item()], G["roundtrip_px"], rtol=1e-14)


def test_product_orb_pattern_equals_oracle_pattern():
    import oracle
    from vo_single_camera_sos_amd import orb_pattern
    assert np.array_equal(orb_pattern.orb_pattern(), oracle.orb_pattern())                 # OpenCV's table on both sides
    assert np.array_equal(orb_pattern.seeded_pattern(), oracle.orb_pattern_seeded())
    assert np.array_equal(orb_pattern.orb_pattern("seeded"), orb_pattern.seeded_pattern())
    assert not np.array_equal(orb_pattern.orb_pattern(), orb_pattern.seeded_pattern())
    ca, sa = orb_pattern.angle_cos_sin(-1.0)
    assert ca.dtype == np.float32 and np.isclose(ca, np.cos(np.deg2rad(1.0))) and sa < 0


def test_annulus_masks_and_bucket_columns():
    gs = _rig()
    top, bot = gs.make_annulus_masks((480, 640))
    assert top.dtype == np.uint8 and set(np.unique(top)) == {0, 255}
    assert not np.any((top > 0) & (bot > 0))          # the two annuli are disjoint
    assert top[239, 319 + 200] == 255 and top[239, 319 + 100] == 0 and bot[239, 319 + 80] == 255
    pn = gs.top_model.panorama
    assert pn.get_panorama_col_from_azimuth(0.0) == 1199
    assert pn.get_panorama_col_from_azimuth(np.pi) == 599
    assert pn.get_panorama_col_from_azimuth(2 * np.pi - 1e-9) in (0, 1)


def _unwrap_nearest(pn):
    """The unwrap of a mask without a GPU: nearest pixel of the panorama's own look-up tables (0 outside the image)."""
    mx, my = pn.float32_maps()

    def unwrap(omni_mask):
        ok = np.isfinite(mx) & np.isfinite(my)
        x, y = np.rint(np.where(ok, mx, -1)).astype(np.int64), np.rint(np.where(ok, my, -1)).astype(np.int64)
        h, w = omni_mask.shape
        ok &= (0 <= x) & (x < w) & (0 <= y) & (y < h)
        return np.where(ok, omni_mask[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0).astype(np.uint8)
    return unwrap


@pytest.mark.parametrize("moved", ["center_point_outer", "center_point_inner", "both"])
@pytest.mark.parametrize("padding", [0, 10])
def test_azimuthal_masks_follow_an_annulus_moved_by_whole_pixels(moved, padding):
    """generate_azimuthal_masks keeps its masks while the request and the annulus are unchanged.  An annulus whose circles
    move by whole pixels has the same shape, pixel count and radii as before: the masks must still be rebuilt (those of a
    fresh Panorama on the moved model), for the model's mask (padding 0) and for one made from the centres (padding > 0)."""
    gs = _rig()
    m, shape = gs.top_model, (480, 640)
    pn = m.panorama
    unwrap = _unwrap_nearest(pn)
    kw = dict(azimuth_mask_degrees=30, overlap_degrees=0, elev_mask_padding=padding, omni_shape=shape, unwrap_fn=unwrap)
    m.mask = m.make_mask(shape)
    before = [a.copy() for a in pn.generate_azimuthal_masks(**kw)]
    n_before = int(np.count_nonzero(m.mask))
    for name in (("center_point_outer", "center_point_inner") if moved == "both" else (moved,)):
        setattr(m, name, getattr(m, name) + np.array([3.0, -2.0]))
    m.mask = m.make_mask(shape)
    assert int(np.count_nonzero(m.mask)) == n_before       # (what the cache key looked at is unchanged)
    fresh = Panorama(m, width=1200).generate_azimuthal_masks(**kw)
    assert any(not np.array_equal(a, b) for a, b in zip(before, fresh))
    got = pn.generate_azimuthal_masks(**kw)
    assert len(got) == len(fresh) == 12
    assert all(np.array_equal(a, b) for a, b in zip(got, fresh))
    assert pn.generate_azimuthal_masks(**kw) is got        # (and an unchanged request still comes from the cache)


# ---- the distorted rig: the branches of the forward model the synthetic rig leaves at zero (a3 pinned on them) ----------
def test_distorted_rig_lut_and_projection_bit_exact():
    from distorted_rig import D, distorted_rig
    gs = distorted_rig()
    assert all(abs(v) > 0 for v in D["top_params"][[0, 1, 3, 4, 5, 8]]) and D["top_params"][6] != D["top_params"][7]
    for name, m in (("top", gs.top_model), ("bot", gs.bot_model)):
        pn = m.panorama
        rows, cols, px, hmax, hmin, circ = D[name + "_pano"]
        assert (pn.rows, pn.cols) == (int(rows), int(cols))
        assert pn.pixel_size == px and pn.cyl_height_max == hmax and pn.z_height_min == hmin and pn.cyl_circumference == circ
        assert np.array_equal([m.lowest_elevation_angle, m.highest_elevation_angle, m.globally_lowest_elevation_angle,
                               m.globally_highest_elevation_angle], D[name + "_elev"])
        sel = D[name + "_lut_rows"]
        lx, ly = np.asarray(pn.world2cam_LUT_map_x), np.asarray(pn.world2cam_LUT_map_y)
        assert np.array_equal(lx[sel], D[name + "_lut_x"], equal_nan=True)
        assert np.array_equal(ly[sel], D[name + "_lut_y"], equal_nan=True)
        assert int(np.isnan(lx).sum()) == int(D[name + "_lut_nan_count"][0])
        assert np.array_equal(np.flatnonzero(np.isnan(lx).any(axis=1)), D[name + "_lut_nan_rows"])
        for tag, arr in (("x", lx), ("y", ly)):      # EVERY entry of the float32 maps, through two sums
            f32 = arr.astype(np.float32)
            w = (np.arange(f32.size, dtype=np.float64).reshape(f32.shape) % 8191.0) + 1.0
            assert np.nansum(f32, dtype=np.float64) == D[name + "_lut_%s_f32_sum" % tag][0]
            assert np.nansum(f32.astype(np.float64) * w) == D[name + "_lut_%s_f32_wsum" % tag][0]
        P = np.ones((1, D["proj_points_wrt_C"].shape[0], 4))
        P[0, :, :3] = D["proj_points_wrt_C"]
        u, v, _ = m.get_pixel_from_3D_point_wrt_C(P)
        assert np.array_equal(np.stack([u.reshape(-1), v.reshape(-1)], axis=1), D["proj_uv_" + name])
        assert np.array_equal(m.T_model_wrt_C, D[name + "_T_model_wrt_C"])
    # the same arrays would NOT come out with the distortion-free model: the fixture does exercise the branch
    m = gs.top_model
    m.precalib_params.k1 = 0.0
    u0, _, _ = m.get_pixel_from_3D_point_wrt_C(P)
    assert np.abs(u0.reshape(-1) - D["proj_uv_top"][:, 0]).max() > 0.05


def test_distorted_rig_angles_bearings_gates():
    from distorted_rig import D, distorted_rig
    from vo_single_camera_sos_amd.omnistereo.common_cv import filter_pixel_correspondences
    gs = distorted_rig()
    for name, m in (("top", gs.top_model), ("bot", gs.bot_model)):
        az, el = m.panorama.get_direction_angles_from_pixel_pano(D["m_" + name], use_LUTs=False)
        assert np.array_equal(az, D["az_" + name], equal_nan=True) and np.array_equal(el, D["el_" + name], equal_nan=True)
        b = m.get_3D_point_from_angles_wrt_focus(azimuth=az, elevation=el)[0]
        assert np.array_equal(b, D["bearing_" + name], equal_nan=True)
    st = filter_pixel_correspondences(matched_points_top=D["m_top"][:, :2], matched_points_bot=D["m_bot"][:, :2],
                                      min_rectified_disparity=1, max_horizontal_diff=2.5)
    assert np.array_equal(st, D["gate_stereo"])


def test_distorted_rig_masks_use_each_circle_s_own_centre_and_json_round_trip(tmp_path):
    from distorted_rig import D, distorted_rig
    from vo_single_camera_sos_amd.omnistereo.gum import GUM, load_gums_json, save_gums_json
    gs = distorted_rig()
    top, bot = gs.make_annulus_masks((480, 640))
    t, b = gs.top_model, gs.bot_model
    assert not np.array_equal(t.center_point_inner, t.center_point_outer)
    want_top = GUM._disc((480, 640), t.center_point_outer, 226) & ~GUM._disc((480, 640), t.center_point_inner, 113) & \
        ~GUM._disc((480, 640), b.center_point_outer, 101)
    want_bot = GUM._disc((480, 640), b.center_point_outer, 101) & GUM._disc((480, 640), b.center_point_inner, 113) & \
        ~GUM._disc((480, 640), b.center_point_inner, 50)
    assert np.array_equal(top > 0, want_top) and np.array_equal(bot > 0, want_bot)
    one_centre = GUM._disc((480, 640), t.center_point, 226) & ~GUM._disc((480, 640), t.center_point, 113)
    assert not np.array_equal(top > 0, one_centre)
    f = str(tmp_path / "rig.json")
    save_gums_json(gs, f)
    back = load_gums_json(f)
    for a, c in ((gs.top_model, back.top_model), (gs.bot_model, back.bot_model)):
        assert np.array_equal(a.center_point_inner, c.center_point_inner) and np.array_equal(a.center_point_outer, c.center_point_outer)
        assert np.array_equal(a.panorama.world2cam_LUT_map_x, c.panorama.world2cam_LUT_map_x, equal_nan=True)
    m2 = back.make_annulus_masks((480, 640))
    assert np.array_equal(m2[0], top) and np.array_equal(m2[1], bot)


# ---- the per-frame API mirrors (camera_models / common_cv / pose_est_tools / pyopengv) ---------------------
def test_filter_pixel_correspondences_matches_reference_gates():
    from vo_single_camera_sos_amd.omnistereo.common_cv import filter_pixel_correspondences
    m_top, m_bot = G["m_top"], G["m_bot"]
    st = filter_pixel_correspondences(matched_points_top=m_top[:, :2], matched_points_bot=m_bot[:, :2],
                                      min_rectified_disparity=1, max_horizontal_diff=2.5)
    ff = filter_pixel_correspondences(matched_points_top=m_top[:, :2], matched_points_bot=m_bot[:, :2],
                                      min_rectified_disparity=-1, max_horizontal_diff=1.25)
    assert np.array_equal(st, G["gate_stereo"]) and np.array_equal(ff, G["gate_f2f"])
    none = filter_pixel_correspondences(m_top[:, :2], m_bot[:, :2], -1, -1)
    assert none.all() and none.shape == (m_top.shape[0],)


def test_tracker_parameters_and_score_definition():
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    tr = object.__new__(pet.TrackerSE3)
    assert pet.TrackerSE3.compute_num_of_iterations_RANSAC(tr, 3, 0.65) == int(G["ransac_iters_3_065"][0])
    assert pet.TrackerSE3.compute_num_of_iterations_RANSAC(tr, 3, 0.90) == int(G["ransac_iters_3_090"][0])
    t = pet.TrackerSE3(camera_model=None)
    assert t.backprojection_score_threshold_3D_to_2D == G["thr_5deg"][0]
    assert t.max_ransac_iterations_3D_to_2D == int(G["ransac_iters_3_065"][0]) and t.detection_method == "GFT"
    T = np.vstack([G["score_T"], [0, 0, 0, 1]])
    s = pet.get_selected_distances_to_model(T, np.arange(64), G["score_p"], G["score_f"], False)
    assert np.allclose(s, G["score_expected"], rtol=0, atol=1e-15)
    inl, outl = pet.select_inliers_within_distance(T, np.arange(64), G["thr_5deg"][0], G["score_p"], G["score_f"], False)
    assert np.array_equal(inl, np.flatnonzero(G["score_expected"] < G["thr_5deg"][0])) and len(inl) + len(outl) == 64
    assert pet.get_length_units_conversion_factor("mm", "m") == 0.001
    assert pet.get_length_units_conversion_factor("m", "mm") == 1000.0 and pet.get_length_units_conversion_factor("m", "m") == 1.0


def test_correspondence_containers():
    from vo_single_camera_sos_amd.omnistereo.camera_models import (KeyPoint, KeyPointAndDescriptor, PanoramicCorrespondences,
                                                                   MatchList, keypoints_to_array)
    kl = [[KeyPoint(1.5, 2.0), KeyPoint(3.0, 4.0)], [], [KeyPoint(5.0, 6.5)]]
    dl = [np.full((2, 32), 7, np.uint8), None, np.full((1, 32), 9, np.uint8)]
    kd = KeyPointAndDescriptor(kl, dl, do_flattening=True)
    assert len(kd.keypoints) == 3 and kd.descriptors.shape == (3, 32) and kd.pixel_coords.shape == (1, 3, 3)
    assert np.array_equal(kd.pixel_coords[0, :, :2], [[1.5, 2.0], [3.0, 4.0], [5.0, 6.5]]) and np.all(kd.pixel_coords[0, :, 2] == 1)
    assert kd.random_colors_RGB.shape == (3, 3) and kd.random_colors_RGB.dtype == np.uint8
    pc = PanoramicCorrespondences(kl, dl, kl, dl, points_3D=np.arange(9.0).reshape(3, 3), do_flattening=True)
    assert pc.m_top.shape == (3, 3) and np.all(pc.m_top[:, 2] == 1) and pc.desc_bot.shape == (3, 32)
    assert pc.points_3D_coords_homo.shape == (3, 4) and np.all(pc.points_3D_coords_homo[:, 3] == 1)
    empty = PanoramicCorrespondences([], [], [], [], points_3D=np.empty((0, 3)))
    assert empty.m_top.shape == (0, 3) and empty.points_3D_coords_homo.shape == (0, 4)
    assert keypoints_to_array([]).shape == (0, 2)
    ml = MatchList([2, 0], [5, 1], [3.0, 8.0])
    assert [m.queryIdx for m in ml] == [2, 0] and ml[1].trainIdx == 1 and ml[0].distance == 3.0 and len(ml) == 2


def test_matcher_and_pyopengv_mirror_fail_loudly_without_gpu():
    import pytest
    import torch
    from vo_single_camera_sos_amd import pyopengv
    from vo_single_camera_sos_amd._lib import SosvoError
    from vo_single_camera_sos_amd.omnistereo.camera_models import FeatureMatcher
    assert FeatureMatcher("ORB", "FLANN", 1).matcher_type == "FLANN"        # served by the exact search
    with pytest.raises(ValueError):
        FeatureMatcher("ORB", "ANNOY", 1)
    fm = FeatureMatcher("GFT", "BF", 1, percentage_good_matches=0.5, num_of_features=77)
    assert fm.percentage_good_matches == 0.5 and fm.num_of_features == 77 and fm.use_radius_match is False
    with pytest.raises(ValueError):
        pyopengv.absolute_pose_ransac(np.zeros((8, 3)), np.zeros((8, 3)), "UPNP", 0.01, 10)
    with pytest.raises(ValueError):
        pyopengv.relative_pose_ransac(np.zeros((8, 3)), np.zeros((8, 3)), "NOPE", 0.01, 10)
    if torch.cuda.is_available():
        return
    d = np.zeros((4, 32), np.uint8)
    with pytest.raises(SosvoError):  # no CPU fallback behind the reference's API
        fm.match(d, d)
    with pytest.raises(SosvoError):
        pyopengv.absolute_pose_ransac(np.eye(3).repeat(3, 0), np.ones((9, 3)), "KNEIP", 0.01, 10)
    with pytest.raises(SosvoError):
        pyopengv.triangulation_triangulate2(np.ones((2, 3)), np.ones((2, 3)), np.zeros(3), np.eye(3))


def test_reference_module_paths_resolve_to_the_mirror():
    """`omnistereo.*` (the reference's module paths, BASELINE north_star: "entry points intact") are the mirror's modules."""
    import importlib
    import omnistereo
    from omnistereo.camera_models import FeatureMatcher
    import omnistereo.pose_est_tools as pet
    import vo_single_camera_sos_amd.omnistereo.pose_est_tools as mirror
    assert pet is mirror and FeatureMatcher is importlib.import_module("vo_single_camera_sos_amd.omnistereo.camera_models").FeatureMatcher
    for name in ("TrackerStereoSE3", "TrackerRGBDSE3", "StereoPanoramicFrame", "RGBDFrame", "run_VO", "driver_VO",
                 "pose_relative_ransac_2D_to_2D", "pose_absolute_ransac_3D_to_2D"):
        assert hasattr(pet, name), name
    assert hasattr(omnistereo.panorama, "Panorama") and hasattr(omnistereo.gum, "GUM")
