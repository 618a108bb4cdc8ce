"""Host-side mirror of the hot-path part of omnistereo/pose_est_tools.py: the per-frame classes and functions of
one VO step with the reference's names, arguments, return structure and error behaviour; the arithmetic runs
on the GPU through libsosvo (FeatureMatcher, pyopengv mirror, the rig's device front end).

    get_selected_distances_to_model / select_inliers_within_distance   pose_est_tools.py:131-203  (numpy, as there)
    match_features_frame_to_frame                                       pose_est_tools.py:211-269
    StereoPanoramicFrame                                                pose_est_tools.py:271-402
    TrackerSE3 / TrackerStereoSE3 (track_frame, bootstrap_tracker)      pose_est_tools.py:594-878

The batched throughput path (vo_single_camera_sos_amd.pipeline.FramePairPipeline) runs the same sequence for many
frame pairs at once without host round trips; this module is the drop-in for code written against the
reference's per-frame API.

    RGBDFrame / TrackerRGBDSE3                                          pose_est_tools.py:404-623, :880-958
    StereoPanoramicKeyFrame / RGBDKeyFrame                              pose_est_tools.py:625-641
    run_VO / driver_VO (frame loop, keyframe policy, TUM pose files)    pose_est_tools.py:1264-1741

Not built: visualisation (vispy / matplotlib windows), the live-camera driver (run_VO_live)."""
import functools
import itertools
import os
import threading
import time
from warnings import warn

from math import log10, sqrt

import numpy as np

from .. import pyopengv
from .._lib import LK_MAX_LEVELS, MatchOptions, StepOptions, f2f_tracker_options, gated_flags, ratio_flags, stereo_refine_options
from . import transformations as tr
from .camera_models import FeatureMatcher, KeyPoint, KeyPointAndDescriptor, PanoramicCorrespondences, keypoints_to_array
from .common_cv import filter_pixel_correspondences
from .common_tools import copy_only_attributes, get_length_units_conversion_factor, make_sure_path_exists

_IDENTITY4 = np.identity(4)
_IDENTITY4.setflags(write=False)   # shared initial pose of device frames: replaced by the tracker, never written in place


def normalized(v):
    return v / np.linalg.norm(v)


def pose_relative_ransac_2D_to_2D(bearing_vectors1, bearing_vectors2, model_error_threshold=0.001,
                                  rel_pose_est_algorithm="STEWENIUS", outlier_fraction_known=0.50):
    """pose_est_tools.py:54-90: 2D-2D relative-pose RANSAC with the iteration budget N = log(0.01) / log(1 - w^n) + 3 std,
    n = 5 ("NISTER", "STEWENIUS"), 7 ("SEVENPT") or 8 ("EIGHTPT") -> (T 4x4 with |t| = 1, inlier indices).  Not reached
    by the VO drivers."""
    from math import log10, sqrt
    n_points_for_model = {"NISTER": 5, "STEWENIUS": 5, "SEVENPT": 7, "EIGHTPT": 8}.get(rel_pose_est_algorithm, -1)
    w = 1.0 - outlier_fraction_known
    num_of_iters = log10(1.0 - 0.99) / log10(1.0 - w ** n_points_for_model)
    std_of_k = sqrt(1.0 - w ** n_points_for_model) / (w ** n_points_for_model)
    max_iterations = int(num_of_iters + 3 * std_of_k)
    T, inliers = pyopengv.relative_pose_ransac(bearing_vectors1[..., :3], bearing_vectors2[..., :3], rel_pose_est_algorithm,
                                               model_error_threshold, max_iterations)
    T_homo = np.identity(4)
    T_homo[:3] = T
    return T_homo, inliers


def pose_absolute_ransac_3D_to_2D(bearing_vectors, points3D, model_error_threshold=0.001, pose_est_algorithm="EPNP",
                                  outlier_fraction_known=0.50, max_iterations=-1):
    """pose_est_tools.py:92-129: central absolute-pose RANSAC with the iteration budget N = log(0.01) / log(1 - w^n)
    + 3 std (n = 2 for "TWOPT", else 3 -- as written there, also for "EPNP") when max_iterations < 0
    -> (T 4x4, inlier indices)."""
    from math import log10, sqrt
    if max_iterations < 0:
        n_points_for_model = 2 if pose_est_algorithm == "TWOPT" else 3
        w = 1.0 - outlier_fraction_known
        num_of_iters = log10(1.0 - 0.99) / log10(1.0 - w ** n_points_for_model)
        std_of_k = sqrt(1.0 - w ** n_points_for_model) / (w ** n_points_for_model)
        max_iterations = int(num_of_iters + 3 * std_of_k)
    T, inliers = pyopengv.absolute_pose_ransac(bearing_vectors[..., :3], points3D[..., :3], pose_est_algorithm,
                                               model_error_threshold, max_iterations)
    T_homo = np.identity(4)
    T_homo[:3] = T
    return T_homo, inliers


def get_selected_distances_to_model(model, indices, bearing_vectors1, bearing_vectors2, is_relative_2D_to_2D_case,
                                    verbose_debug=False):
    """pose_est_tools.py:150-203: OpenGV's absolute-pose score 1 - f . normalize(R^T (p - t)) per index (the
    relative 2D-2D case adds the score of the triangulated point in frame 1).  Unused at run time in the
    reference too; it pins the scoring definition the RANSAC kernel implements."""
    translation = model[:3, 3]
    rotation = model[:3, :3]
    inverse = np.identity(4)
    inverse[:3, :3] = rotation.T
    inverse[:3, 3] = -inverse[:3, :3].dot(translation[:3])
    if is_relative_2D_to_2D_case:
        p_all = pyopengv.triangulation_triangulate2(bearing_vectors1[..., :3], bearing_vectors2[..., :3], translation, rotation)
    else:
        p_all = bearing_vectors1.copy()
    scores = []
    for i in indices:
        p_homo = np.ones(4)
        p_homo[:3] = p_all[i][:3]
        reprojection2 = normalized(inverse.dot(p_homo)[:3])
        score = 1.0 - bearing_vectors2[i, :3].T.dot(reprojection2)
        if is_relative_2D_to_2D_case:
            score = (1.0 - bearing_vectors1[i, :3].T.dot(normalized(p_homo[:3]))) + score
        scores.append(score)
    return scores


def select_inliers_within_distance(model_coefficients, indices_all, threshold, bearing_vectors1, bearing_vectors2,
                                   is_relative_2D_to_2D_case):
    """pose_est_tools.py:131-148"""
    d = np.array(get_selected_distances_to_model(model_coefficients, indices_all, bearing_vectors1, bearing_vectors2,
                                                 is_relative_2D_to_2D_case))
    test = d < threshold
    return indices_all[test], indices_all[np.invert(test)]


def match_features_frame_to_frame(cam_model, train_kpts, train_desc, query_kpts, query_desc, random_colors_RGB,
                                  max_horizontal_diff=-1, max_descriptor_distance_radius=-1, keypts_as_points_train=None,
                                  keypts_as_points_query=None, pano_img_train=None, pano_img_query=None,
                                  show_matches=False, win_name="Matches (Frame-to-Frame)"):
    """pose_est_tools.py:211-269: query = current frame, train = keyframe; first percentage_good_matches of the
    sorted matches; gate |du| <= max_horizontal_diff -- no wrap-around, as the reference, unless the camera model carries
    set_cyclic_columns: then d <= max or cols - d <= max, in the search too when it is gated.
    -> (train idx, train kpts, train desc), (query idx, query kpts, query desc), colours"""
    fm = cam_model.feature_matcher_for_motion
    if getattr(fm, "gated", False):   # the search under the |du| gate applied below (off when that gate is off)
        pts = [keypoints_to_array(k) if p is None else np.asarray(p)
               for k, p in ((query_kpts, keypts_as_points_query), (train_kpts, keypts_as_points_train))]
        cyc = dict(period=cam_model.top_model.panorama.cols) if getattr(cam_model, "cyclic_columns", False) else {}
        q, t, _ = fm.match_gated_many([(query_desc, train_desc, pts[0], pts[1])], -1.0, max_horizontal_diff,
                                      fm.gated_max_distance, **cyc)[0]
    else:
        q, t, _ = fm.match_arrays(query_desc, train_desc)
    matched_train_indices, matched_query_indices = [], []
    matched_kpts_train, matched_kpts_query, matched_desc_train, matched_desc_query, random_colors = [], [], [], [], []
    good = int(fm.percentage_good_matches * len(q))
    if good > 0:
        t_all, q_all = t[:good], q[:good]
        train_kpts, query_kpts = np.asarray(train_kpts, dtype=object), np.asarray(query_kpts, dtype=object)
        k_train_all, k_query_all = train_kpts[t_all], query_kpts[q_all]
        if keypts_as_points_train is None:
            keypts_as_points_train = keypoints_to_array(k_train_all).astype(np.float64)
        else:
            keypts_as_points_train = np.asarray(keypts_as_points_train)[t_all]
        if keypts_as_points_query is None:
            keypts_as_points_query = keypoints_to_array(k_query_all).astype(np.float64)
        else:
            keypts_as_points_query = np.asarray(keypts_as_points_query)[q_all]
        if max_horizontal_diff >= 0:
            ok = filter_pixel_correspondences(matched_points_top=keypts_as_points_train,
                                              matched_points_bot=keypts_as_points_query, min_rectified_disparity=-1,
                                              max_horizontal_diff=max_horizontal_diff)
            if getattr(cam_model, "cyclic_columns", False) and max_horizontal_diff > 0:   # ... or the short way round
                d = np.abs(np.asarray(keypts_as_points_train)[..., 0] - np.asarray(keypts_as_points_query)[..., 0])
                ok = np.logical_or(ok, float(cam_model.top_model.panorama.cols) - d <= max_horizontal_diff)
            matched_train_indices, matched_query_indices = t_all[ok], q_all[ok]
            matched_kpts_train, matched_kpts_query = k_train_all[ok], k_query_all[ok]
        else:
            matched_train_indices, matched_query_indices = t_all, q_all
            matched_kpts_train, matched_kpts_query = k_train_all, k_query_all
        matched_desc_train = np.asarray(train_desc)[matched_train_indices]
        matched_desc_query = np.asarray(query_desc)[matched_query_indices]
        try:
            random_colors = np.asarray(random_colors_RGB)[matched_train_indices]
        except Exception:
            print("Problem, it only has", len(random_colors_RGB))
    return (matched_train_indices, matched_kpts_train, matched_desc_train), \
        (matched_query_indices, matched_kpts_query, matched_desc_query), random_colors


def _device_angles_and_bearings(ctx, pano, m_pano):
    """Pixels [n, >= 2] of a panorama -> (azimuth [n], elevation [n], unit bearing [n, 3]) as Context.pano_to_bearing gives them."""
    import torch
    if len(m_pano) == 0:   # (a frame without stereo matches)
        return np.zeros(0), np.zeros(0), np.zeros((0, 3))
    uv = np.ascontiguousarray(np.asarray(m_pano, dtype=np.float64).reshape(len(m_pano), -1)[:, :2])
    az, el, b = ctx.pano_to_bearing(torch.from_numpy(uv).to(ctx.device), pano.cols, pano.rows, pano.pixel_size, pano.cyl_height_max)
    ctx.synchronize()
    return az.cpu().numpy(), el.cpu().numpy(), b.cpu().numpy()


class StereoPanoramicFrame(object):
    """pose_est_tools.py:271-402: one omnistereo frame = detected + stereo-matched + triangulated + range-filtered
    correspondences of the rig's current omni image."""

    def __init__(self, stereo_camera_model, frame_id, **kwargs):
        self.frame_id = frame_id
        self.parent_id = kwargs.get("parent_id", -1)
        self.T_frame_wrt_tracking_ref_frame = np.identity(4)
        top, bot = stereo_camera_model.top_model, stereo_camera_model.bot_model
        self.panoramic_image_top = None if top.panorama.panoramic_img is None else top.panorama.panoramic_img.copy()
        self.panoramic_image_bottom = None if bot.panorama.panoramic_img is None else bot.panorama.panoramic_img.copy()
        self.use_midpoint_triangulation = True
        self.use_opengv_triangulation = False
        self.conversion_factor_length_to_m = get_length_units_conversion_factor(stereo_camera_model.units, "m")
        self.first_row_to_crop_bottom = 0
        self.total_time = 0.
        self.median_win_size = 11
        self.min_disp = 1
        self.max_u_dist = 2.5 if self.use_midpoint_triangulation else 0.5
        from_m = get_length_units_conversion_factor("m", stereo_camera_model.units)
        self.min_range = 0.5 * from_m
        self.max_range = 7.0 * from_m
        self.pano_correspondences = None
        self.num_valid_keypoints = 0
        self.establish_stereo_correspondences(omnistereo_model=stereo_camera_model)

    def establish_stereo_correspondences(self, omnistereo_model, collect_time_statistics=False):
        fm = omnistereo_model.feature_matcher_for_static_stereo
        top, bot = omnistereo_model.top_model, omnistereo_model.bot_model
        kl_top, dl_top = top.detect_sparse_features_on_panorama(feature_detection_method=fm.feature_detection_method,
                                                                num_of_features=fm.num_of_features,
                                                                median_win_size=self.median_win_size, show=False)
        kl_bot, dl_bot = bot.detect_sparse_features_on_panorama(feature_detection_method=fm.feature_detection_method,
                                                                num_of_features=fm.num_of_features,
                                                                median_win_size=self.median_win_size, show=False)
        (m_top0, k_top0, d_top0), (m_bot0, k_bot0, d_bot0), colors0 = omnistereo_model.match_features_panoramic_top_bottom(
            keypts_list_top=kl_top, desc_list_top=dl_top, keypts_list_bot=kl_bot, desc_list_bot=dl_bot,
            min_rectified_disparity=self.min_disp, max_horizontal_diff=self.max_u_dist, show_matches=False)
        # direction angles and bearings (pose_est_tools.py:344-352) from the stage the engines' stereo assembly computes them
        # with, sosvo_pano_to_bearing: panorama.get_direction_angles_from_pixel_pano / get_3D_point_from_angles_wrt_focus give
        # the same values in numpy's arithmetic, which differs from the device's in the last bit of about 1 elevation in 70 and
        # 1 bearing entry in 24 -- enough to move the refined pose in its 15th digit, so that this per-frame path and the
        # sequence engines wrote pose files that differed in their last digits
        az1, el1, b1 = _device_angles_and_bearings(omnistereo_model._context(), top.panorama, m_top0)
        az2, el2, b2 = _device_angles_and_bearings(omnistereo_model._context(), bot.panorama, m_bot0)
        if self.use_opengv_triangulation:
            T = omnistereo_model.T_bot_wrt_top
            xyz_top = pyopengv.triangulation_triangulate2(b1, b2, T[:3, 3], T[:3, :3])
            xyz_top_homo = np.concatenate((xyz_top, np.ones(xyz_top.shape[:-1])[..., np.newaxis]), axis=-1)
            xyz0 = np.einsum("ij, nj->ni", top.T_model_wrt_C, xyz_top_homo)
        else:
            xyz0 = omnistereo_model.get_triangulated_point_from_direction_angles(
                dir_angs_top=(az1, el1), dir_angs_bot=(az2, el2), use_midpoint_triangulation=self.use_midpoint_triangulation)[0]
        good = omnistereo_model.filter_panoramic_points_due_to_range(xyz0, min_3D_range=self.min_range,
                                                                     max_3D_range=self.max_range)
        self.num_valid_keypoints = int(np.count_nonzero(good))
        # a tracker that tracks (set_f2f_tracker) follows this frame's points into the next frame's gray panoramas: they stay
        # on the device, [2, rows, cols] u8 with the rows the front end computed (gray_rows: int32 [2, 2] or None = all)
        self.gray_panoramas = self.gray_rows = None
        if getattr(omnistereo_model, "lk_options", None) is not None:
            fe = omnistereo_model._front_end(fm.feature_detection_method, fm.num_of_features, self.median_win_size)
            # (a seam-free front end's panoramas are padded: the tracker's circle is their interior, a tensor of its own)
            self.gray_panoramas = fe.gray_interior() if fe.seam_free else fe.gray.clone()
            # the rows the sequence engines' front end computes for this detector (GFT with the fused median: the reach of
            # its masks and descriptors, else every row): the tracker clamps to them there, so it does here, although this
            # front end has computed them all
            if fe.method == "GFT" and fe.median_win_size in (3, 5, 11):
                m, key = fe.model, (fe.edge, fe.cos_a, fe.sin_a)
                cache = m.__dict__.setdefault("_gray_rows", {})
                if key not in cache:
                    cache[key] = fe.ctx.gray_rows_needed(m.mask_bits, m.nmask, fe.edge, m.pattern, fe.cos_a, fe.sin_a)
                self.gray_rows = cache[key]
        self.bearing_vectors_top_stereo_triangulated = b1[good]
        self.bearing_vectors_bottom_stereo_triangulated = b2[good]
        self.pano_correspondences = PanoramicCorrespondences(
            kpts_top_list=k_top0[good], desc_top_list=d_top0[good], kpts_bot_list=k_bot0[good], desc_bot_list=d_bot0[good],
            points_3D=xyz0[good], m_top_array=m_top0[good], m_bot_array=m_bot0[good],
            random_colors_RGB_list=colors0[good], do_flattening=False)


class TrackerSE3(object):
    """pose_est_tools.py:594-720 (the tracking parameters; visualisation and result paths left out)."""

    def __init__(self, camera_model, show_3D_points=False, **kwargs):
        self.camera_model = camera_model
        self.show_3D_points = show_3D_points
        self.T_C_wrt_S_init = np.identity(4)
        self.T_C_curr_frame_wrt_S_est = np.identity(4)
        self.xyz_homo_points_wrt_C_inliers = []
        self.rgb_points_inliers = []
        self.num_tracked_correspondences = 0
        self.inlier_tracked_correspondences_ratio = 0.
        self.number_of_cams = 1
        self.T_Ckey_wrt_S_est_list = []
        self.set_global_parameters_for_tracking()

    def set_global_parameters_for_tracking(self):
        """pose_est_tools.py:672-707"""
        self.backprojection_score_threshold_3D_to_2D_in_degrees = 5.
        self.backprojection_score_threshold_3D_to_2D = 1.0 - np.cos(np.deg2rad(self.backprojection_score_threshold_3D_to_2D_in_degrees))
        self.detection_method = "GFT"
        self.matching_type = "BF"
        self.k_best_matches = 1
        self.percentage_good_matches = 1.0
        self.use_descriptor_radius_match_for_motion = False
        # the matchers' crossCheck: off, as the reference builds them (camera_models.py:401-402); see set_cross_check
        self.cross_check_static_stereo = False
        self.cross_check_for_motion = False
        # the search under the pixel gates (FeatureMatcher.match_gated): off; see set_gated_matching
        self.gated_static_stereo = False
        self.gated_for_motion = False
        self.gated_max_distance = None
        # Lowe's ratio rule on the device (FeatureMatcher's ratio): off; see set_ratio_test
        self.ratio_static_stereo = None
        self.ratio_for_motion = None
        # sub-pixel refinement of the detected keypoints (window half-size): off; see set_subpixel_refinement
        self.subpix_half = None
        # Lucas-Kanade tracking in place of the frame-to-frame matcher (an LKOptions): off; see set_f2f_tracker
        self.lk_options = None
        # sub-pixel static stereo (a StereoLKOptions): off; see set_stereo_refinement
        self.stereo_lk_options = None
        self.num_features_detection_for_motion = 1000
        self.max_horizontal_search_ratio = 0.50
        self.pose_est_algorithm = "EPNP"
        self.n_points_for_RANSAC_model = 3
        self.correspondences_outliers_fraction = 0.65
        self.max_ransac_iterations_3D_to_2D = -1
        if self.max_ransac_iterations_3D_to_2D < 0:
            self.max_ransac_iterations_3D_to_2D = self.compute_num_of_iterations_RANSAC(
                n_points_for_model=self.n_points_for_RANSAC_model,
                correspondences_outliers_fraction=self.correspondences_outliers_fraction)

    def compute_num_of_iterations_RANSAC(self, n_points_for_model, correspondences_outliers_fraction):
        """pose_est_tools.py:709-720"""
        w = 1.0 - correspondences_outliers_fraction
        desired_prob_only_inlier_selection = 0.998
        num_of_iters = log10(1.0 - desired_prob_only_inlier_selection) / log10(1.0 - w ** n_points_for_model)
        std_of_k = sqrt(1.0 - w ** n_points_for_model) / (w ** n_points_for_model)
        return int(num_of_iters + 3 * std_of_k)

    # What the track_frame of the two families differ in beside their solvers, each as the reference has it
    min_matches_per_cam = 1.0            # tracking needs 2 n (min_matches_per_cam * number_of_cams) correspondences
    refuses_without_model = False        # fewer inliers than the model needs points: the frame is reported as not tracked
    device_track_resets = {}             # attributes the host path fills and a device record does not
    chain_pose = staticmethod(np.dot)    # (keyframe pose, frame wrt keyframe) -> frame pose

    def min_matches_to_track(self):
        return 2 * self.n_points_for_RANSAC_model * (self.min_matches_per_cam * self.number_of_cams)

    def _keep_pose(self, current_frame, T):
        """T [3, 4], the frame wrt its reference in the model's units -> current_frame.T_frame_wrt_tracking_ref_frame [m] and,
        chained with the newest keyframe's pose, self.T_C_curr_frame_wrt_S_est."""
        T_homo = np.identity(4)
        T_homo[:3] = T
        T_homo[:3, 3] = T[:3, 3] * current_frame.conversion_factor_length_to_m
        current_frame.T_frame_wrt_tracking_ref_frame = T_homo
        T_key = self.T_Ckey_wrt_S_est_list[-1] if self.T_Ckey_wrt_S_est_list else np.identity(4)
        self.T_C_curr_frame_wrt_S_est = self.chain_pose(T_key, T_homo)

    def _track_device_frame(self, reference_frame, current_frame):
        """track_frame on frames of a sequence engine's store: the [16] record (refined pose, inliers, correspondences,
        status) of the pair -- the speculative one when the reference is the frame's predecessor, one serial tracking
        call against the keyframe slot otherwise -- put through the bookkeeping of the family's track_frame."""
        eng = current_frame.engine
        ref_seq = getattr(reference_frame, "seq_index", None)
        if current_frame.spec_record is not None and ref_seq == current_frame.seq_index - 1:
            rec = current_frame.spec_record
        elif current_frame.spec2_record is not None and ref_seq == current_frame.seq_index - 2:
            rec = current_frame.spec2_record      # the frame in between was not promoted: tracked against t - 2 in the batch
        else:
            rec = eng.track(eng.key_slot, current_frame.slot, current_frame.seed)
        num_initial_matches = int(rec[13])
        if num_initial_matches < self.min_matches_to_track():
            return False, "Cannot track on only %d point correspondences" % (num_initial_matches)
        self.__dict__.update(self.device_track_resets)
        self.num_tracked_correspondences = int(rec[12])
        self.inlier_tracked_correspondences_ratio = float(self.num_tracked_correspondences) / float(num_initial_matches)
        if self.refuses_without_model and self.num_tracked_correspondences < self.n_points_for_RANSAC_model:
            return False, "RANSAC (%s) found no model among %d correspondences" % (self.pose_est_algorithm, num_initial_matches)
        self._keep_pose(current_frame, rec[:12].reshape(3, 4))
        return True, "tracking used %d inlier point correspondences" % (self.num_tracked_correspondences)


class TrackerStereoSE3(TrackerSE3):
    """pose_est_tools.py:722-878"""
    min_matches_per_cam = 0.33
    device_track_resets = dict(indices_inliers_combined=None)    # (the inlier list stays on the device)

    def __init__(self, camera_model, show_3D_points=False, **kwargs):
        TrackerSE3.__init__(self, camera_model, show_3D_points, **kwargs)
        self.omnistereo_model = self.camera_model
        self.number_of_cams = 2
        self.bootstrap_tracker()

    def bootstrap_tracker(self):
        """pose_est_tools.py:849-878"""
        om = self.omnistereo_model
        self.cam_offsets = np.array([om.top_model.T_model_wrt_C[:3, 3], om.bot_model.T_model_wrt_C[:3, 3]])
        self.cam_rotations = np.array([om.top_model.T_model_wrt_C[:3, :3], om.bot_model.T_model_wrt_C[:3, :3]])
        self.num_features_detection_for_static_stereo = 1000
        om.feature_matcher_for_static_stereo = FeatureMatcher(
            method=self.detection_method, matcher_type=self.matching_type, k_best=self.k_best_matches,
            percentage_good_matches=self.percentage_good_matches, num_of_features=self.num_features_detection_for_static_stereo,
            use_radius_match=False, cross_check=self.cross_check_static_stereo, gated=self.gated_static_stereo,
            gated_max_distance=self.gated_max_distance, ratio=self.ratio_static_stereo)
        self.max_horizontal_diff_f2f_matches = 0.125 * self.max_horizontal_search_ratio * om.top_model.panorama.cols
        om.feature_matcher_for_motion = FeatureMatcher(
            method=self.detection_method, matcher_type=self.matching_type, k_best=self.k_best_matches,
            percentage_good_matches=self.percentage_good_matches, num_of_features=self.num_features_detection_for_motion,
            use_radius_match=self.use_descriptor_radius_match_for_motion, cross_check=self.cross_check_for_motion,
            gated=self.gated_for_motion, gated_max_distance=self.gated_max_distance, ratio=self.ratio_for_motion)
        om.lk_options = self.lk_options    # (the frames keep their gray panoramas on the device when the tracker tracks)
        self.omni_mask_extra_padding = 10
        shape = None if om.current_omni_img is None else om.current_omni_img.shape[:2]
        if shape is None:
            shape = (om.top_model.image_size[1], om.top_model.image_size[0])
        if om.top_model.mask is None or om.bot_model.mask is None:
            om.make_annulus_masks(shape)
        for m in (om.top_model, om.bot_model):
            m.panorama.generate_azimuthal_masks(azimuth_mask_degrees=30, overlap_degrees=0, show=False,
                                                elev_mask_padding=self.omni_mask_extra_padding,
                                                stand_masks_azimuth_coord_in_degrees_list=[50, 170, 290],
                                                stand_masks_width_in_degrees=10, omni_shape=shape)

    def track_frame(self, reference_frame, current_frame):
        """pose_est_tools.py:736-847 -> (ok, message); sets current_frame.T_frame_wrt_tracking_ref_frame and
        self.T_C_curr_frame_wrt_S_est."""
        self.num_tracked_correspondences = 0
        self.inlier_tracked_correspondences_ratio = 0.
        if isinstance(current_frame, _DeviceFrame):
            return self._track_device_frame(reference_frame, current_frame)
        if self.lk_options is not None:
            return self._track_frame_lk(reference_frame, current_frame)
        ref, cur = reference_frame.pano_correspondences, current_frame.pano_correspondences
        (t_top, _, _), (q_top, _, _), _ = match_features_frame_to_frame(
            cam_model=self.omnistereo_model, train_kpts=ref.kpts_top, train_desc=ref.desc_top, query_kpts=cur.kpts_top,
            query_desc=cur.desc_top, random_colors_RGB=ref.random_colors_RGB,
            max_horizontal_diff=self.max_horizontal_diff_f2f_matches, max_descriptor_distance_radius=-1,
            keypts_as_points_train=ref.m_top, keypts_as_points_query=cur.m_top)
        (t_bot, _, _), (q_bot, _, _), _ = match_features_frame_to_frame(
            cam_model=self.omnistereo_model, train_kpts=ref.kpts_bot, train_desc=ref.desc_bot, query_kpts=cur.kpts_bot,
            query_desc=cur.desc_bot, random_colors_RGB=ref.random_colors_RGB,
            max_horizontal_diff=self.max_horizontal_diff_f2f_matches, max_descriptor_distance_radius=-1,
            keypts_as_points_train=ref.m_bot, keypts_as_points_query=cur.m_bot)
        t_top, q_top, t_bot, q_bot = [np.asarray(a, dtype=np.int64) for a in (t_top, q_top, t_bot, q_bot)]
        bearings = [current_frame.bearing_vectors_top_stereo_triangulated[q_top],
                    current_frame.bearing_vectors_bottom_stereo_triangulated[q_bot]]
        points = [ref.points_3D_coords_homo[t_top][..., :3], ref.points_3D_coords_homo[t_bot][..., :3]]
        cam_all = np.concatenate([np.zeros((len(points[c]), 1)) + float(c) for c in range(self.number_of_cams)])
        b_all = np.vstack(bearings).reshape(-1, 3)
        p_all = np.vstack(points).reshape(-1, 3)
        num_initial_matches = b_all.shape[0]
        if num_initial_matches < self.min_matches_to_track():
            return False, "Cannot track on only %d point correspondences" % (num_initial_matches)
        T_ransac, inliers = pyopengv.absolute_pose_noncentral_ransac(
            b_all, cam_all, p_all, self.cam_offsets, self.cam_rotations, self.backprojection_score_threshold_3D_to_2D,
            self.max_ransac_iterations_3D_to_2D)
        self.indices_inliers_combined = inliers
        self.num_tracked_correspondences = len(inliers)
        self.inlier_tracked_correspondences_ratio = float(self.num_tracked_correspondences) / float(num_initial_matches)
        T_nl = pyopengv.absolute_pose_noncentral_optimize_nonlinear(
            b_all[inliers], cam_all[inliers], p_all[inliers], self.cam_offsets, self.cam_rotations, T_ransac[:3, 3],
            T_ransac[:3, :3])
        self._keep_pose(current_frame, T_nl)
        if self.show_3D_points:
            self.xyz_homo_points_wrt_C_inliers = np.hstack((p_all[inliers] * current_frame.conversion_factor_length_to_m,
                                                            np.ones((len(inliers), 1))))
        return True, "tracking used %d inlier point correspondences" % (self.num_tracked_correspondences)

    LK_FRAME_CAP = 4096     # the points of a frame the tracker follows: the sequence engines' frame_cap (_sos_engine_settings)

    def _track_frame_lk(self, reference_frame, current_frame):
        """track_frame with set_f2f_tracker(..., "lk"): the reference frame's stereo points m_top / m_bot are tracked into the
        current frame's gray panoramas (Context.gray_pyramid / track_lk, two problems: top view, bottom view) and stacked by
        Context.f2f_assemble_tracked -- the stages, the layout and the row range of the sequence engines' tracking step."""
        import torch
        from ..device import make_rig
        om, o, ref = self.omnistereo_model, self.lk_options, reference_frame.pano_correspondences
        ctx = om._context()
        if reference_frame.gray_panoramas is None or current_frame.gray_panoramas is None:
            raise RuntimeError("f2f_tracker=\"lk\": the frames were built before set_f2f_tracker and keep no gray panoramas")
        dev = ctx.device
        n = min(len(ref.m_top), self.LK_FRAME_CAP)
        cap = max(n, 1)
        # view-major images [top of the reference, top of the current frame, bottom ..., bottom ...]
        gray = torch.stack([reference_frame.gray_panoramas[0], current_frame.gray_panoramas[0],
                            reference_frame.gray_panoramas[1], current_frame.gray_panoramas[1]])
        pts = np.zeros((2, cap, 2), np.float32)
        pts[0, :n], pts[1, :n] = ref.m_top[:n, :2], ref.m_bot[:n, :2]
        X = np.zeros((1, cap, 3))
        X[0, :n] = ref.points_3D_coords_homo[:n, ..., :3].reshape(n, 3)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)    # noqa: E731
        prev = to(pts)
        cyclic = bool(getattr(om, "cyclic_columns", False))
        pyr = (ctx.gray_pyramid_cyclic if cyclic else ctx.gray_pyramid)(gray, o.levels, row_range=reference_frame.gray_rows)
        res = ctx.track_lk(pyr, i32([0, 2]), i32([1, 3]), prev, i32([n, n]), half=o.half, max_iter=o.max_iter, eps=o.eps,
                           min_eig=o.min_eig, fb_max=o.fb_max)
        top, bot = om.top_model, om.bot_model
        geo = [(m.panorama.cols, m.panorama.rows, m.panorama.pixel_size, m.panorama.cyl_height_max) for m in (top, bot)]
        rig = make_rig(geo[0], geo[1], top.F[:3, 0], bot.F[:3, 0], 0.0, 0.0, f2f_max_hdiff=self.max_horizontal_diff_f2f_matches)
        frames = dict(m_top=prev[0:1], m_bot=prev[1:2], X=to(X), M=i32([n]))
        nxt, st = res[0], res[1]
        corr = ctx.f2f_assemble_tracked(rig, frames, i32([0]), nxt[0:1], nxt[1:2], st[0:1], st[1:2], 2 * cap,
                                        **(dict(cyclic=True) if cyclic else {}))
        ctx.synchronize()
        num_initial_matches = int(corr["n"].cpu().numpy()[0])
        if num_initial_matches < self.min_matches_to_track():
            return False, "Cannot track on only %d point correspondences" % (num_initial_matches)
        b_all = corr["f"][0, :num_initial_matches].cpu().numpy()
        p_all = corr["p"][0, :num_initial_matches].cpu().numpy()
        cam_all = corr["cam"][0, :num_initial_matches].cpu().numpy().astype(np.float64).reshape(-1, 1)
        T_ransac, inliers = pyopengv.absolute_pose_noncentral_ransac(
            b_all, cam_all, p_all, self.cam_offsets, self.cam_rotations, self.backprojection_score_threshold_3D_to_2D,
            self.max_ransac_iterations_3D_to_2D)
        self.indices_inliers_combined = inliers
        self.num_tracked_correspondences = len(inliers)
        self.inlier_tracked_correspondences_ratio = float(self.num_tracked_correspondences) / float(num_initial_matches)
        T_nl = pyopengv.absolute_pose_noncentral_optimize_nonlinear(
            b_all[inliers], cam_all[inliers], p_all[inliers], self.cam_offsets, self.cam_rotations, T_ransac[:3, 3],
            T_ransac[:3, :3])
        self._keep_pose(current_frame, T_nl)
        if self.show_3D_points:
            self.xyz_homo_points_wrt_C_inliers = np.hstack((p_all[inliers] * current_frame.conversion_factor_length_to_m,
                                                            np.ones((len(inliers), 1))))
        return True, "tracking used %d inlier point correspondences" % (self.num_tracked_correspondences)


class _DeviceFrame(object):
    """What DeviceStereoFrame and DeviceRGBDFrame share: a frame whose data live in the frame store of a sequence engine
    (HBM; slot `slot` of the store while the frame's window is current, the keyframe slot once promoted) instead of host
    arrays.  run_VO's sequence mode builds these, `window` frames per batched front-end pass, from the engine's records
    (`info`).  A family supplies engine_consts: the attributes that are the same for every frame of an engine."""

    def __init__(self, engine, info, camera_model, frame_id, seq_index, **kwargs):
        consts = getattr(engine, "_frame_consts", None)
        if consts is None:   # (ctypes field reads are slow: once per engine; an engine belongs to one camera model)
            consts = engine._frame_consts = self.engine_consts(engine, camera_model)
        self.__dict__.update(consts)
        self.frame_id = frame_id
        self.parent_id = kwargs.get("parent_id", -1)
        self.T_frame_wrt_tracking_ref_frame = _IDENTITY4   # (replaced, never written in place, by the tracker)
        self.engine, self.slot, self.seq_index = engine, int(info["slot"]), int(seq_index)
        self.seed, self.spec_record, self.spec2_record = int(info["seed"]), info["spec"], info.get("spec2")
        self.num_valid_keypoints = int(info["count"])

    def promote(self):
        self.engine.promote(self.slot)


class DeviceStereoFrame(_DeviceFrame, StereoPanoramicFrame):
    """A StereoPanoramicFrame in the store of a pipeline.SequenceEngine: same attributes as the host frame except
    pano_correspondences / the bearing arrays, which stay on the device."""

    @staticmethod
    def engine_consts(engine, stereo_camera_model):
        return dict(
            panoramic_image_top=None, panoramic_image_bottom=None, use_midpoint_triangulation=True,
            use_opengv_triangulation=False, first_row_to_crop_bottom=0, total_time=0., pano_correspondences=None,
            conversion_factor_length_to_m=get_length_units_conversion_factor(stereo_camera_model.units, "m"),
            median_win_size=int(engine.cfg.median_ksize), min_disp=engine.rig_cfg.stereo_min_disp,
            max_u_dist=engine.rig_cfg.stereo_max_hdiff, min_range=engine.rig_cfg.min_range, max_range=engine.rig_cfg.max_range)


BATCHED_DETECTORS = ("GFT", "ORB", "FAST", "AGAST")   # the detection methods the sequence engines run


def set_detection_method(tracker, method):
    """tracker.detection_method = method (None: leave the tracker's own), and the feature matchers bootstrap_tracker built
    from it follow: the frames detect with their feature_detection_method."""
    if method is None:
        return
    tracker.detection_method = str(method).upper()
    cm = tracker.camera_model
    for fm in (getattr(cm, "feature_matcher_for_static_stereo", None), getattr(cm, "feature_matcher_for_motion", None)):
        if fm is not None:
            fm.feature_detection_method = tracker.detection_method


def parse_cross_check(cross_check):
    """run_VO's cross_check argument -> (static stereo, frame to frame) switches, or None for "the tracker's own setting":
    None -> None; True / False -> both matchers; "stereo" / "f2f" -> that matcher alone ("both", "none" are accepted too)."""
    if cross_check is None:
        return None
    if isinstance(cross_check, (bool, np.bool_)):
        return bool(cross_check), bool(cross_check)
    table = {"stereo": (True, False), "f2f": (False, True), "both": (True, True), "none": (False, False)}
    name = str(cross_check).lower()
    if not isinstance(cross_check, str) or name not in table:
        raise ValueError("cross_check: None, True, False, \"stereo\" or \"f2f\"; got %r" % (cross_check,))
    return table[name]


def _set_matcher_option(tracker, name, value, validate, setting, check, mirror):
    """What set_cross_check / set_gated_matching / set_ratio_test share.  value as parse_cross_check takes its argument (None:
    nothing happens); validate(stereo, f2f) checks the option's own values; an RGB-D tracker has the frame-to-frame matcher
    only (True / False / "f2f" set it, "stereo" is a ValueError); setting(on) -> the FeatureMatcher attributes of a matcher
    switched `on`, check(fm, on) raises what that matcher refuses (k_best > 1, radius match, float descriptors);
    mirror(stereo, f2f) -> the tracker's attributes.  Every matcher is checked before anything is kept: a refused setting
    leaves matchers and tracker as they were.  The matchers bootstrap_tracker built carry the setting, so the per-frame
    mirror path and the engine chosen from the tracker's settings both follow."""
    if value is None:
        return
    try:
        stereo, f2f = parse_cross_check(value)
    except ValueError:
        if name == "cross_check":
            raise
        raise ValueError("%s: None, True, False, \"stereo\", \"f2f\" or \"both\"; got %r" % (name, value))
    validate(stereo, f2f)
    cm = tracker.camera_model
    if _is_rgbd_model(cm):
        if isinstance(value, str) and stereo:
            raise ValueError("%s=%r: an RGB-D tracker has no static-stereo matcher" % (name, value))
        stereo = False
    matchers = [(fm, on) for fm, on in ((getattr(cm, "feature_matcher_for_static_stereo", None), stereo),
                                        (getattr(cm, "feature_matcher_for_motion", None), f2f)) if fm is not None]
    before = [{k: getattr(fm, k) for k in setting(on)} for fm, on in matchers]
    try:
        for fm, on in matchers:
            fm.__dict__.update(setting(on))
            check(fm, on)
    except ValueError:
        for (fm, _), old in zip(matchers, before):
            fm.__dict__.update(old)
        raise
    tracker.__dict__.update(mirror(stereo, f2f))


def set_cross_check(tracker, cross_check):
    """Switch the mutual-consistency filter (cv2.BFMatcher's crossCheck, camera_models.py:401) of the tracker's matchers:
    cross_check as parse_cross_check takes it (None: leave the tracker's own setting).  Who carries the switch, and what an
    RGB-D tracker refuses: _set_matcher_option."""
    _set_matcher_option(tracker, "cross_check", cross_check, lambda stereo, f2f: None, lambda on: dict(cross_check=on),
                        lambda fm, on: fm._check_cross_check(),
                        lambda stereo, f2f: dict(cross_check_static_stereo=stereo, cross_check_for_motion=f2f))


def set_gated_matching(tracker, gated_matching, gated_max_distance=None):
    """Switch the search under the pixel gates (FeatureMatcher.match_gated) of the tracker's matchers: gated_matching as
    parse_cross_check takes its argument (None: leave the tracker's own setting, and gated_max_distance is ignored);
    gated_max_distance: None = no cap, or 1 .. 256.  Who carries the switch, and what an RGB-D tracker refuses:
    _set_matcher_option."""
    cap = gated_max_distance      # (gated_flags: ValueError for a cap outside 1 .. 256; then an integer)
    _set_matcher_option(tracker, "gated_matching", gated_matching, lambda stereo, f2f: gated_flags(stereo, f2f, cap),
                        lambda on: dict(gated=on, gated_max_distance=None if cap is None else int(cap)),
                        lambda fm, on: on and fm._check_gated(cap),
                        lambda stereo, f2f: dict(gated_static_stereo=stereo, gated_for_motion=f2f,
                                                 gated_max_distance=None if cap is None else int(cap)))


def set_ratio_test(tracker, ratio_test, ratio=None):
    """Switch Lowe's ratio rule (FeatureMatcher's ratio: evaluated on the device, fused into the search) of the tracker's
    matchers: ratio_test as parse_cross_check takes its argument (None: leave the tracker's own setting, and ratio is
    ignored); ratio: a float in (0, 1) with ratio * 64 an integer (0.75: the reference's, camera_models.py:423), required
    when a matcher is switched on.  Who carries the setting, and what an RGB-D tracker refuses: _set_matcher_option."""
    of = lambda on: float(ratio) if on else None      # noqa: E731 (ratio_flags: ValueError for a ratio that is no 64th, or none)
    _set_matcher_option(tracker, "ratio_test", ratio_test, lambda stereo, f2f: ratio_flags(stereo, f2f, ratio),
                        lambda on: dict(ratio=of(on)), lambda fm, on: fm._check_ratio(),
                        lambda stereo, f2f: dict(ratio_static_stereo=of(stereo), ratio_for_motion=of(f2f)))


def set_subpixel_refinement(tracker, subpix, half=5):
    """Switch the sub-pixel refinement of the detected keypoints (cv2.cornerSubPix restated in integers, on the device:
    Context.refine_subpix, after the descriptors and before the static-stereo matching).  subpix: None = leave the tracker's
    own setting (and half is ignored), True / False; half: the window half-size 2 .. 5 (None: 5).  The static-stereo matcher
    bootstrap_tracker built carries the setting to the frames, so the per-frame mirror path and the engine chosen from the
    tracker's settings both follow.  An RGB-D tracker reads depth at the keypoints' integer pixels: True is a ValueError."""
    from .._lib import subpix_half      # (a name run_VO's arguments use too)
    if subpix is None:
        return
    if not isinstance(subpix, (bool, np.bool_)):
        raise ValueError("subpix_refine: None, True or False; got %r" % (subpix,))
    value = subpix_half(5 if half is None else half) if subpix else None     # (ValueError for a half outside 2 .. 5)
    cm = tracker.camera_model
    if value is not None and _is_rgbd_model(cm):
        raise ValueError("subpix_refine: an RGB-D tracker reads depth at the keypoints' integer pixels")
    fm = getattr(cm, "feature_matcher_for_static_stereo", None)
    if fm is not None:
        fm.subpix_half = value
    tracker.subpix_half = value


def set_f2f_tracker(tracker, f2f_tracker, lk=None):
    """Where the frame-to-frame correspondences come from.  f2f_tracker: None = leave the tracker's own setting (and lk must be
    None), "match" = the descriptor matcher (the reference's way), "lk" = pyramidal Lucas-Kanade tracking of the reference
    frame's stereo points into the current frame's gray panoramas (Context.track_lk; cv2.calcOpticalFlowPyrLK,
    camera_models.py:3070); lk: its settings, None / an LKOptions / a dict of its fields.  The camera model carries the setting
    to the frames (they keep their gray panoramas on the device), so the per-frame mirror path and the engine chosen from the
    tracker's settings both follow.  An RGB-D tracker refuses "lk"; so does a tracker whose frame-to-frame matcher has an
    option set (cross_check, gated_matching, ratio_test): the tracker replaces that matcher."""
    if f2f_tracker is None:
        if lk is not None:
            raise ValueError("lk settings without f2f_tracker=\"lk\"")
        return
    cm = tracker.camera_model
    opts = MatchOptions.from_matchers(None, getattr(cm, "feature_matcher_for_motion", None))
    value = f2f_tracker_options(f2f_tracker, lk, opts, rgbd=_is_rgbd_model(cm))
    tracker.lk_options = cm.lk_options = value


def set_cyclic_columns(tracker, on):
    """Cyclic panorama columns frame to frame.  on: None = leave the tracker's own setting, False = off,
    "seam_free" = True plus the seam-free front end (GUMStereo._front_end detects on the padded panoramas
    and unpads after the features, _refine_stereo_lk adds the halo before its upload and unpads after; ORB is refused),
    True = column `cols` is column 0 again: the frame-to-frame |du| gate is cyclic (on the host, in the gated search and in
    the assembles) and, with set_f2f_tracker(..., "lk"), so are the pyramids and the tracker.  Call it after set_f2f_tracker
    and the matcher's setters: it checks the panorama width against them.  The camera model carries the setting, so the
    per-frame mirror path and the engine chosen from the tracker's settings both follow.  An RGB-D tracker refuses True."""
    if on is None:
        return
    cm = tracker.camera_model
    value = False
    if on:
        if _is_rgbd_model(cm):
            raise ValueError("cyclic_columns: an RGB-D camera's pinhole image is not cyclic")
        fm, lk = getattr(cm, "feature_matcher_for_motion", None), getattr(tracker, "lk_options", None)
        value = StepOptions.of(gated_f2f=bool(getattr(fm, "gated", False)), ratio_f2f=getattr(fm, "ratio", None) is not None,
                               f2f_tracker="match" if lk is None else "lk", lk=lk, cyclic_columns=on,
                               rig=(cm.top_model.panorama.cols, cm.bot_model.panorama.cols), store_levels=LK_MAX_LEVELS,
                               order=("lk", "cyclic"), detection_method=tracker.detection_method).cyclic      # (the engines' check of the width, and only that)
    tracker.cyclic_columns = cm.cyclic_columns = value


def set_stereo_refinement(tracker, stereo_refine, stereo_lk=None):
    """Sub-pixel static stereo.  stereo_refine: None = leave the tracker's own setting (and stereo_lk must be None), False = off,
    "lk" = after the top / bottom matching the bottom keypoint of every matched pair is tracked from the top panorama into the
    bottom one by one-level Lucas-Kanade with the matcher's partner as the initial flow (Context.refine_stereo_lk; the
    cv2.calcOpticalFlowPyrLK(prevImg = top, nextImg = bottom) call of camera_models.py:3070); stereo_lk: its settings, None / a
    StereoLKOptions / a dict of its fields.  The static-stereo matcher bootstrap_tracker built carries the setting to the frames,
    so the per-frame mirror path and the engine chosen from the tracker's settings both follow.  An RGB-D tracker has no static
    stereo: "lk" is a ValueError."""
    if stereo_refine is None:
        if stereo_lk is not None:
            raise ValueError("stereo_lk settings without stereo_refine=\"lk\"")
        return
    cm = tracker.camera_model
    value = stereo_refine_options(None if stereo_refine is False else stereo_refine, stereo_lk, rgbd=_is_rgbd_model(cm))
    fm = getattr(cm, "feature_matcher_for_static_stereo", None)
    if fm is not None:
        fm.stereo_lk_options = value
    tracker.stereo_lk_options = value


def _has_batched_counterpart(tracker, fm):
    """Whether the sequence engines run what `tracker` is set to; fm: the matcher the family's frames detect with (None:
    none yet)."""
    method = str(tracker.detection_method).upper()
    return (method in BATCHED_DETECTORS and tracker.matching_type == "BF" and tracker.k_best_matches == 1
            and not tracker.use_descriptor_radius_match_for_motion
            and (fm is None or str(fm.feature_detection_method).upper() == method))


def _sos_engine_settings(tracker, camera_model, first_image):
    """What a sequence engine that computes what `tracker` (a TrackerStereoSE3 with the reference's settings) and
    StereoPanoramicFrame compute is built from -> (positional arguments after ctx, keyword arguments, cache key), or None
    when the configuration has no batched counterpart."""
    from ..frontend import mirror_kp_cap
    from ..pipeline import RigConfig
    om = camera_model
    method = str(tracker.detection_method).upper()
    fm = getattr(om, "feature_matcher_for_static_stereo", None)   # (what StereoPanoramicFrame detects with)
    if not _has_batched_counterpart(tracker, fm):
        return None
    top, bot = om.top_model, om.bot_model
    if not (np.array_equal(tracker.cam_rotations[0], np.identity(3)) and np.array_equal(tracker.cam_rotations[1], np.identity(3))
            and np.array_equal(tracker.cam_offsets[0], top.F[:3, 0]) and np.array_equal(tracker.cam_offsets[1], bot.F[:3, 0])):
        return None
    if om.current_omni_img is None:
        om.current_omni_img = first_image
    model = om._device_model()
    from_m = get_length_units_conversion_factor("m", om.units)
    geo = [(m.panorama.cols, m.panorama.rows, m.panorama.pixel_size, m.panorama.cyl_height_max) for m in (top, bot)]
    rig = RigConfig(pano_top=geo[0], pano_bot=geo[1], F_top=top.F[:3, 0], F_bot=bot.F[:3, 0], min_range=0.5 * from_m,
                    max_range=7.0 * from_m, stereo_min_disp=1.0, stereo_max_hdiff=2.5,
                    f2f_max_hdiff=tracker.max_horizontal_diff_f2f_matches, pct_good_matches=tracker.percentage_good_matches)
    nfeat = tracker.num_features_detection_for_static_stereo
    cap = mirror_kp_cap(method, nfeat)      # as GUMStereo._front_end (the mirror path's capacity)
    # the step options (what the mirror path runs) are part of the engine's key; one cap and one ratio serve both its matchers
    so = StepOptions.from_tracker(tracker, om)
    if so is None:
        return None
    key = (method, int(nfeat), cap, float(tracker.backprojection_score_threshold_3D_to_2D),
           int(tracker.max_ransac_iterations_3D_to_2D), float(tracker.max_horizontal_diff_f2f_matches),
           float(tracker.percentage_good_matches), tuple(geo[0]), tuple(geo[1]), tuple(top.F[:3, 0]), tuple(bot.F[:3, 0]), id(model), so)
    kwargs = dict(num_of_features=nfeat, kp_cap=cap, frame_cap=4096, median_win_size=11,
                  thr=tracker.backprojection_score_threshold_3D_to_2D, max_iter=tracker.max_ransac_iterations_3D_to_2D,
                  adaptive=True, lm_iter=pyopengv.LM_MAX_ITERATIONS, ransac_solver="GP3P", detection_method=method, **so.kwargs())
    return (model, rig), kwargs, key


class RGBDFrame(object):
    """pose_est_tools.py:404-623: one RGB-D frame = keypoints with valid depth, their descriptors, 3-D points and
    bearings.  Detection + description + back-projection run on the GPU (RGBDFrontEnd, one frame)."""

    def __init__(self, rgbd_camera_model, frame_id, **kwargs):
        self.rgbd_camera_model = rgbd_camera_model
        self.frame_id = frame_id
        self.parent_id = kwargs.get("parent_id", -1)
        self.T_frame_wrt_tracking_ref_frame = kwargs.get("T_wrt_ref", np.identity(4))
        self.conversion_factor_length_to_m = get_length_units_conversion_factor(rgbd_camera_model.units, "m")
        self.total_time = 0.
        self.median_win_size = 0
        self.min_range = 0.8
        self.max_range = 7.
        self.mask = kwargs.get("mask", None)
        self.rgb_img = kwargs.get("rgb_img", None)
        self.depth_map = kwargs.get("depth_map", None)
        self.num_valid_keypoints = 0
        self.keypoints_and_descriptors = None
        self.bearing_vectors = None
        self.keypoints_3D_points = None
        self.current_depth = None
        if (self.rgb_img is not None) and (self.depth_map is not None):
            self.establish_keypoints(rgb=self.rgb_img, depth=self.depth_map)

    def filter_3D_points_due_to_range(self, xyz_points_wrt_C, min_3D_range=0, max_3D_range=0.):
        """pose_est_tools.py:570-592 (numpy, as there)."""
        valid = np.ones(shape=(xyz_points_wrt_C.shape), dtype="bool")
        if min_3D_range > 0 or max_3D_range > 0:
            nrm = np.nan_to_num(np.linalg.norm(xyz_points_wrt_C, axis=0, keepdims=True), copy=True)
            if min_3D_range > 0:
                valid = np.logical_and(valid, nrm >= min_3D_range)
            if max_3D_range > 0:
                valid = np.logical_and(valid, nrm <= max_3D_range)
        return valid

    def establish_keypoints(self, rgb, depth):
        """pose_est_tools.py:600-623.  `rgb` is handed to the detector as it is (the gray conversion weights the
        first channel as blue, like cv2.COLOR_BGR2GRAY applied to whatever the caller passes, :531)."""
        fm = self.rgbd_camera_model.feature_matcher_for_motion
        method = "GFT" if fm is None else str(fm.feature_detection_method).upper()
        if method not in BATCHED_DETECTORS:
            raise NotImplementedError("RGB-D detection method %r: GFT (the trackers' default, pose_est_tools.py:684), ORB, "
                                      "FAST and AGAST are built" % method)
        nfeat = 50 if fm is None else fm.num_of_features
        self.current_depth = depth
        # (the depth of a keypoint is read at its truncated pixel, .astype(np.uint) at :611: sosvo_rgbd_assemble)
        fe = self.rgbd_camera_model._front_end(np.asarray(rgb).shape[:2], nfeat, self.median_win_size, self.min_range,
                                               self.max_range, self.mask, method)
        fe.load_frames(np.ascontiguousarray(rgb)[None], np.ascontiguousarray(depth, dtype=np.float32)[None])
        fe.run()
        fe.ctx.synchronize()
        M = int(fe.frames["M"][0])
        m = fe.frames["m"][0, :M].cpu().numpy()
        self.keypoints_3D_points = fe.frames["X"][0, :M].cpu().numpy()
        self.bearing_vectors = fe.frames["b"][0, :M].cpu().numpy()
        kpts = [KeyPoint(x, y, size=31.0) for x, y in m]
        self.keypoints_and_descriptors = KeyPointAndDescriptor(kpts_list=kpts, desc_list=fe.frames["d"][0, :M].cpu().numpy(),
                                                               coords_array=m.astype(np.float64), do_flattening=False)
        self.num_valid_keypoints = M


class _KeyFrame(object):
    """A frame promoted to keyframe: a blind copy of its attributes (pose_est_tools.py:625-641)."""

    def __init__(self, frame, **kwargs):
        if isinstance(frame, _DeviceFrame):   # (plain instance attributes only: the same blind copy, without dir())
            self.__dict__.update(frame.__dict__)
        else:
            copy_only_attributes(objfrom=frame, objto=self)
        self.children_ids = []


class StereoPanoramicKeyFrame(_KeyFrame, StereoPanoramicFrame):
    """pose_est_tools.py:625-632"""


class RGBDKeyFrame(_KeyFrame, RGBDFrame):
    """pose_est_tools.py:634-641"""


class DeviceRGBDFrame(_DeviceFrame, RGBDFrame):
    """An RGBDFrame whose keypoints, descriptors, points and bearings stay in the store of a pipeline.RGBDSequenceEngine."""

    @staticmethod
    def engine_consts(engine, rgbd_camera_model):
        return dict(
            rgbd_camera_model=rgbd_camera_model, total_time=0., mask=None, rgb_img=None, depth_map=None, current_depth=None,
            keypoints_and_descriptors=None, bearing_vectors=None, keypoints_3D_points=None,
            conversion_factor_length_to_m=get_length_units_conversion_factor(rgbd_camera_model.units, "m"),
            median_win_size=engine.cfg.median_ksize, min_range=engine.cam_cfg.min_range, max_range=engine.cam_cfg.max_range)


def _rgbd_engine_settings(tracker, camera_model, first_rgb):
    """As _sos_engine_settings for a TrackerRGBDSE3 and RGBDFrame."""
    from ..pipeline import RGBDCamConfig
    cm = camera_model
    method = str(tracker.detection_method).upper()
    fm = getattr(cm, "feature_matcher_for_motion", None)   # (what RGBDFrame detects with)
    if not _has_batched_counterpart(tracker, fm):
        return None
    cam = RGBDCamConfig(cm.fx, cm.fy, cm.center_x, cm.center_y, cm.focal_length_m, cm.depth_is_Z, 0.8, 7.0,
                        f2f_max_hdiff=tracker.max_horizontal_diff_f2f_matches, pct_good_matches=tracker.percentage_good_matches)
    shape = tuple(int(v) for v in np.asarray(first_rgb).shape[:2])
    so = StepOptions.from_tracker(tracker, cm)
    key = (method, shape, int(tracker.num_features_detection_for_motion), float(tracker.backprojection_score_threshold_3D_to_2D),
           int(tracker.max_ransac_iterations_3D_to_2D), float(tracker.max_horizontal_diff_f2f_matches),
           float(tracker.percentage_good_matches), str(tracker.pose_est_algorithm), float(cm.fx), float(cm.fy), float(cm.center_x),
           float(cm.center_y), float(cm.focal_length_m), bool(cm.depth_is_Z), so)
    kwargs = dict(image_shape=shape, num_of_features=tracker.num_features_detection_for_motion, median_win_size=0,
                  thr=tracker.backprojection_score_threshold_3D_to_2D, max_iter=tracker.max_ransac_iterations_3D_to_2D,
                  adaptive=True, lm_iter=pyopengv.LM_MAX_ITERATIONS, pose_est_algorithm=tracker.pose_est_algorithm,
                  detection_method=method, **so.match.rgbd_kwargs())
    return (cam,), kwargs, key


def _engine_settings(tracker, camera_model, first_image):
    """_sos_engine_settings or _rgbd_engine_settings, by the camera model's family."""
    return (_rgbd_engine_settings if _is_rgbd_model(camera_model) else _sos_engine_settings)(tracker, camera_model, first_image)


def _engine_for(tracker, camera_model, first_image, window, lanes=None):
    """The sequence engine (lanes None) or the multi-sequence engine of `lanes` lanes that computes what `tracker` and its
    family's frames compute -> (engine, settings key), or (None, None) when the configuration has no batched counterpart.
    An engine (frame store, pinned staging buffers, scratch) stays with the camera model and serves later runs with the same
    settings and window: building one costs more than tracking a hundred frames.  One engine per model and kind (a new
    configuration replaces the old one's buffers; a solo run between two multi-sequence runs does not evict their engine)."""
    from .. import pipeline
    settings = _engine_settings(tracker, camera_model, first_image)
    if settings is None:
        return None, None
    args, kwargs, key = settings
    multi = lanes is not None
    name = (("SequenceEngine", "MultiSequenceEngine"), ("RGBDSequenceEngine", "RGBDMultiSequenceEngine"))[_is_rgbd_model(camera_model)][multi]
    if multi:
        full, kwargs = key + (int(window), int(lanes)), dict(kwargs, lanes=lanes)
    else:
        full = key[:1] + (int(window),) + key[1:]
    cache = camera_model.__dict__.setdefault("_multi_sequence_engines" if multi else "_sequence_engines", {})
    eng = cache.get(full)
    if multi and eng is not None and (eng._error is not None or eng._live):
        eng = None          # (a device call failed, or a run is still on it: not reused)
    if eng is None:
        cache.clear()
        eng = cache[full] = getattr(pipeline, name)(camera_model._context(), *args, window=window, **kwargs)
    elif multi:
        eng.reset_counters()
    else:
        eng.reset()
    return eng, key


def sequence_engine_for(tracker, camera_model, first_image, window):
    """The pipeline.SequenceEngine that computes what `tracker` (a TrackerStereoSE3 with the reference's settings) and
    StereoPanoramicFrame compute, or None when the configuration has no batched counterpart (then run_VO keeps the
    per-frame mirror path)."""
    return _engine_for(tracker, camera_model, first_image, window)[0]


def rgbd_sequence_engine_for(tracker, camera_model, first_rgb, window):
    """The pipeline.RGBDSequenceEngine that computes what `tracker` (a TrackerRGBDSE3) and RGBDFrame compute, or None when
    the configuration has no batched counterpart (then run_VO keeps the per-frame mirror path)."""
    return _engine_for(tracker, camera_model, first_rgb, window)[0]


def multi_sequence_engine_for(tracker, camera_model, first_image, window, lanes):
    """The pipeline.MultiSequenceEngine / RGBDMultiSequenceEngine of `lanes` lanes with the settings sequence_engine_for /
    rgbd_sequence_engine_for would give a single-sequence engine -> (engine, settings key), or (None, None) when the
    configuration has no batched counterpart."""
    return _engine_for(tracker, camera_model, first_image, window, lanes)


class TrackerRGBDSE3(TrackerSE3):
    """pose_est_tools.py:880-958: central 3D-2D tracking of RGB-D frames."""
    refuses_without_model = True
    chain_pose = staticmethod(tr.concatenate_matrices)     # (multiplies into an identity first, as the reference does here)

    def __init__(self, camera_model, show_3D_points=False, **kwargs):
        TrackerSE3.__init__(self, camera_model, show_3D_points, **kwargs)
        self.number_of_cams = 1
        self.T_C_wrt_S_init = np.identity(4)
        self.T_C_curr_frame_wrt_S_est = kwargs.get("T_C_wrt_S_init", self.T_C_wrt_S_init)
        self.bootstrap_tracker()

    def bootstrap_tracker(self):
        """pose_est_tools.py:956-958"""
        self.camera_model.feature_matcher_for_motion = FeatureMatcher(
            method=self.detection_method, matcher_type=self.matching_type, k_best=self.k_best_matches,
            percentage_good_matches=self.percentage_good_matches, num_of_features=self.num_features_detection_for_motion,
            use_radius_match=self.use_descriptor_radius_match_for_motion, cross_check=self.cross_check_for_motion,
            gated=self.gated_for_motion, gated_max_distance=self.gated_max_distance, ratio=self.ratio_for_motion)
        self.max_horizontal_diff_f2f_matches = self.max_horizontal_search_ratio * (self.camera_model.center_x * 2.)

    def track_frame(self, reference_frame, current_frame):
        """pose_est_tools.py:896-954 -> (ok, message)."""
        self.num_tracked_correspondences = 0
        self.inlier_tracked_correspondences_ratio = 0.
        if isinstance(current_frame, _DeviceFrame):
            return self._track_device_frame(reference_frame, current_frame)
        ref, cur = reference_frame.keypoints_and_descriptors, current_frame.keypoints_and_descriptors
        (t_idx, _, _), (q_idx, _, _), _ = match_features_frame_to_frame(
            cam_model=self.camera_model, train_kpts=ref.keypoints, train_desc=ref.descriptors, query_kpts=cur.keypoints,
            query_desc=cur.descriptors, random_colors_RGB=ref.random_colors_RGB,
            keypts_as_points_train=ref.pixel_coords, keypts_as_points_query=cur.pixel_coords,
            max_horizontal_diff=self.max_horizontal_diff_f2f_matches, max_descriptor_distance_radius=-1)
        t_idx, q_idx = np.asarray(t_idx, dtype=np.int64), np.asarray(q_idx, dtype=np.int64)
        num_initial_matches = len(t_idx)
        if num_initial_matches < self.min_matches_to_track():
            return False, "Cannot track on only %d point correspondences" % (num_initial_matches)
        b = current_frame.bearing_vectors[q_idx]
        p = reference_frame.keypoints_3D_points[t_idx]
        T_ransac, inliers = pyopengv.absolute_pose_ransac(b[..., :3], p[..., :3], self.pose_est_algorithm,
                                                          self.backprojection_score_threshold_3D_to_2D,
                                                          self.max_ransac_iterations_3D_to_2D)
        self.num_tracked_correspondences = len(inliers)
        self.inlier_tracked_correspondences_ratio = float(self.num_tracked_correspondences) / float(num_initial_matches)
        if self.num_tracked_correspondences < self.n_points_for_RANSAC_model:
            # no consensus model (e.g. EPNP on an exactly coplanar point set, where it has no solution): report the
            # frame as not tracked instead of refining from an empty inlier set
            return False, "RANSAC (%s) found no model among %d correspondences" % (self.pose_est_algorithm, num_initial_matches)
        T_nl = pyopengv.absolute_pose_optimize_nonlinear(b[inliers], p[inliers], T_ransac[:3, 3], T_ransac[:3, :3])
        self._keep_pose(current_frame, T_nl)
        if self.show_3D_points:
            self.xyz_homo_points_wrt_C_inliers = np.hstack((p[inliers] * current_frame.conversion_factor_length_to_m,
                                                            np.ones((len(inliers), 1))))
        return True, "tracking used %d inlier point correspondences" % (self.num_tracked_correspondences)


# A tracker's construction writes to its camera model (the feature matchers; bootstrap_tracker regenerates the azimuthal masks
# of the panoramas in place), and an engine is built from the model's masks: the lanes of run_VO_many share one camera model,
# so both happen under this lock (a solo run_VO finds it free).
_CAMERA_MODEL_LOCK = threading.RLock()


def _is_rgbd_model(camera_model):
    from .camera_models import RGBDCamModel
    return isinstance(camera_model, RGBDCamModel)


def sequence_windows(it, eng, W, images_of, engine_state, on_window=None, stop=None):
    """run_VO's sequence mode: the items (frame index, image, depth map or None) of the iterator `it`, `W` at a time through
    the batched front end of `eng` (a pipeline.SequenceEngine / RGBDSequenceEngine), yielded one by one as
    (frame index, image, None, record dict, position in the sequence).  images_of(list of items) -> what eng.stage_host
    takes; engine_state: run_VO's counters ("window_s", "windows"); on_window() is called when a window's records are in,
    before its frames are yielded (run_VO writes the previous window's lines there); stop: the event that ends the helper
    thread (default: a new one; set when the generator ends).
    A source that raises ends the run after the frames read before the failure, as the per-frame path does.  However the
    generator ends (exhausted, failed, closed), no call of this run reaches the engine once it has: the engine goes to the
    next run with the same camera model (sequence_engine_for), and a late upload would put this run's frames into its
    buffers.  The helper thread is joined unless it is waiting for a source that blocks (a live camera); then it leaves
    without touching the engine when the source returns."""
    import queue
    W = int(W)
    stop = threading.Event() if stop is None else stop
    failed = []      # a read that failed after some frames of a window: raised by the next read, once those are processed

    def next_chunk():
        if failed:
            raise failed.pop()
        chunk = []
        try:
            for item in it:
                chunk.append(item)
                if len(chunk) >= W:
                    break
        except Exception as e:
            if not chunk:
                raise
            failed.append(e)
        return chunk
    chunk = next_chunk()
    if not chunk:
        return
    # a helper thread pulls the NEXT window from the source and copies it into the engine's other pinned buffer while
    # this one is processed (the copy releases the GIL); a buffer returns to the thread after its upload was synchronised
    free, ready = queue.Queue(), queue.Queue()
    free.put(1)
    # the helper thread holds `lock` while it calls the engine and checks `stop` under it; `reading` says it waits in the source
    lock, reading = threading.Lock(), [False]

    def producer():
        try:
            while True:
                with lock:
                    if stop.is_set():
                        break
                    reading[0] = True
                try:
                    c = next_chunk()
                finally:
                    with lock:
                        reading[0] = False
                if not c:
                    break
                b = free.get()
                if b is None:
                    break
                with lock:
                    if stop.is_set():
                        break
                    t0 = time.perf_counter()
                    eng.stage_host(images_of(c), b)
                    eng.stage_s["stage_to_pinned"] += time.perf_counter() - t0
                    if stop.is_set():
                        break
                    if eng.early_upload:
                        eng.upload_staged(b, len(c))   # the copy to the device starts now, beside the current window's kernels
                ready.put((c, b))
            ready.put((None, None))
        except BaseException as e:   # handed to the consumer
            ready.put((e, None))
    t0 = time.perf_counter()
    eng.stage_host(images_of(chunk), 0)
    eng.stage_s["stage_to_pinned"] += time.perf_counter() - t0
    worker = threading.Thread(target=producer, name="sosvo-stage", daemon=True)
    worker.start()
    seq_index, buf = 0, 0
    try:
        t0 = time.perf_counter()
        eng.enqueue_staged(buf, len(chunk))
        engine_state["window_s"] += time.perf_counter() - t0
        while chunk:
            t0 = time.perf_counter()
            infos = eng.collect()                        # (synchronises: the upload from `buf` is complete)
            engine_state["windows"] += 1
            free.put(buf)
            # the next window goes onto the GPU BEFORE this one's records are worked through, when the helper thread
            # has it staged already (an image sequence: nearly always; a live source: never -- its frames are not
            # held back for it)
            nxt = None
            if eng.enqueue_ahead:
                try:
                    nxt = ready.get_nowait()
                except queue.Empty:
                    nxt = None
                if nxt is not None and nxt[0] is not None and not isinstance(nxt[0], BaseException):
                    eng.enqueue_staged(nxt[1], len(nxt[0]))
            engine_state["window_s"] += time.perf_counter() - t0
            if on_window is not None:
                on_window()                              # (run_VO: the previous window's lines, off the per-frame path)
            for item, info in zip(chunk, infos):
                yield item[0], item[1], None, info, seq_index
                seq_index += 1
            if nxt is None:
                nxt = ready.get()
                if nxt[0] is not None and not isinstance(nxt[0], BaseException):
                    t0 = time.perf_counter()
                    eng.enqueue_staged(nxt[1], len(nxt[0]))
                    engine_state["window_s"] += time.perf_counter() - t0
            chunk, buf = nxt
            if isinstance(chunk, BaseException):
                raise chunk
    finally:
        stop.set()
        free.put(None)
        with lock:                   # (waits for an engine call in flight; after it the thread makes none)
            in_source = reading[0]
        if not in_source:            # (otherwise it ends when the source returns)
            worker.join()


def _tum_fields(t, q):
    """" tx ty tz qx qy qz qw" + newline of a translation and a quaternion (w first), every number as its repr."""
    return " %s %s %s %s %s %s %s\n" % (repr(t[0]), repr(t[1]), repr(t[2]), repr(q[1]), repr(q[2]), repr(q[3]), repr(q[0]))


class _VOOutput(object):
    """What run_VO says and writes: printed_messages.log and stdout, the two TUM pose files and keyframe_ids.txt.
    Sequence mode keeps the per-frame host work small: messages and pose lines are collected and written once per window
    (same text, same order), the quaternions of a window's poses come from ONE batched eigen-decomposition
    (tr.quaternions_from_matrices: bit-identical rows).  The per-frame paths (frame_window 0, live sources) flush every frame."""

    def __init__(self, results_path):
        self.log = open(os.path.join(results_path, "printed_messages.log"), "w")
        self.results_path = results_path
        self.out_msgs, self.log_only, self.pending, self.kf_lines = [], [], [], []   # stdout + log | log only | poses | keyframes
        self.say = self.out_msgs.append

    def open_pose_files(self, est_poses_filename):
        self.est_path = os.path.join(self.results_path, est_poses_filename)
        self.kf_path = os.path.join(self.results_path, "keyframe_ids.txt")
        self.est_file = open(self.est_path, "w")
        self.gt_file = open(self.est_path.replace("estimated", "gt_associated"), "w")
        self.kf_file = open(self.kf_path, "w")

    def say_to_log_only(self, msg):
        self.log_only.append((len(self.out_msgs), msg))     # (a failure message goes to the log only, where it was said)

    def pose(self, idx, T_est, T_gt):
        """(TUM lines idx tx ty tz qx qy qz qw, :1611-1621, with quaternion_from_matrix(isprecise=False): formatted by flush)"""
        self.pending.append((idx, T_est, T_gt))

    def keyframe(self, idx):
        self.kf_lines.append("%d\n" % idx)

    def flush(self):
        out_msgs, log_only, pending = self.out_msgs, self.log_only, self.pending
        if out_msgs or log_only:
            if out_msgs:
                print("\n".join(out_msgs))
            lines, extra = list(out_msgs), sorted(log_only, key=lambda e: e[0], reverse=True)
            for pos, line in extra:
                lines.insert(pos, line)
            self.log.write("\n".join(lines) + "\n")
            del out_msgs[:], log_only[:]
        if pending:
            idxs = [p_[0] for p_ in pending]
            Te = np.stack([p_[1] for p_ in pending])
            qe, te = tr.quaternions_from_matrices(Te).tolist(), Te[:, :3, 3].tolist()
            self.est_file.write("".join("%d%s" % (i, _tum_fields(t, q)) for i, t, q in zip(idxs, te, qe)))
            gts = [p_[2] for p_ in pending]
            uniq = {}
            for g in gts:                        # (one shared identity for a run without ground truth: decomposed once)
                uniq.setdefault(id(g), g)
            keys = list(uniq)
            Tg = np.stack([uniq[k_] for k_ in keys])
            bad = np.isnan(Tg).any(axis=(1, 2))
            qg = tr.quaternions_from_matrices(np.where(bad[:, None, None], np.identity(4), Tg)).tolist()
            tg = Tg[:, :3, 3].tolist()
            line_of = {k_: " nan nan nan nan nan nan nan\n" if b_ else _tum_fields(t, q) for k_, b_, t, q in zip(keys, bad.tolist(), tg, qg)}
            self.gt_file.write("".join("%d%s" % (i, line_of[id(g)]) for i, g in zip(idxs, gts)))
            del pending[:]

    def close(self):
        self.flush()
        self.kf_file.write("".join(self.kf_lines))
        for f in (self.est_file, self.gt_file, self.kf_file, self.log):
            f.close()


def _file_frames(camera_model, image_names, depth_names, indices):
    """(frame index, image, depth map or None) from the files of a sequence (depth_names None: no depth maps); the next frame
    is decoded on a helper thread while the current one is tracked (the decoder releases the GIL)."""
    from concurrent.futures import ThreadPoolExecutor
    from .common_cv import get_depthmap_float32_from_png, imread

    def load(k):
        img = imread(image_names[k])
        if img is None:   # (imread's None for a file it cannot decode ends the run here, for every frame window alike)
            raise OSError("cannot read the image file %s" % image_names[k])
        if depth_names is not None:
            # the reference converts BGR -> RGB (:1430) and then treats the array as BGR (:531): reproduced as is
            return indices[k], np.ascontiguousarray(img[..., ::-1]), \
                get_depthmap_float32_from_png(depth_names[k], camera_model.scaling_factor)
        return indices[k], img, None
    with ThreadPoolExecutor(max_workers=1) as pool:
        pending = pool.submit(load, 0) if len(indices) else None
        for k in range(len(indices)):
            item = pending.result()
            pending = pool.submit(load, k + 1) if k + 1 < len(indices) else None
            yield item


def _windowed_frames(source, frame_window, engine_for, tracker, camera_model, engine_state, on_window):
    """The frames of source(), `frame_window` at a time through the batched front end of the engine that
    engine_for(tracker, camera_model, first image, frame_window) gives on the first frame (kept in engine_state); no batched
    counterpart of this configuration: the frames as they are, for the per-frame path."""
    W = int(frame_window)
    it = iter(source())
    first = next(it, None)
    if first is None:
        return
    engine_state["tried"] = True
    eng = engine_state["engine"] = engine_for(tracker, camera_model, first[1], W)
    it = itertools.chain([first], it)
    if eng is None:
        yield from it
        return
    images_of = (lambda c: [(item[1], item[2]) for item in c]) if _is_rgbd_model(camera_model) else (lambda c: [item[1] for item in c])
    yield from sequence_windows(it, eng, W, images_of, engine_state, on_window=on_window)


def _ground_truth_of(gt_poses_filename, camera_model, T_C_wrt_S_init, img_indices, live):
    """-> the function frame index -> ground-truth pose T_gt in the frame the estimates are in.  No ground-truth file (a live
    run has none, :1012): one shared identity for every frame; a frame the file has no pose for: NaN (a live run: identity)."""
    from .common_tools import get_poses_from_file
    pose_output_file_units = "m"
    have_file = gt_poses_filename is not None and os.path.exists(gt_poses_filename)
    if have_file:
        _, gt_list = get_poses_from_file(poses_filename=gt_poses_filename, input_units="m",
                                         output_working_units=pose_output_file_units, indices=[], pose_format="tum",
                                         zero_up_wrt_origin=True)
    else:
        gt_list = max(len(img_indices), img_indices[-1] + 1) * [np.identity(4)]
    T_Rgt_wrt_S = T_S_wrt_Rgt = None
    if have_file and getattr(camera_model, "T_Cest_wrt_Rgt", None) is not None:
        # fixed hand-eye transformation between the estimated camera frame and the ground-truth rig frame (:1362-1367)
        k_units = get_length_units_conversion_factor(camera_model.units, pose_output_file_units)
        T_Cest_wrt_Rgt = np.array(camera_model.T_Cest_wrt_Rgt, dtype=np.float64, copy=True)
        T_Cest_wrt_Rgt[:3, 3] = k_units * T_Cest_wrt_Rgt[:3, 3]
        T_Rgt_wrt_S = tr.concatenate_matrices(T_C_wrt_S_init, tr.inverse_matrix(T_Cest_wrt_Rgt))
        T_S_wrt_Rgt = tr.inverse_matrix(T_Rgt_wrt_S)

    def T_gt_of(idx):
        T_gt = gt_list[idx] if idx < len(gt_list) else (np.identity(4) if live else np.full((4, 4), np.nan))
        if T_Rgt_wrt_S is not None:
            T_gt = tr.concatenate_matrices(T_Rgt_wrt_S, T_gt, T_S_wrt_Rgt)   # :1472
        return T_gt
    return T_gt_of


# the share of the running average of tracked correspondences / of the keyframe's keypoints a new keyframe needs (:1308-1313)
KEYFRAME_MIN_TRACKED, KEYFRAME_MIN_KEYPOINTS = 0.10, 0.10


def keyframe_policy(dist, ang, n_tracked, tracked_prev_avg, M_F, M_K, thresholds, prefix="", idx=0, tracked_wrt_keyframe=0):
    """The keyframe policy (:1516-1550) for a tracked frame: dist [m] and ang [radians] of its pose wrt the keyframe, n_tracked
    correspondences per camera against the average tracked_prev_avg since the keyframe, M_F / M_K valid keypoints of the frame /
    the keyframe, thresholds = (pos_thr, pos_max, ang_thr, ang_max); prefix, idx and tracked_wrt_keyframe go into the message
    -> (create a keyframe, the message to say or None)."""
    pos_thr, pos_max, ang_thr, ang_max = thresholds
    if not ((pos_thr < dist < pos_max) or (ang_thr < ang < ang_max)):
        return False, None
    if not (n_tracked > KEYFRAME_MIN_TRACKED * tracked_prev_avg and M_F > KEYFRAME_MIN_KEYPOINTS * M_K):
        return False, "%sFrame [%d] as Keyframe...doesn't satisfy %d > %.2f * %.2f and %d > %.2f * %.2f" % (
            prefix, idx, n_tracked, KEYFRAME_MIN_TRACKED, tracked_prev_avg, M_F, KEYFRAME_MIN_KEYPOINTS, M_K)
    reason = None
    if pos_thr < dist < pos_max:
        if ang < ang_max:
            reason = "translation %.2f < %.4f < %.2f [m]" % (pos_thr, dist, pos_max)
    elif ang_thr < ang:
        if dist < pos_max < ang_max:   # as written in the reference (:1534)
            reason = " rotation: %.2f > %.2f [radians]" % (ang, ang_thr)
    if reason is None:
        return False, "%sFrame [%d] as failed to create Keyframe due to some CRAZYNESS" % (prefix, idx)
    return True, "%sFrame [%d] as Keyframe due to %s... with %d tracked keypoint correspondences after tracking %d frames" % (
        prefix, idx, reason, n_tracked, tracked_wrt_keyframe)


def _vo_summary(prefix, number_of_keyframes, acc, n_done, est_path, kf_path):
    """The closing message of a run from its accumulators (process time per phase, tracked correspondences, inlier ratios)."""
    d = float(max(n_done, 1))
    return "\n".join([
        "%sVO done with %d keyframes" % (prefix, number_of_keyframes),
        "Image Read Avg Time: {time:.8f} seconds".format(time=acc["read"] / d),
        "Frame Setup Avg Time: {time:.8f} seconds".format(time=acc["setup"] / d),
        "Frame Tracking Avg Time: {time:.8f} seconds".format(time=acc["track"] / d),
        "Overall Frame VO Avg Time: {time:.8f} seconds".format(time=acc["vo"] / d),
        "Total Number of tracked correspondences: {corrs}".format(corrs=int(acc["corr"])),
        "Average Number of tracked correspondences: {corrs}".format(corrs=int(int(acc["corr"]) / d)),
        "Average tracked correspondences RANSAC inlier ratio: {ratio:.8f}".format(ratio=acc["ratio"] / d),
        "Estimated poses in TUM format SAVED as " + est_path,
        "Keyframes (indices) SAVED as " + kf_path])


def run_VO(visualizer_3D_VO, camera_model, gt_poses_filename=None, est_poses_filename="estimated_frame_poses_TUM.txt",
           img_filename_template=None, depth_filename_template=None, img_indices=(), results_path="~/temp", thread_name="",
           _live_frames=None, _keyframe_thresholds=None, frame_window=None, detection_method=None, _engine_for=None,
           cross_check=None, gated_matching=None, gated_max_distance=None, ratio_test=None, ratio=None,
           subpix_refine=None, subpix_half=None, f2f_tracker=None, lk=None, stereo_refine=None, stereo_lk=None, cyclic_columns=None):
    """pose_est_tools.py:1264-1678 without the 3-D visualisation (visualizer_3D_VO must be None): the frame loop,
    the keyframe policy (translation 0.01-0.20 m or rotation 1-10 degrees wrt the keyframe, enough tracked
    correspondences and keypoints), pose chaining through the keyframes, and the result files
        estimated_frame_poses_TUM.txt, gt_associated_frame_poses_TUM.txt  "idx tx ty tz qx qy qz qw" [m]
        keyframe_ids.txt, printed_messages.log
    -> dict(poses=[(idx, T 4x4)], keyframe_ids=[...], tracked=number of tracked frames, message=summary).

    frame_window: SEQUENCE MODE (pipeline.SequenceEngine / RGBDSequenceEngine): the front ends of `frame_window` frames
    run as ONE batch on the GPU and the frames are tracked from the device-resident frame store (speculatively against
    their predecessors, serially against the keyframe where that guess fails).  None = 32 for an image sequence, 1 for a
    live source; 0 = the per-frame mirror path (StereoPanoramicFrame on host arrays, one set of C-ABI calls per stage).
    The pose file does not depend on the window size (byte-identical for 1, 2, 32, ...); the mirror path agrees with
    it to rounding (its bearings go through numpy's trigonometry, the store's through the library's).

    detection_method: "GFT", "ORB", "FAST" or "AGAST" for the tracker and its frames; None = the tracker's own (GFT).

    cross_check, gated_matching / gated_max_distance, ratio_test / ratio, subpix_refine / subpix_half, f2f_tracker / lk,
    stereo_refine / stereo_lk, cyclic_columns: the step options.  Each is None = the tracker's own setting (off; "match"), or
    what its setter takes and describes: set_cross_check (True / False = both matchers, "stereo" / "f2f" = the static-stereo /
    the frame-to-frame matcher alone), set_gated_matching and set_ratio_test (the same values), set_subpixel_refinement,
    set_f2f_tracker, set_stereo_refinement, set_cyclic_columns.  Sequence mode and the mirror path follow alike.  An RGB-D
    camera model has the frame-to-frame matcher only: it refuses "stereo", sub-pixel keypoints, "lk" and cyclic columns."""
    from .common_cv import get_images
    if visualizer_3D_VO is not None:
        raise NotImplementedError("3-D visualisation is not built: pass visualizer_3D_VO=None")
    pyopengv.set_seed(0)  # a run is a pure function of its inputs (OpenGV seeds its sampler from the clock)
    prefix = thread_name + ": " if len(thread_name) > 0 else ""
    rgbd = _is_rgbd_model(camera_model)
    trackerClass, KeyFrameClass = (TrackerRGBDSE3, RGBDKeyFrame) if rgbd else (TrackerStereoSE3, StereoPanoramicKeyFrame)
    results_path = os.path.realpath(os.path.expanduser(results_path))
    make_sure_path_exists(results_path)
    out = _VOOutput(results_path)
    # indoor thresholds (pose_est_tools.py:1308-1313); run_VO_live passes its own (:991-1003)
    thresholds = _keyframe_thresholds or (0.01, 0.20, np.deg2rad(1.0), np.deg2rad(10.0))
    if _live_frames is None:
        image_names = get_images(img_filename_template, indices_list=img_indices, return_names_only=True)
        depth_names = get_images(depth_filename_template, indices_list=img_indices, return_names_only=True) if rgbd else None
        if img_indices is None or len(img_indices) == 0:
            img_indices = list(range(len(image_names)))
        frames = functools.partial(_file_frames, camera_model, image_names, depth_names, img_indices)
    else:
        img_indices = [0]
        frames = _live_frames
    with _CAMERA_MODEL_LOCK:
        tracker = trackerClass(camera_model=camera_model, show_3D_points=False, results_path=results_path)
        set_detection_method(tracker, detection_method)   # (before the engine is chosen: it runs the tracker's detector)
        set_cross_check(tracker, cross_check)             # (likewise: it runs the matchers' crossCheck)
        set_gated_matching(tracker, gated_matching, gated_max_distance)   # (... and their search under the gates)
        set_ratio_test(tracker, ratio_test, ratio)                        # (... and their ratio rule)
        set_subpixel_refinement(tracker, subpix_refine, subpix_half)      # (... and the frames' sub-pixel keypoints)
        set_f2f_tracker(tracker, f2f_tracker, lk)                         # (... and tracking in place of the f2f matcher)
        set_stereo_refinement(tracker, stereo_refine, stereo_lk)          # (... and the sub-pixel static stereo)
        set_cyclic_columns(tracker, cyclic_columns)                       # (... and the seam; after the matcher's and the tracker's)
    if frame_window is None:
        frame_window = 32 if _live_frames is None else 1
    engine_state = dict(engine=None, tried=False, window_s=0.0, windows=0)
    if int(frame_window) > 0:   # sequence mode: the same frames, `frame_window` at a time through the batched front end
        # (_engine_for: run_VO_many hands a lane of its multi-sequence engine to each of its runs)
        engine_for = _engine_for or (rgbd_sequence_engine_for if rgbd else sequence_engine_for)
        frames = functools.partial(_windowed_frames, frames, frame_window, engine_for, tracker, camera_model, engine_state, out.flush)
    T_gt_of = _ground_truth_of(gt_poses_filename, camera_model, tracker.T_C_wrt_S_init, img_indices, live=_live_frames is not None)
    out.open_pose_files(est_poses_filename)

    reference_frame, current_frame = None, None
    create_keyframe = True
    current_keyframe_id = img_indices[0]
    tracked_wrt_keyframe = 0
    tracked_prev_avg = 0.
    inlier_ratio_cma = tracker.inlier_tracked_correspondences_ratio
    acc = dict(read=0., setup=0., track=0., vo=0., corr=0., ratio=0.)
    poses_out, keyframe_ids = [], []
    n_done = 0
    frame_iter = iter(frames())
    img_index_number = -1
    try:
        while True:
            t_frame = t0 = time.process_time()
            try:
                item = next(frame_iter)
            except StopIteration:
                break
            idx, img, depth_map = item[:3]
            dev_info = item[3] if len(item) > 3 else None
            img_index_number += 1
            t1 = time.process_time()
            if img_index_number > 0:
                acc["read"] += t1 - t0
            t0 = t1
            if dev_info is not None:
                current_frame = (DeviceRGBDFrame if rgbd else DeviceStereoFrame)(
                    engine_state["engine"], dev_info, camera_model, frame_id=idx, seq_index=item[4], parent_id=current_keyframe_id)
            elif rgbd:
                current_frame = RGBDFrame(rgbd_camera_model=camera_model, frame_id=idx, rgb_img=img, depth_map=depth_map,
                                          parent_id=current_keyframe_id)
            else:
                camera_model.set_current_omni_image(img, generate_panoramas=False, view=False, apply_mask=True, mask_RGB=(0, 0, 0))
                current_frame = StereoPanoramicFrame(stereo_camera_model=camera_model, frame_id=idx, parent_id=current_keyframe_id)
            t1 = time.process_time()
            if img_index_number > 0:
                acc["setup"] += t1 - t0
            T_gt = T_gt_of(idx)
            if img_index_number > 0:
                t0 = t1
                ok, msg = tracker.track_frame(reference_frame=reference_frame, current_frame=current_frame)
                if not ok:
                    out.say_to_log_only(msg)
                    warn("%sWarning failed: %s" % (prefix, msg))
                    break
                reference_frame.children_ids.append(current_frame.frame_id)
                tracked_wrt_keyframe += 1
                acc["track"] += time.process_time() - t0
                n_tracked = tracker.num_tracked_correspondences / float(tracker.number_of_cams)
                acc["corr"] += n_tracked
                create_keyframe, msg = keyframe_policy(
                    tr.rpe_translation_metric(current_frame.T_frame_wrt_tracking_ref_frame),
                    tr.rpe_rotation_metric(current_frame.T_frame_wrt_tracking_ref_frame), n_tracked, tracked_prev_avg,
                    current_frame.num_valid_keypoints, reference_frame.num_valid_keypoints, thresholds, prefix, idx, tracked_wrt_keyframe)
                if msg is not None:
                    out.say(msg)
                tracked_prev_avg = (n_tracked + (float(tracked_wrt_keyframe) - 1.) * tracked_prev_avg) / float(tracked_wrt_keyframe)
                acc["ratio"] += tracker.inlier_tracked_correspondences_ratio
                inlier_ratio_cma = (tracker.inlier_tracked_correspondences_ratio + float(img_index_number - 1) * inlier_ratio_cma) \
                    / float(img_index_number)
            if create_keyframe:
                tracked_wrt_keyframe = 0
                tracked_prev_avg = 0.
                reference_frame = KeyFrameClass(frame=current_frame)
                if dev_info is not None:
                    current_frame.promote()   # the frame's record moves to the store's keyframe slot
                current_keyframe_id = reference_frame.frame_id
                out.keyframe(current_keyframe_id)
                keyframe_ids.append(current_keyframe_id)
                if len(tracker.T_Ckey_wrt_S_est_list) > 0:
                    T_key = tr.concatenate_matrices(tracker.T_Ckey_wrt_S_est_list[-1], reference_frame.T_frame_wrt_tracking_ref_frame)
                else:
                    T_key = tracker.T_C_curr_frame_wrt_S_est
                tracker.T_Ckey_wrt_S_est_list.append(T_key)
                create_keyframe = False
            T_now = np.array(tracker.T_C_curr_frame_wrt_S_est, copy=True)
            out.pose(idx, T_now, T_gt)
            poses_out.append((idx, T_now))
            if img_index_number > 0:
                acc["vo"] += time.process_time() - t_frame
            n_done = img_index_number
            out.say("%sDONE with F[%d] (Parent K[%d]). C.M.Avg. RANSAC inlier ratio = %.3f"
                % (prefix, current_frame.frame_id, current_frame.parent_id, inlier_ratio_cma))
            if dev_info is None:   # (sequence mode: lines are written once per window, out.flush in the window generator)
                out.flush()
        summary = _vo_summary(prefix, len(keyframe_ids), acc, n_done, out.est_path, out.kf_path)
        out.say(summary)
    finally:   # (an exception too: the lines of the frames tracked so far and the keyframe file are written)
        close = getattr(frame_iter, "close", None)
        if close is not None:
            close()   # (sequence mode: its staging thread ends before the engine can go to another run)
        out.close()
    result = dict(poses=poses_out, keyframe_ids=keyframe_ids, tracked=n_done, message=summary)
    if engine_state["engine"] is not None:
        eng = engine_state["engine"]
        result["sequence_mode"] = dict(frame_window=eng.W, windows=engine_state["windows"], serial_tracking_calls=eng.serial_calls,
                                       front_end_and_speculation_s=engine_state["window_s"], stage_s=dict(eng.stage_s))
    return result


def run_VO_live(visualizer_3D_VO, camera_model, cam_working_thread, est_poses_filename="estimated_frame_poses_TUM.txt",
                results_path="~/temp", thread_name="", frame_window=None, detection_method=None, cross_check=None,
                gated_matching=None, gated_max_distance=None, ratio_test=None, ratio=None,
                subpix_refine=None, subpix_half=None, f2f_tracker=None, lk=None, stereo_refine=None, stereo_lk=None, cyclic_columns=None):
    """pose_est_tools.py:960-1262: the VO loop on the frames of a running camera thread.  `cam_working_thread` is the
    reference's CamAsWorkingThread contract (webcam_live.py:256-291; `omnistereo.webcam_live.FrameSourceThread` here):
    `.current_frame` = the most recent omni image (None when the source ends), `.quit_flag`.  Each pass of the loop
    takes whatever frame is current (frames arriving faster than the tracker are skipped, a frame still current is
    processed again, as in the reference), numbers it 0, 1, 2, ... and runs run_VO's frame body with the live keyframe
    thresholds (:998-1003: translation 0.05-0.50 m or rotation 5-60 degrees); omnistereo models only (:1066-1073)."""
    if _is_rgbd_model(camera_model):
        raise NotImplementedError("run_VO_live tracks omnistereo models only (the RGB-D branch of the reference is commented out, :1069-1073)")

    def frames():
        idx = 0
        while not cam_working_thread.quit_flag:   # :1051
            img = cam_working_thread.current_frame
            if img is None:
                break
            yield idx, img, None
            idx += 1
    return run_VO(visualizer_3D_VO, camera_model, gt_poses_filename=None, est_poses_filename=est_poses_filename,
                  results_path=results_path, thread_name=thread_name, _live_frames=frames,
                  _keyframe_thresholds=(0.05, 0.50, np.deg2rad(5.0), np.deg2rad(60.0)), frame_window=frame_window,
                  detection_method=detection_method, cross_check=cross_check, gated_matching=gated_matching,
                  gated_max_distance=gated_max_distance, ratio_test=ratio_test, ratio=ratio,
                  subpix_refine=subpix_refine, subpix_half=subpix_half, f2f_tracker=f2f_tracker,
                   lk=lk, stereo_refine=stereo_refine, stereo_lk=stereo_lk, cyclic_columns=cyclic_columns)


def _est_poses_filename(timestamped):
    """The pose file's name: plain next to a worker thread's run, with the time of the call otherwise (:1700-1706)."""
    if not timestamped:
        return "estimated_frame_poses_TUM.txt"
    from datetime import datetime
    now = datetime.now()
    return "estimated_frame_poses_TUM-%d-%d-%d-%d-%d-%d.txt" % (now.year, now.month, now.day, now.hour, now.minute, now.second)


def _on_worker_thread(fn, **kwargs):
    """fn(**kwargs) on a thread of its own (one libsosvo context per host thread, INTEGRATION.md section 6: the worker creates
    its own) -> its result; what it raises is raised here."""
    result, failure = [], []

    def work():
        try:
            result.append(fn(**kwargs))
        except BaseException as e:  # noqa: B902 -- handed to the calling thread
            failure.append(e)
    th = threading.Thread(target=work)
    th.start()
    th.join()
    if failure:
        raise failure[0]
    return result[0]


def _scene_ground_truth_and_indices(scene_path, num_scene_images, first_image_index, last_image_index, step_for_scene_images):
    """-> (gt_TUM.txt of the scene, None for a scene taken with a static rig; the frame index list) (:1708-1722)."""
    low = scene_path.lower()
    rig_is_static = "static" in low or "GCT" in scene_path.upper() or "CCNY" in scene_path.upper() or "park" in low \
        or "grand" in low
    last = min(last_image_index, num_scene_images) if last_image_index > 0 else num_scene_images
    return (None if rig_is_static else os.path.join(scene_path, "gt_TUM.txt")), list(range(first_image_index, last, step_for_scene_images))


def driver_VO_live(camera_model, scene_path_vo_results, cam_working_thread, visualize_VO=False, use_multithreads_for_VO=True,
                   thread_name="LIVE", frame_window=None, detection_method=None, cross_check=None,
                   gated_matching=None, gated_max_distance=None, ratio_test=None, ratio=None,
                   subpix_refine=None, subpix_half=None, f2f_tracker=None, lk=None, stereo_refine=None, stereo_lk=None, cyclic_columns=None):
    """pose_est_tools.py:1743-1797: start the camera thread, run run_VO_live (on a worker thread or inline), then stop
    and join the camera thread."""
    if visualize_VO:
        raise NotImplementedError("3-D visualisation is not built: visualize_VO must be False")
    options = dict(detection_method=detection_method, cross_check=cross_check, gated_matching=gated_matching,
                   gated_max_distance=gated_max_distance, ratio_test=ratio_test, ratio=ratio,
                   subpix_refine=subpix_refine, subpix_half=subpix_half, f2f_tracker=f2f_tracker,
                   lk=lk, stereo_refine=stereo_refine, stereo_lk=stereo_lk, cyclic_columns=cyclic_columns)
    est_poses_filename = _est_poses_filename(timestamped=not use_multithreads_for_VO)
    cam_working_thread.start()
    if not getattr(cam_working_thread, "lockstep", False):
        while cam_working_thread.current_frame is None and cam_working_thread.is_alive() and not cam_working_thread.quit_flag:
            time.sleep(0.001)   # (the reference starts tracking at once and stops if no frame has arrived yet)
    kwargs = dict(visualizer_3D_VO=None, camera_model=camera_model, cam_working_thread=cam_working_thread,
                  est_poses_filename=est_poses_filename, results_path=scene_path_vo_results, thread_name=thread_name,
                  frame_window=frame_window, **options)
    try:
        result = _on_worker_thread(run_VO_live, **kwargs) if use_multithreads_for_VO else run_VO_live(**kwargs)
    finally:
        cam_working_thread.quit_flag = True   # :1792-1793
        cam_working_thread.join()
    print("DONE")
    return result


def driver_VO(camera_model, scene_path, scene_path_vo_results, scene_img_filename_template, depth_filename_template,
              num_scene_images, visualize_VO=False, use_multithreads_for_VO=True, step_for_scene_images=1, first_image_index=0,
              last_image_index=-1, thread_name="", frame_window=None, detection_method=None, cross_check=None,
              gated_matching=None, gated_max_distance=None, ratio_test=None, ratio=None,
              subpix_refine=None, subpix_half=None, f2f_tracker=None, lk=None, stereo_refine=None, stereo_lk=None, cyclic_columns=None):
    """pose_est_tools.py:1680-1741: frame index list, ground truth file discovery (gt_TUM.txt unless the scene is a
    static one), run_VO on a worker thread (as the reference does next to its GUI loop) or inline."""
    if visualize_VO:
        raise NotImplementedError("3-D visualisation is not built: visualize_VO must be False")
    options = dict(detection_method=detection_method, cross_check=cross_check, gated_matching=gated_matching,
                   gated_max_distance=gated_max_distance, ratio_test=ratio_test, ratio=ratio,
                   subpix_refine=subpix_refine, subpix_half=subpix_half, f2f_tracker=f2f_tracker,
                   lk=lk, stereo_refine=stereo_refine, stereo_lk=stereo_lk, cyclic_columns=cyclic_columns)
    gt_poses_filename, vo_frame_indices = _scene_ground_truth_and_indices(scene_path, num_scene_images, first_image_index,
                                                                          last_image_index, step_for_scene_images)
    kwargs = dict(visualizer_3D_VO=None, camera_model=camera_model, gt_poses_filename=gt_poses_filename,
                  est_poses_filename=_est_poses_filename(timestamped=not use_multithreads_for_VO),
                  img_filename_template=scene_img_filename_template, depth_filename_template=depth_filename_template,
                  img_indices=vo_frame_indices, results_path=scene_path_vo_results, thread_name=thread_name,
                  frame_window=frame_window, **options)
    result = _on_worker_thread(run_VO, **kwargs) if use_multithreads_for_VO else run_VO(**kwargs)
    print("%s Done with VO for %s!" % (thread_name, scene_path))
    return result


def _lane_limit(n_sequences, lanes, window):
    """Lanes that run concurrently: `lanes` (None: one per sequence), at most one per sequence, and few enough for the
    shape limits of the sequence entry points (include/sosvo.h: lanes * window <= 8192 slot pairs per tracking call,
    lanes * (2 window + 1) <= 65535 slots)."""
    S = int(n_sequences) if lanes is None else int(lanes)
    if S < 1:
        raise ValueError("lanes: at least one")
    return max(1, min(S, int(n_sequences), 8192 // int(window), 65535 // (2 * int(window) + 1)))


def run_VO_many(camera_model, sequences, frame_window=32, detection_method=None, lanes=None, shard=None,
                _keyframe_thresholds=None, cross_check=None, gated_matching=None, gated_max_distance=None, ratio_test=None,
                ratio=None, subpix_refine=None, subpix_half=None, f2f_tracker=None, lk=None, stereo_refine=None, stereo_lk=None, cyclic_columns=None):
    """run_VO on SEVERAL sequences of one camera model at once: the sequences advance together as the lanes of one
    pipeline.MultiSequenceEngine / RGBDMultiSequenceEngine (one frame store, one stream; per round ONE front-end launch
    over the windows of all live lanes, one tracking launch per speculative guess, and the serial tracking calls the lanes
    need at that moment as ONE batched call).  Tracking one sequence is a serial chain that cannot fill the GPU; several
    sequences are where the parallelism of real VO comes from.

    sequences: a list of dicts of run_VO's per-sequence arguments (img_filename_template, depth_filename_template,
    gt_poses_filename, img_indices, results_path, thread_name, est_poses_filename; or _live_frames, run_VO's in-memory
    source, as scripts/bench_sequences.py uses it); every sequence gets the four result files run_VO writes, in its own
    results_path.  estimated_frame_poses_TUM.txt, gt_associated_frame_poses_TUM.txt and
    keyframe_ids.txt are those of run_VO(frame_window=...) on that sequence alone, byte for byte: a frame record is a
    function of its image and a tracking record of (reference record, current record, seed), so the launch that computes a
    record does not change it.  The "Avg Time" lines of printed_messages.log are NOT comparable between a lane and a solo
    run: they come from process_time(), which counts the CPU time of every lane's thread.
    frame_window: as run_VO's, at least 1 (the per-frame mirror path and live sources have no lanes).
    lanes: how many sequences run concurrently (None: all, capped by the shape limits of the entry points); further
    sequences take a lane as one frees up.
    shard=(rank, world_size): this call processes parallel.shard_range(len(sequences), rank, world_size) only -- sequences
    are independent, so ranks need no collective; a rank with an empty share returns [].
    All sequences share the camera model: one rig, one frame size, one detector, one set of tracker settings; a sequence
    whose tracker or frames do not fit the engine is refused (ValueError from its lane).  Each lane runs run_VO on its own
    host thread; what the lanes would share they do not use or do not share: the sampler seed of pyopengv.set_seed is only
    read by the mirror path, the lanes' engine has a cache of its own beside the single-sequence engine's, current_omni_img
    and the device model of the camera model are only touched under the lock (_CAMERA_MODEL_LOCK) that also covers every
    lane's tracker construction -- which regenerates the panoramas' azimuthal masks in place --, the staging pool of
    pipeline.py is created under a lock.
    -> the list of run_VO's dicts in input order (of this rank's share), each "sequence_mode" entry extended by lane,
    lanes and the engine's launch counters (pipeline._MultiSequenceBase.reset_counters).  An exception of a lane (a reader
    that fails, a sequence that does not fit) is raised after every other lane has finished and written its files."""
    from ..parallel import shard_range
    sequences = list(sequences)
    if shard is not None:
        lo, hi = shard_range(len(sequences), int(shard[0]), int(shard[1]))
        sequences = sequences[lo:hi]
    if not sequences:
        return []
    W = int(frame_window)
    if W < 1:
        raise ValueError("run_VO_many: frame_window >= 1 (the per-frame mirror path has no lanes)")
    allowed = {"img_filename_template", "depth_filename_template", "gt_poses_filename", "img_indices", "results_path",
               "thread_name", "est_poses_filename", "_live_frames"}
    for q in sequences:
        if not isinstance(q, dict) or not set(q) <= allowed or ("img_filename_template" not in q and "_live_frames" not in q):
            raise ValueError("run_VO_many: a sequence is a dict of %s" % ", ".join(sorted(allowed)))
    rgbd = _is_rgbd_model(camera_model)
    if any((q.get("depth_filename_template") is not None) != rgbd for q in sequences if "_live_frames" not in q):
        raise ValueError("run_VO_many: %s" % ("an RGB-D camera model needs a depth_filename_template for every sequence" if rgbd
                                              else "an omnistereo camera model takes no depth maps: SOS and RGB-D "
                                                   "sequences do not mix"))
    S = _lane_limit(len(sequences), lanes, W)
    options = dict(detection_method=detection_method, cross_check=cross_check, gated_matching=gated_matching,
                   gated_max_distance=gated_max_distance, ratio_test=ratio_test, ratio=ratio,
                   subpix_refine=subpix_refine, subpix_half=subpix_half, f2f_tracker=f2f_tracker,
                   lk=lk, stereo_refine=stereo_refine, stereo_lk=stereo_lk, cyclic_columns=cyclic_columns)
    shared = dict(engine=None, key=None)
    guard, exited = threading.Lock(), set()

    def engine_for_lane(s):
        def engine_for(tracker, cm, first_image, window):
            # (the first lane to arrive builds the engine, current_omni_img and the device model with it, from masks no
            # other lane's tracker is regenerating at that moment)
            with _CAMERA_MODEL_LOCK, guard:
                shape = tuple(np.asarray(first_image).shape[:2])
                if shared["engine"] is None:
                    shared["engine"], shared["key"] = multi_sequence_engine_for(tracker, cm, first_image, window, S)
                    shared["shape"] = shape
                    if shared["engine"] is None:
                        shared["engine"] = False
                    else:   # every lane that still has work counts as live from the first round on: the rounds wait for
                        for other in range(S):          # the lanes that are still reading their first frame
                            if other not in exited:
                                shared["engine"].begin(other)
                if shared["engine"] is False:
                    raise ValueError("run_VO_many: this tracker configuration has no batched engine")
                settings = _engine_settings(tracker, cm, first_image)
                if settings is None or settings[2] != shared["key"] or shape != shared["shape"]:
                    raise ValueError("run_VO_many: the sequence does not fit the lanes' engine (another frame size, rig or "
                                     "tracker configuration)")
            return shared["engine"].begin(s)
        return engine_for
    todo = list(enumerate(sequences))[::-1]
    results, failures = [None] * len(sequences), [None] * len(sequences)

    def work(s):
        while True:
            with guard:
                job = todo.pop() if todo else None
                if job is None:
                    exited.add(s)
            if job is None:
                if shared["engine"]:
                    shared["engine"].end(s)     # (a lane counted as live before it had anything to run)
                return
            i, q = job
            try:
                out = run_VO(None, camera_model, frame_window=W, _keyframe_thresholds=_keyframe_thresholds,
                             _engine_for=engine_for_lane(s), **options, **q)
                if "sequence_mode" in out:
                    out["sequence_mode"].update(lane=s, lanes=S)
                results[i] = out
            except BaseException as e:  # noqa: B902 -- raised by the calling thread, after the other lanes
                failures[i] = e
            finally:
                eng = shared["engine"]
                if eng:
                    try:
                        eng.end(s)
                    except BaseException as e:  # noqa: B902 -- (a device call of the round this lane's end set off)
                        if failures[i] is None:
                            failures[i] = e
    threads = [threading.Thread(target=work, args=(s,), name="sosvo-lane-%d" % s) for s in range(S)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    if shared["engine"]:
        counters = dict(shared["engine"].counters)
        for out in results:
            if out is not None and "sequence_mode" in out:
                out["sequence_mode"].update(counters)
    for e in failures:
        if e is not None:
            raise e
    return results


def driver_VO_many(camera_model, scenes, visualize_VO=False, step_for_scene_images=1, first_image_index=0, last_image_index=-1,
                   frame_window=None, detection_method=None, lanes=None, shard=None, cross_check=None, gated_matching=None,
                   gated_max_distance=None, ratio_test=None, ratio=None,
                   subpix_refine=None, subpix_half=None, f2f_tracker=None, lk=None, stereo_refine=None, stereo_lk=None, cyclic_columns=None):
    """driver_VO for several scenes of one camera model through run_VO_many.  scenes: a list of dicts(scene_path,
    scene_path_vo_results, scene_img_filename_template, depth_filename_template, num_scene_images, thread_name); the frame
    index list and the ground-truth file of each scene are found as driver_VO finds them.  -> run_VO_many's list."""
    if visualize_VO:
        raise NotImplementedError("3-D visualisation is not built: visualize_VO must be False")
    options = dict(detection_method=detection_method, cross_check=cross_check, gated_matching=gated_matching,
                   gated_max_distance=gated_max_distance, ratio_test=ratio_test, ratio=ratio,
                   subpix_refine=subpix_refine, subpix_half=subpix_half, f2f_tracker=f2f_tracker,
                   lk=lk, stereo_refine=stereo_refine, stereo_lk=stereo_lk, cyclic_columns=cyclic_columns)
    sequences = []
    for sc in scenes:
        gt_poses_filename, indices = _scene_ground_truth_and_indices(sc["scene_path"], int(sc["num_scene_images"]), first_image_index,
                                                                     last_image_index, step_for_scene_images)
        sequences.append(dict(gt_poses_filename=gt_poses_filename, est_poses_filename=_est_poses_filename(timestamped=False),
                              img_filename_template=sc["scene_img_filename_template"],
                              depth_filename_template=sc.get("depth_filename_template"), img_indices=indices,
                              results_path=sc["scene_path_vo_results"], thread_name=sc.get("thread_name", "")))
    results = run_VO_many(camera_model, sequences, frame_window=32 if frame_window is None else frame_window, lanes=lanes,
                          shard=shard, **options)
    print("Done with VO for %d sequences!" % len(results))
    return results
