"""ctypes binding of libsosvo.so (the C ABI declared in include/sosvo.h).

The product path has no CPU fallback: if the HIP library is missing or a symbol is
absent this module raises, it never routes anywhere else.
"""
import ctypes
import os
import re
from collections import namedtuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsosvo.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sosvo.h")

c_i32 = ctypes.c_int32
c_f64 = ctypes.c_double
c_f32 = ctypes.c_float
c_u64 = ctypes.c_uint64
c_p = ctypes.c_void_p

SOSVO_OK = 0
STATUS_NAMES = {0: "SOSVO_OK", -1: "SOSVO_ERR_ARG", -2: "SOSVO_ERR_HIP", -3: "SOSVO_ERR_NODEVICE",
                -4: "SOSVO_ERR_CAPACITY"}

KEY_SHIFT = 20
KEY_IDX_MASK = 0xFFFFF
KEY_NONE = 0xFFFFFFFF
DESC_BYTES = 32


class SosvoError(RuntimeError):
    pass


# name -> (restype, argtypes); must list every function of include/sosvo.h (tested).
SIGNATURES = {
    "sosvo_abi_version": (c_i32, []),
    "sosvo_orb_bit_pattern_31": (c_i32, [c_p]),
    "sosvo_create": (c_i32, [ctypes.POINTER(c_p), c_i32, c_p]),
    "sosvo_destroy": (c_i32, [c_p]),
    "sosvo_set_stream": (c_i32, [c_p, c_p]),
    "sosvo_set_hint": (c_i32, [c_p, c_i32, c_i32]),
    "sosvo_set_lk_options": (c_i32, [c_p, c_p]),
    "sosvo_set_stereo_lk_options": (c_i32, [c_p, c_p]),
    "sosvo_synchronize": (c_i32, [c_p]),
    "sosvo_last_error": (ctypes.c_char_p, [c_p]),
    "sosvo_timer_start": (c_i32, [c_p]),
    "sosvo_timer_stop": (c_i32, [c_p]),
    "sosvo_timer_elapsed_ms": (c_i32, [c_p, ctypes.POINTER(c_f32)]),
    "sosvo_profile_enable": (c_i32, [c_p, c_i32]),
    "sosvo_profile_count": (c_i32, [c_p]),
    "sosvo_debug_fill_scratch": (c_i32, [c_p, c_i32]),
    "sosvo_profile_get": (c_i32, [c_p, c_i32, ctypes.c_char_p, c_i32, ctypes.POINTER(c_f32)]),
    "sosvo_unwrap": (c_i32, [c_p, c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p]),
    "sosvo_unwrap_prepare": (c_i32, [c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p]),
    "sosvo_unwrap_prepare_seam_free": (c_i32, [c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p]),
    "sosvo_mask_bits_seam_free": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_p]),
    "sosvo_keypoints_unpad": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_i32]),
    "sosvo_gray_unpad": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_p, c_p]),
    "sosvo_unwrap_table": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p]),
    "sosvo_median_gray": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p]),
    "sosvo_unwrap_median_gray": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_p]),
    "sosvo_unwrap_median_gray_rows": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p]),
    "sosvo_gray_rows_needed": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_f32, c_f32, c_p]),
    "sosvo_detect_gft": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_f64, c_f64, c_i32, c_i32, c_p,
                                 c_p, c_p]),
    "sosvo_detect_gft_candidates": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, ctypes.POINTER(c_i32), c_p, c_p,
                                            c_p]),
    "sosvo_gauss7": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, ctypes.c_int64, c_p, ctypes.c_int64, c_p]),
    "sosvo_describe_orb": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_f32, c_f32, c_p, c_i32,
                                   c_p]),
    "sosvo_describe_orb_rows": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_f32, c_f32, c_p, c_i32,
                                        c_p, c_p]),
    "sosvo_subpix_weights": (c_i32, [c_p, c_i32, c_p]),
    "sosvo_refine_subpix": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_i32, c_i32, c_f64, c_p]),
    "sosvo_gray_pyramid_bytes": (c_i32, [c_p, c_i32, c_i32, c_i32, c_i32, ctypes.POINTER(ctypes.c_int64)]),
    "sosvo_gray_pyramid": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p, c_p]),
    "sosvo_gray_pyramid_cyclic": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p, c_p]),
    "sosvo_track_lk": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_p, c_i32, c_i32, c_p, c_p, c_i32, c_i32,
                               c_f64, c_f64, c_i32, c_p, c_p, c_p, c_p, c_f64]),
    "sosvo_refine_stereo_lk": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_p, c_i32, c_i32, c_p, c_p, c_p, c_p, c_p, c_f64, c_f64,
                                       c_p, c_p]),
    "sosvo_orb_pyramid_pixels": (ctypes.c_int64, [c_i32, c_i32]),
    "sosvo_orb_mask_pyramid": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p]),
    "sosvo_detect_orb": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_p]),
    "sosvo_describe_orb_levels": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_p, c_p, c_p]),
    "sosvo_detect_describe_orb": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_p, c_p,
                                          c_p, c_p]),
    "sosvo_detect_fast": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_p]),
    "sosvo_detect_agast": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_p]),
    "sosvo_match_hamming": (c_i32, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p]),
    "sosvo_match_hamming_gated": (c_i32, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_f64, c_f64,
                                          c_i32, c_p]),
    "sosvo_match_hamming_gated_cyclic": (c_i32, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_f64,
                                                 c_f64, c_i32, c_p]),
    "sosvo_match_hamming_ratio": (c_i32, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_f64, c_f64,
                                          c_i32, c_i32, c_p, c_p]),
    "sosvo_match_radius": (c_i32, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p]),
    "sosvo_cross_check_matches": (c_i32, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_p, c_p]),
    "sosvo_sort_matches": (c_i32, [c_p, c_p, c_p, c_p, c_i32, c_i32, c_p]),
    "sosvo_pano_to_bearing": (c_i32, [c_p, c_p, c_i32, c_f64, c_f64, c_f64, c_f64, c_p, c_p, c_p]),
    "sosvo_triangulate_midpoint": (c_i32, [c_p, c_p, c_p, c_p, c_p, c_i32, c_p, c_p, c_p]),
    "sosvo_triangulate2": (c_i32, [c_p, c_p, c_p, c_i32, c_p, c_p, c_p]),
    "sosvo_range_filter": (c_i32, [c_p, c_p, c_i32, c_f64, c_f64, c_p]),
    "sosvo_rgbd_backproject": (c_i32, [c_p, c_p, c_i32, c_i32, c_p, c_p, c_i32, c_f64, c_f64, c_f64, c_f64, c_f64,
                                       c_i32, c_p, c_p]),
    "sosvo_stereo_assemble": (c_i32, [c_p] + [c_p] * 9 + [c_i32] * 4 + [c_p] * 9),
    "sosvo_f2f_assemble": (c_i32, [c_p] + [c_p] * 7 + [c_i32] + [c_p] * 6 + [c_i32, c_i32] + [c_p] * 7),
    "sosvo_f2f_assemble_tracked": (c_i32, [c_p] + [c_p] * 5 + [c_i32] + [c_p] * 5 + [c_i32, c_i32] + [c_p] * 7),
    "sosvo_f2f_assemble_cyclic": (c_i32, [c_p] + [c_p] * 7 + [c_i32] + [c_p] * 6 + [c_i32, c_i32] + [c_p] * 7),
    "sosvo_f2f_assemble_tracked_cyclic": (c_i32, [c_p] + [c_p] * 5 + [c_i32] + [c_p] * 5 + [c_i32, c_i32] + [c_p] * 7),
    "sosvo_ransac_abs_pose": (c_i32, [c_p, c_p, c_p, c_p, c_p, c_p, c_i32, c_i32, c_p, c_i32, c_i32, c_f64,
                                      c_i32, c_i32, c_u64, c_p, c_p, c_p, c_p, c_p, c_p]),
    "sosvo_ransac_abs_pose_seeds": (c_i32, [c_p, c_p, c_p, c_p, c_p, c_p, c_i32, c_i32, c_p, c_i32, c_i32, c_f64,
                                            c_i32, c_i32, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "sosvo_match_l2": (c_i32, [c_p, c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p]),
    "sosvo_ransac_rel_pose": (c_i32, [c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_f64, c_i32, c_i32, c_u64, c_p, c_p, c_p, c_p,
                                      c_p, c_p]),
    "sosvo_refine_abs_pose": (c_i32, [c_p, c_p, c_p, c_p, c_p, c_p, c_i32, c_p, c_i32, c_i32, c_p, c_p, c_i32,
                                      c_p, c_p, c_p]),
    "sosvo_rgbd_assemble": (c_i32, [c_p, c_p, c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_p, c_p, c_p]),
    "sosvo_f2f_assemble_central": (c_i32, [c_p, c_f64, c_f64, c_p, c_p, c_p, c_p, c_i32, c_p, c_p, c_p, c_p, c_i32, c_i32,
                                           c_p, c_p, c_p, c_p, c_p]),
    "sosvo_frame_pair_batch_workspace": (ctypes.c_size_t, [c_p]),
    "sosvo_frame_pair_batch": (c_i32, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.c_size_t, c_p]),
    "sosvo_frame_pair_batch_streams_workspace": (ctypes.c_size_t, [c_p, c_i32]),
    "sosvo_frame_pair_batch_streams": (c_i32, [c_p, c_p, c_p, c_i32, c_p, c_p, c_p, c_p, c_p, ctypes.c_size_t, c_p]),
    "sosvo_frame_pair_batch_streams_enqueue": (c_i32, [c_p, c_p, c_p, c_i32, c_p, c_p, c_p, c_p, c_p, ctypes.c_size_t, c_p]),
    "sosvo_frame_pair_batch_streams_join": (c_i32, [c_p]),
    "sosvo_sequence_workspace": (ctypes.c_size_t, [c_p, c_i32, c_i32]),
    "sosvo_sequence_front_end": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_p, c_i32, c_i32, c_p, c_p, c_p, c_p, ctypes.c_size_t]),
    "sosvo_sequence_track": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_p, c_p, c_i32, c_u64, c_p, ctypes.c_size_t, c_p]),
    "sosvo_sequence_copy_slot": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p, ctypes.c_size_t]),
    "sosvo_sequence_frame_counts": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p, ctypes.c_size_t, c_p]),
    "sosvo_sequence_front_end_slots": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_p, c_i32, c_p, c_p, c_p, c_p, c_p, ctypes.c_size_t]),
    "sosvo_sequence_track_seeds": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_p, c_p, c_p, c_i32, c_p, ctypes.c_size_t, c_p]),
    "sosvo_sequence_copy_slots": (c_i32, [c_p, c_p, c_i32, c_i32, c_p, c_p, c_i32, c_p, ctypes.c_size_t]),
    "sosvo_rgbd_sequence_workspace": (ctypes.c_size_t, [c_p, c_i32, c_i32]),
    "sosvo_rgbd_sequence_front_end": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_p, c_p, c_i32, c_i32, c_p, c_p, c_p, ctypes.c_size_t]),
    "sosvo_rgbd_sequence_track": (c_i32, [c_p, c_p, c_i32, c_i32, c_p, c_p, c_i32, c_u64, c_p, ctypes.c_size_t, c_p]),
    "sosvo_rgbd_sequence_copy_slot": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p, ctypes.c_size_t]),
    "sosvo_rgbd_sequence_frame_counts": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p, ctypes.c_size_t, c_p]),
    "sosvo_rgbd_sequence_front_end_slots": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_p, c_p, c_i32, c_p, c_p, c_p, c_p,
                                                    ctypes.c_size_t]),
    "sosvo_rgbd_sequence_track_seeds": (c_i32, [c_p, c_p, c_i32, c_i32, c_p, c_p, c_p, c_i32, c_p, ctypes.c_size_t, c_p]),
    "sosvo_rgbd_sequence_copy_slots": (c_i32, [c_p, c_p, c_i32, c_i32, c_p, c_p, c_i32, c_p, ctypes.c_size_t]),
    "sosvo_rgbd_pair_batch_workspace": (ctypes.c_size_t, [c_p]),
    "sosvo_rgbd_pair_batch": (c_i32, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.c_size_t, c_p]),
    "sosvo_census_9x7": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p]),
    "sosvo_dense_stereo": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_i32, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p]),
    "sosvo_dense_stereo_paths": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_i32, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_p,
                                         c_p]),
    "sosvo_dense_triangulate": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p]),
    "sosvo_dense_speckle": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p]),
}

HINT_SHARED_DEVICE = 1
HINT_SCORE_FP64_ONLY = 2
HINT_MATCH_UNSPLIT = 3
HINT_ROLLING_NARROW = 4
FLAG_CAM_ROT_IDENTITY = 1
FLAG_EPNP = 2
FLAG_GP3P = 4
FLAG_TWOPT = 8
FLAG_CROSS_CHECK_STEREO = 0x1000   # mutual matches only: static stereo (sosvo_batch_cfg.ransac_flags)
FLAG_CROSS_CHECK_F2F = 0x2000      # ... frame to frame (sosvo_batch_cfg.ransac_flags, sosvo_rgbd_batch_cfg.flags)
FLAG_GATED_STEREO = 0x4000         # search under the pixel gates: static stereo (sosvo_batch_cfg.ransac_flags)
FLAG_GATED_F2F = 0x8000            # ... frame to frame (sosvo_batch_cfg.ransac_flags, sosvo_rgbd_batch_cfg.flags)
GATED_MAX_DIST_SHIFT = 16          # SOSVO_GATED_MAX_DIST(d): bits 16-24, 0 = no cap
GATED_MAX_DIST_MASK = 0x1FF << GATED_MAX_DIST_SHIFT
FLAG_RATIO_STEREO = 0x10           # the ratio rule: static stereo (sosvo_batch_cfg.ransac_flags)
FLAG_RATIO_F2F = 0x20              # ... frame to frame (sosvo_batch_cfg.ransac_flags, sosvo_rgbd_batch_cfg.flags)
RATIO_64THS_SHIFT = 25             # SOSVO_RATIO_64THS(r): bits 25-30, the ratio in 64ths, 1 .. 63
RATIO_64THS_MASK = 0x3F << RATIO_64THS_SHIFT
FLAG_SUBPIX = 0x40                 # sub-pixel keypoint refinement before the static stereo (sosvo_batch_cfg.ransac_flags)
SUBPIX_HALF_SHIFT = 10             # SOSVO_SUBPIX_HALF(h): bits 10-11, the window half-size 2 .. 5 stored as h - 2
SUBPIX_HALF_MASK = 3 << SUBPIX_HALF_SHIFT
SUBPIX_MAX_ITER = 10               # what the one-call and sequence entry points run the stage with
SUBPIX_EPS = 0.01
FLAG_LK_F2F = 0x80                 # Lucas-Kanade tracking in place of the frame-to-frame matcher (sosvo_batch_cfg.ransac_flags)
FLAG_LK_STEREO = 0x100             # sub-pixel static stereo: sosvo_refine_stereo_lk in the front end (sosvo_batch_cfg.ransac_flags)
FLAG_CYCLIC_F2F = 0x200            # cyclic panorama columns frame to frame (sosvo_batch_cfg.ransac_flags only: DESIGN.md section 34)
FLAG_SEAM_FREE = -0x80000000       # the seam-free front end: the int32 sign bit, the word's last free one
SEAM_HALO = 40                     # SOSVO_SEAM_HALO: the cyclic columns a seam-free front end pads on either side
SEAM_REACH = 35                    # columns a stage may read around a keypoint of the original columns
SEAM_FREE = "seam_free"            # the third value of cyclic_columns: True plus the seam-free front end
LK_INITIAL_FLOW = 1                # SOSVO_LK_INITIAL_FLOW: next_pts holds the starting guess on entry
LK_CYCLIC_COLUMNS = 4              # SOSVO_LK_CYCLIC_COLUMNS: the columns are one period (a panorama is a full circle)
LK_MAX_HALF, LK_MAX_LEVELS, LK_MAX_ITER, LK_MAX_CAP = 10, 4, 30, 4096
DETECTOR_GFT = 0
DETECTOR_ORB = 1
DETECTOR_FAST = 2
DETECTOR_AGAST = 3
DETECTORS = {"GFT": DETECTOR_GFT, "ORB": DETECTOR_ORB, "FAST": DETECTOR_FAST, "AGAST": DETECTOR_AGAST}
RGBD_DETECTOR_SHIFT = 8
RGBD_DETECTOR_MASK = 3 << RGBD_DETECTOR_SHIFT
REL_FIVEPT = 5
REL_SEVENPT = 7
REL_EIGHTPT = 8


class Rig(ctypes.Structure):
    """Mirror of `struct sosvo_rig` (include/sosvo.h)."""
    _fields_ = [("pano_top", c_f64 * 4), ("pano_bot", c_f64 * 4), ("F_top", c_f64 * 3), ("F_bot", c_f64 * 3),
                ("min_range", c_f64), ("max_range", c_f64), ("stereo_min_disp", c_f64),
                ("stereo_max_hdiff", c_f64), ("f2f_max_hdiff", c_f64), ("pct_good_matches", c_f64)]



class RgbdCam(ctypes.Structure):
    """Mirror of `struct sosvo_rgbd_cam` (include/sosvo.h)."""
    _fields_ = [("fx", c_f64), ("fy", c_f64), ("cx", c_f64), ("cy", c_f64), ("focal_length_m", c_f64),
                ("depth_is_Z", c_i32), ("reserved", c_i32), ("min_range", c_f64), ("max_range", c_f64)]


class BatchCfg(ctypes.Structure):
    """Mirror of `struct sosvo_batch_cfg` (include/sosvo.h)."""
    _fields_ = [("n_pairs", c_i32), ("H", c_i32), ("W", c_i32), ("rows", c_i32), ("cols", c_i32), ("nmask", c_i32),
                ("kp_cap", c_i32), ("frame_cap", c_i32), ("median_ksize", c_i32), ("max_corners", c_i32), ("edge", c_i32),
                ("ransac_max_iter", c_i32), ("ransac_adaptive", c_i32), ("lm_max_iter", c_i32), ("quality", c_f64),
                ("min_distance", c_f64), ("ransac_threshold", c_f64), ("seed", c_u64), ("cos_a", c_f32), ("sin_a", c_f32),
                ("ransac_flags", c_i32), ("detector", c_i32)]


class RgbdBatchCfg(ctypes.Structure):
    """Mirror of `struct sosvo_rgbd_batch_cfg` (include/sosvo.h)."""
    _fields_ = [("n_pairs", c_i32), ("rows", c_i32), ("cols", c_i32), ("kp_cap", c_i32), ("frame_cap", c_i32),
                ("median_ksize", c_i32), ("max_corners", c_i32), ("edge", c_i32), ("ransac_max_iter", c_i32),
                ("ransac_adaptive", c_i32), ("lm_max_iter", c_i32), ("flags", c_i32), ("quality", c_f64),
                ("min_distance", c_f64), ("ransac_threshold", c_f64), ("pct_good_matches", c_f64), ("f2f_max_hdiff", c_f64),
                ("seed", c_u64), ("cos_a", c_f32), ("sin_a", c_f32)]


def detector_code(method):
    """feature_detection_method ("GFT", "ORB", "FAST", "AGAST", any case) -> enum sosvo_detector; others raise."""
    name = str(method).upper()
    if name not in DETECTORS:
        raise NotImplementedError("detection method %r: the batched paths run %s" % (method, ", ".join(DETECTORS)))
    return DETECTORS[name]


def rgbd_detector_flags(method):
    """SOSVO_RGBD_DETECTOR(d): the detector's bits of sosvo_rgbd_batch_cfg.flags."""
    return detector_code(method) << RGBD_DETECTOR_SHIFT


def cross_check_flags(stereo=False, f2f=False):
    """The SOSVO_FLAG_CROSS_CHECK_* bits of a batch configuration for the two matchers' switches."""
    return (FLAG_CROSS_CHECK_STEREO if stereo else 0) | (FLAG_CROSS_CHECK_F2F if f2f else 0)


def gated_flags(stereo=False, f2f=False, max_distance=None):
    """The SOSVO_FLAG_GATED_* bits and the SOSVO_GATED_MAX_DIST field of a batch configuration.  max_distance: None = no
    cap (the field's 0), or 1 .. 256.  The cap belongs to the gated search: without a switch it is not encoded."""
    if max_distance is not None and (int(max_distance) != max_distance or not 1 <= max_distance <= 256):
        raise ValueError("gated_max_distance must be None or an integer in 1 .. 256, got %r" % (max_distance,))
    flags = (FLAG_GATED_STEREO if stereo else 0) | (FLAG_GATED_F2F if f2f else 0)
    if flags and max_distance is not None:
        flags |= int(max_distance) << GATED_MAX_DIST_SHIFT
    return flags


def ratio_64ths(ratio):
    """A Python ratio -> SOSVO_RATIO_64THS's r: a float in (0, 1) with ratio * 64 an integer (0.75 -> 48).  Nothing is
    rounded: the device rule is the integer rule 64 * d1 < r * d2, and a ratio it cannot represent is refused."""
    try:
        x = float(ratio) * 64.0
    except (TypeError, ValueError):
        raise ValueError("ratio must be a float in (0, 1) with ratio * 64 an integer, got %r" % (ratio,))
    if not (x == x and 1.0 <= x <= 63.0 and x == int(x)):
        if x != x:
            raise ValueError("ratio must be a float in (0, 1) with ratio * 64 an integer, got %r" % (ratio,))
        lo, hi = sorted(sorted(range(1, 64), key=lambda c: abs(c - x))[:2])
        raise ValueError("ratio must be a float in (0, 1) with ratio * 64 an integer, got %r; the nearest admissible values "
                         "are %r (%d/64) and %r (%d/64)" % (ratio, lo / 64.0, lo, hi / 64.0, hi))
    return int(x)


def ratio_flags(stereo=False, f2f=False, ratio=None):
    """The SOSVO_FLAG_RATIO_* bits and the SOSVO_RATIO_64THS field of a batch configuration.  ratio: see ratio_64ths; a
    switch needs one.  The ratio belongs to the rule: without a switch it is checked but not encoded."""
    r = None if ratio is None else ratio_64ths(ratio)
    flags = (FLAG_RATIO_STEREO if stereo else 0) | (FLAG_RATIO_F2F if f2f else 0)
    if flags and r is None:
        raise ValueError("the ratio test needs a ratio (a float in (0, 1) with ratio * 64 an integer, e.g. 0.75)")
    if flags:
        flags |= r << RATIO_64THS_SHIFT
    return flags


def subpix_half(subpix):
    """A `subpix` argument (None / False: off; True: half 5; or the window half-size 2 .. 5) -> the half-size or None."""
    if subpix is None or subpix is False:
        return None
    if subpix is True:
        return 5
    if int(subpix) != subpix or not 2 <= subpix <= 5:
        raise ValueError("subpix must be None or a window half-size in 2 .. 5, got %r" % (subpix,))
    return int(subpix)


def subpix_flags(subpix=None):
    """The SOSVO_FLAG_SUBPIX bit and the SOSVO_SUBPIX_HALF field of a batch configuration; the field belongs to the
    switch: without it nothing is encoded."""
    half = subpix_half(subpix)
    return 0 if half is None else FLAG_SUBPIX | ((half - 2) << SUBPIX_HALF_SHIFT)


def subpix_half_of(flags):
    """SOSVO_SUBPIX_HALF_OF(flags) with the switch set, else None."""
    flags = int(flags)
    return ((flags & SUBPIX_HALF_MASK) >> SUBPIX_HALF_SHIFT) + 2 if flags & FLAG_SUBPIX else None


def subpix_weights(half):
    """sosvo_subpix_weights: the library's weight table of a window half-size (host call, no GPU)."""
    w = (c_i32 * 11)()      # (the largest table: half 5)
    rc = load().sosvo_subpix_weights(None, int(half), w)
    if rc != 0:
        raise SosvoError("sosvo_subpix_weights(%r) -> %s" % (half, STATUS_NAMES.get(rc, rc)))
    return list(w)[:2 * int(half) + 1]


class _Settings(object):
    """What LKOptions and StereoLKOptions share: the range checks of their fields and of().  `arg`, `kind`: their argument and
    themselves as the messages name them."""
    __slots__ = ()

    @classmethod
    def _check(cls, integers, numbers):
        for name, v, lo, hi in integers:
            if isinstance(v, bool) or not isinstance(v, (int, float)) or int(v) != v or not lo <= v <= hi:
                raise ValueError("%s %s must be an integer in %d .. %d, got %r" % (cls.arg, name, lo, hi, v))
        for name, v in numbers:
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= v < float("inf"):
                raise ValueError("%s %s must be a finite number >= 0, got %r" % (cls.arg, name, v))

    @classmethod
    def of(cls, value):
        """An `lk` / `stereo_lk` argument (None: the defaults; a value of the class; a dict of its fields) -> the value."""
        if value is None or isinstance(value, cls):
            return cls() if value is None else value
        if not isinstance(value, dict):
            raise ValueError("%s must be None, %s or a dict of its fields, got %r" % (cls.arg, cls.kind, value))
        if set(value) - set(cls._fields):
            raise ValueError("%s: unknown settings %s" % (cls.arg, sorted(set(value) - set(cls._fields))))
        return cls(**value)


class LKOptions(_Settings, namedtuple("LKOptions", "half levels max_iter eps min_eig fb_max")):
    """The settings of the pyramidal Lucas-Kanade tracker (sosvo_track_lk) as one checked value: window half-size 2 .. 10,
    pyramid levels 1 .. 4, max_iter 1 .. 30, eps >= 0, min_eig >= 0 (OpenCV's minEigThreshold), fb_max None (no
    forward-backward check) or > 0 pixels.  Defaults: cv2.calcOpticalFlowPyrLK's (21 x 21 window, maxLevel 2 -> 3 levels,
    TermCriteria(30, 0.01), 1e-4).  A value out of range raises ValueError; nothing is rounded."""
    __slots__, arg, kind = (), "lk", "an LKOptions"

    def __new__(cls, half=10, levels=3, max_iter=30, eps=0.01, min_eig=1e-4, fb_max=None):
        cls._check((("half", half, 2, LK_MAX_HALF), ("levels", levels, 1, LK_MAX_LEVELS), ("max_iter", max_iter, 1, LK_MAX_ITER)),
                   (("eps", eps), ("min_eig", min_eig)))
        if fb_max is not None and (isinstance(fb_max, bool) or not isinstance(fb_max, (int, float))
                                   or not 0.0 < fb_max < float("inf")):
            raise ValueError("lk fb_max must be None or a finite number > 0 (pixels), got %r" % (fb_max,))
        return super().__new__(cls, int(half), int(levels), int(max_iter), float(eps), float(min_eig),
                               None if fb_max is None else float(fb_max))


class LkOptionsStruct(ctypes.Structure):
    """Mirror of `struct sosvo_lk_options` (include/sosvo.h)."""
    _fields_ = [("half", c_i32), ("levels", c_i32), ("max_iter", c_i32), ("reserved", c_i32), ("eps", c_f64), ("min_eig", c_f64),
                ("fb_max", c_f64)]

    @classmethod
    def of(cls, lk):
        """An LKOptions -> the struct of sosvo_set_lk_options (fb_max None -> 0: no forward-backward check)."""
        return cls(lk.half, lk.levels, lk.max_iter, 0, lk.eps, lk.min_eig, 0.0 if lk.fb_max is None else lk.fb_max)


class StereoLKOptions(_Settings, namedtuple("StereoLKOptions", "half max_iter eps min_eig max_shift")):
    """The settings of the static-stereo Lucas-Kanade refinement (sosvo_refine_stereo_lk) as one checked value: window
    half-size 2 .. 10, max_iter 1 .. 30, eps >= 0, min_eig >= 0, max_shift None (= half) or a finite number >= 0 (pixels; 0
    means half as well): a tracked position further than that from the matcher's partner on either axis is reverted.  A
    value out of range raises ValueError; nothing is rounded."""
    __slots__, arg, kind = (), "stereo_lk", "a StereoLKOptions"

    def __new__(cls, half=4, max_iter=30, eps=0.01, min_eig=1e-4, max_shift=None):
        cls._check((("half", half, 2, LK_MAX_HALF), ("max_iter", max_iter, 1, LK_MAX_ITER)), (("eps", eps), ("min_eig", min_eig)))
        if max_shift is not None and (isinstance(max_shift, bool) or not isinstance(max_shift, (int, float))
                                      or not 0.0 <= max_shift < float("inf")):
            raise ValueError("stereo_lk max_shift must be None or a finite number >= 0 (pixels), got %r" % (max_shift,))
        return super().__new__(cls, int(half), int(max_iter), float(eps), float(min_eig),
                               None if max_shift is None else float(max_shift))

    @property
    def bound(self):
        """The acceptance bound in pixels: max_shift, or half where it is None or 0."""
        return float(self.max_shift) if self.max_shift else float(self.half)


class StereoLkOptionsStruct(ctypes.Structure):
    """Mirror of `struct sosvo_stereo_lk_options` (include/sosvo.h)."""
    _fields_ = [("half", c_i32), ("max_iter", c_i32), ("eps", c_f64), ("min_eig", c_f64), ("max_shift", c_f64)]

    @classmethod
    def of(cls, o):
        """A StereoLKOptions -> the struct of sosvo_set_stereo_lk_options (max_shift None -> 0: half)."""
        return cls(o.half, o.max_iter, o.eps, o.min_eig, 0.0 if o.max_shift is None else o.max_shift)


def stereo_refine_options(stereo_refine, stereo_lk, rgbd=False):
    """The `stereo_refine` / `stereo_lk` arguments of the engines' constructors -> the StereoLKOptions of an engine that refines
    its static stereo by tracking ("lk"), None for one that does not (None).  Settings without the switch are refused, and so
    is the switch on an RGB-D engine: it has no static stereo."""
    if stereo_refine not in (None, "lk"):
        raise ValueError("stereo_refine: None or \"lk\", got %r" % (stereo_refine,))
    if stereo_refine is None:
        if stereo_lk is not None:
            raise ValueError("stereo_lk settings without stereo_refine=\"lk\"")
        return None
    if rgbd:
        raise ValueError("stereo_refine=\"lk\": an RGB-D camera has no static stereo")
    return StereoLKOptions.of(stereo_lk)


def f2f_tracker_options(f2f_tracker, lk, opts=None, rgbd=False):
    """The `f2f_tracker` / `lk` arguments -> the LKOptions of an engine that tracks ("lk"), None for one that matches ("match").
    Refused: settings without the tracker, the options (`opts`, a MatchOptions) of the matcher it replaces, an RGB-D engine."""
    if f2f_tracker not in ("match", "lk"):
        raise ValueError("f2f_tracker: \"match\" or \"lk\", got %r" % (f2f_tracker,))
    if f2f_tracker != "lk":
        if lk is not None:
            raise ValueError("lk settings without f2f_tracker=\"lk\"")
        return None
    if rgbd:
        raise ValueError("f2f_tracker=\"lk\": the RGB-D engines have no Lucas-Kanade tracking")
    if opts is not None and (opts.cross_check_f2f or opts.gated_f2f or opts.ratio_f2f):
        raise ValueError("f2f_tracker=\"lk\" replaces the frame-to-frame matcher: cross_check_f2f / gated_f2f / ratio_f2f "
                         "cannot be set with it")
    return LKOptions.of(lk)


def cyclic_value(cyclic_columns):
    """A `cyclic_columns` argument -> False, True or SEAM_FREE ("seam_free": True plus the seam-free front end).  Anything but
    the string is taken by its truth, as it always was."""
    if isinstance(cyclic_columns, str):
        if cyclic_columns != SEAM_FREE:
            raise ValueError("cyclic_columns: False, True or \"seam_free\", got %r" % (cyclic_columns,))
        return SEAM_FREE
    return bool(cyclic_columns)


def seam_free_check(cols, detection_method="GFT", edge=31, stereo_lk=None):
    """What SOSVO_FLAG_SEAM_FREE asks of the shape and the detector (the C layer's refusals, before the device is asked
    anything): a width of 40 .. 16304 columns, no ORB detector, edge <= 31, stereo-LK windows inside the halo's clean columns."""
    for w in cols if isinstance(cols, (tuple, list)) else (cols,):
        if not (w == int(w) and SEAM_HALO <= w and w + 2 * SEAM_HALO <= 16384):
            raise ValueError("cyclic_columns=\"seam_free\": the panorama width must be an integer in %d .. %d, got %r"
                             % (SEAM_HALO, 16384 - 2 * SEAM_HALO, w))
    if str(detection_method).upper() == "ORB":
        raise ValueError("cyclic_columns=\"seam_free\": the ORB detector's pyramid levels keep borders of their own, which the "
                         "%d-column halo covers on level 0 only" % SEAM_HALO)
    if edge > 31:
        raise ValueError("cyclic_columns=\"seam_free\" needs edge <= 31, got %r" % (edge,))
    if stereo_lk is not None and 2 + stereo_lk.half + -(-stereo_lk.bound // 1) > SEAM_REACH:
        raise ValueError("cyclic_columns=\"seam_free\" with stereo_refine=\"lk\": 2 + half + ceil(max_shift) must be <= %d, got "
                         "half %d, max_shift %r" % (SEAM_REACH, stereo_lk.half, stereo_lk.bound))


def gray_pyramid_bytes(nimg, rows, cols, levels):
    """sosvo_gray_pyramid_bytes: bytes of the levels 1 .. levels - 1 of nimg images (host call, no GPU)."""
    out = ctypes.c_int64(0)
    rc = load().sosvo_gray_pyramid_bytes(None, int(nimg), int(rows), int(cols), int(levels), ctypes.byref(out))
    if rc != 0:
        raise SosvoError("sosvo_gray_pyramid_bytes(%r, %r, %r, %r) -> %s" % (nimg, rows, cols, levels, STATUS_NAMES.get(rc, rc)))
    return int(out.value)


class MatchOptions(namedtuple("MatchOptions", "cross_check_stereo cross_check_f2f gated_stereo gated_f2f gated_max_distance "
                                              "ratio_stereo ratio_f2f ratio")):
    """The matchers' options as ONE value, the `match` of a StepOptions: what every public constructor builds and passes inward,
    down to the flags of a batch configuration (flags()) or the arguments of Context.match_1nn.  Checked on construction by
    the three flag functions above (their ValueErrors).  Immutable and hashable: it is its own engine-cache key.  A new
    matcher option is a field here, an argument of Context.match_1nn and of match_1nn in pipeline.hip."""
    __slots__ = ()

    def __new__(cls, cross_check_stereo=False, cross_check_f2f=False, gated_stereo=False, gated_f2f=False,
                gated_max_distance=None, ratio_stereo=False, ratio_f2f=False, ratio=None):
        v = super().__new__(cls, bool(cross_check_stereo), bool(cross_check_f2f), bool(gated_stereo), bool(gated_f2f),
                            gated_max_distance, bool(ratio_stereo), bool(ratio_f2f), ratio)
        v.flags()
        return v

    def flags(self):
        """The options' bits of sosvo_batch_cfg.ransac_flags / sosvo_rgbd_batch_cfg.flags."""
        return (cross_check_flags(self.cross_check_stereo, self.cross_check_f2f)
                | gated_flags(self.gated_stereo, self.gated_f2f, self.gated_max_distance)
                | ratio_flags(self.ratio_stereo, self.ratio_f2f, self.ratio))

    @property
    def ratio_64ths_stereo(self):
        """The static-stereo matcher's ratio in 64ths; 0: off."""
        return ratio_64ths(self.ratio) if self.ratio_stereo else 0

    @property
    def ratio_64ths_f2f(self):
        return ratio_64ths(self.ratio) if self.ratio_f2f else 0

    @classmethod
    def rgbd(cls, cross_check=False, gated_f2f=False, gated_max_distance=None, ratio_f2f=False, ratio=None):
        """From the RGB-D classes' names: a camera without static stereo has the frame-to-frame matcher only."""
        return cls(cross_check_f2f=cross_check, gated_f2f=gated_f2f, gated_max_distance=gated_max_distance, ratio_f2f=ratio_f2f,
                   ratio=ratio)

    def rgbd_kwargs(self):
        """The inverse of rgbd()."""
        return dict(cross_check=self.cross_check_f2f, gated_f2f=self.gated_f2f, gated_max_distance=self.gated_max_distance,
                    ratio_f2f=self.ratio_f2f, ratio=self.ratio)

    @classmethod
    def from_matchers(cls, fm_stereo, fm_f2f):
        """What a batched engine runs for a pair of FeatureMatchers (None: no such matcher), or None when they have no batched
        counterpart: an engine has one cap and one ratio for both matchers.  Cap and ratio of a matcher that is off are dropped."""
        fms = (fm_stereo, fm_f2f)
        cross, gated = ([bool(getattr(fm, name, False)) for fm in fms] for name in ("cross_check", "gated"))
        caps = {getattr(fm, "gated_max_distance", None) for fm, on in zip(fms, gated) if on}
        ratios = [getattr(fm, "ratio", None) for fm in fms]
        if len(caps) > 1 or len({r for r in ratios if r is not None}) > 1:
            return None
        return cls(cross[0], cross[1], gated[0], gated[1], caps.pop() if caps else None, ratios[0] is not None,
                   ratios[1] is not None, ratios[0] if ratios[0] is not None else ratios[1])


class StepOptions(namedtuple("StepOptions", "match subpix lk stereo_lk cyclic")):
    """Everything a step can be told, as ONE value: `match` a MatchOptions; `subpix` the window half-size 2 .. 5 of the sub-pixel
    keypoint refinement or None; `lk` the LKOptions of a step that tracks frame to frame, None for one that matches;
    `stereo_lk` the StereoLKOptions of one that refines its static stereo, or None; `cyclic`: False, True (the panorama columns are one
    period) or "seam_free" (True plus the seam-free front end).  Every public constructor builds one from its own arguments first (of() / rgbd() run the checks) and uses it from
    there, down to flags().  Hashable: its own engine-cache key.  A new option is a field here, a public keyword and its C flag."""
    __slots__ = ()
    # of()'s checks in the order the pair pipeline and the batched layers have always run them: of two broken rules the first
    # one speaks.  "lk" parses the tracker's settings alone; "tracker" is f2f_tracker_options, and gives `lk` too
    PAIR_ORDER = ("lk", "cyclic", "stereo_lk", "tracker", "subpix", "match")
    BATCH_ORDER = ("match", "tracker", "stereo_lk", "cyclic", "subpix")

    def __new__(cls, match=None, subpix=None, lk=None, stereo_lk=None, cyclic=False):
        return super().__new__(cls, MatchOptions() if match is None else match, subpix_half(subpix), lk, stereo_lk, cyclic_value(cyclic))

    def flags(self):
        """The options' bits of sosvo_batch_cfg.ransac_flags (an RGB-D value has the matcher's alone: sosvo_rgbd_batch_cfg.flags)."""
        return (self.match.flags() | subpix_flags(self.subpix) | (FLAG_LK_F2F if self.lk is not None else 0)
                | (FLAG_LK_STEREO if self.stereo_lk is not None else 0) | (FLAG_CYCLIC_F2F if self.cyclic else 0)
                | (FLAG_SEAM_FREE if self.cyclic == SEAM_FREE else 0))

    @property
    def seam_free(self):
        """The front end is the seam-free one (cyclic == "seam_free")."""
        return self.cyclic == SEAM_FREE

    @classmethod
    def of(cls, cross_check_stereo=False, cross_check_f2f=False, gated_stereo=False, gated_f2f=False, gated_max_distance=None,
           ratio_stereo=False, ratio_f2f=False, ratio=None, subpix=None, f2f_tracker="match", lk=None, stereo_refine=None,
           stereo_lk=None, cyclic_columns=False, rig=None, store_levels=None, order=BATCH_ORDER, tracker_sees_match=True,
           gray=True, detection_method="GFT", edge=31):
        """From the public keyword names (FramePairPipeline's docstring describes them), checked.  rig: a RigConfig or the
        panoramas' (top, bottom) widths, the period of cyclic_columns (not looked at without).  store_levels: the pyramid levels
        a frame store keeps whatever the settings (the batched engines: SOSVO_LK_MAX_LEVELS), None for a caller that builds the
        levels it tracks on.  order: the checks to run, in turn.  tracker_sees_match: f2f_tracker="lk" refuses the options of
        the matcher it replaces ("match" comes before "tracker" then).  gray: False = no gray panoramas to read (a pair
        pipeline without a front end): what reads them is refused.  detection_method, edge: what cyclic_columns="seam_free" looks at besides the widths."""
        def needs_gray(on, what, who):
            if on is not None and not gray:
                raise ValueError("%s needs a front end: the %s reads the gray panoramas" % (what, who))
            return on

        def cyclic():
            if not cyclic_columns:
                return False
            o, widths = v["lk"], (rig.pano_top[0], rig.pano_bot[0]) if hasattr(rig, "pano_top") else tuple(rig)
            for w in widths:
                if not (w == int(w) and 1 <= w <= 16384):
                    raise ValueError("cyclic_columns: the panorama width must be a positive integer up to 16384, got %r" % (w,))
            for w in widths if o is not None else ():
                levels = max(o.levels, store_levels or 1)
                if int(w) % (1 << (levels - 1)) or (int(w) >> (o.levels - 1)) < 2 * o.half + 3:
                    raise ValueError("cyclic_columns with f2f_tracker=\"lk\": a panorama width of %d columns is no multiple of %d, or "
                                     "its top level is narrower than the %d-column template" % (w, 1 << (levels - 1), 2 * o.half + 3))
            if gated_f2f and ratio_f2f:
                raise ValueError("cyclic_columns: the ratio form of the gated frame-to-frame matcher has no cyclic gate")
            if gated_f2f and widths[0] != widths[1]:
                raise ValueError("cyclic_columns with gated_f2f: one search serves both views, their widths must be equal (%r, %r)"
                                 % widths)
            if cyclic_value(cyclic_columns) == SEAM_FREE:
                if not gray:
                    raise ValueError("cyclic_columns=\"seam_free\" needs a front end: it is the front end that changes")
                if widths[0] != widths[1]:
                    raise ValueError("cyclic_columns=\"seam_free\": both panoramas must have one width (%r, %r)" % widths)
                seam_free_check(widths, detection_method, edge)
            return cyclic_value(cyclic_columns)
        match = (cross_check_stereo, cross_check_f2f, gated_stereo, gated_f2f, gated_max_distance, ratio_stereo, ratio_f2f, ratio)
        v, checks = {}, dict(
            match=lambda: MatchOptions(*match),
            lk=lambda: LKOptions.of(lk) if f2f_tracker == "lk" else None,
            tracker=lambda: needs_gray(f2f_tracker_options(f2f_tracker, lk, v["match"] if tracker_sees_match else None),
                                       "f2f_tracker=\"lk\"", "tracker"),
            stereo_lk=lambda: needs_gray(stereo_refine_options(stereo_refine, stereo_lk), "stereo_refine=\"lk\"", "refinement"),
            subpix=lambda: subpix_half(needs_gray(subpix, "subpix", "refinement")), cyclic=cyclic)
        for name in order:
            v["lk" if name == "tracker" else name] = checks[name]()
        if v.get("cyclic") == SEAM_FREE:    # (the refinement's settings may be parsed after the widths: PAIR_ORDER)
            seam_free_check((), stereo_lk=v.get("stereo_lk"))
        return cls(**v)

    @classmethod
    def rgbd(cls, cross_check=False, gated_f2f=False, gated_max_distance=None, ratio_f2f=False, ratio=None, f2f_tracker="match",
             lk=None, stereo_refine=None, stereo_lk=None, cyclic_columns=False):
        """From the RGB-D classes' names: a camera without static stereo has the frame-to-frame matcher only (`match` is
        MatchOptions.rgbd), no tracker, and a pinhole image that is not cyclic -- asking for one of these is a ValueError."""
        f2f_tracker_options(f2f_tracker, lk, rgbd=True)
        stereo_refine_options(stereo_refine, stereo_lk, rgbd=True)
        if cyclic_columns:
            raise ValueError("cyclic_columns: an RGB-D camera's pinhole image is not cyclic")
        return cls(MatchOptions.rgbd(cross_check, gated_f2f, gated_max_distance, ratio_f2f, ratio))

    def kwargs(self):
        """The inverse of of(): the public keywords of a constructor that is handed this value.  Options that came after the
        matcher's are left out when they are off, so that such a constructor is called as it was before they existed."""
        kw = dict(self.match._asdict(), subpix=self.subpix)
        if self.lk is not None:
            kw.update(f2f_tracker="lk", lk=self.lk)
        if self.stereo_lk is not None:
            kw.update(stereo_refine="lk", stereo_lk=self.stereo_lk)
        if self.cyclic:
            kw.update(cyclic_columns=self.cyclic)
        return kw

    @classmethod
    def from_tracker(cls, tracker, camera_model):
        """What a batched engine runs for a tracker and its camera model, read where the set_* functions of pose_est_tools wrote
        it (the matchers, tracker.lk_options, camera_model.cyclic_columns); None where MatchOptions.from_matchers is."""
        fm = getattr(camera_model, "feature_matcher_for_static_stereo", None)
        match = MatchOptions.from_matchers(fm, getattr(camera_model, "feature_matcher_for_motion", None))
        return None if match is None else cls(match, getattr(fm, "subpix_half", None), getattr(tracker, "lk_options", None),
                                              getattr(fm, "stereo_lk_options", None), getattr(camera_model, "cyclic_columns", False))


DENSE_CYCLIC_COLUMNS = 1           # SOSVO_DENSE_CYCLIC_COLUMNS: the census taps wrap modulo cols
DENSE_DISPARITIES = 64             # SOSVO_DENSE_DISPARITIES: one lane of a wave per disparity
DENSE_MAX_P2, DENSE_MAX_MIN_DISPARITY = 8191, 1024
DENSE_MAX_P2_EIGHT_PATHS = 8127    # SOSVO_DENSE_MAX_P2_EIGHT_PATHS: S = the sum of eight L <= 8 * (64 + P2) stays u16


def dense_paths(paths, options=None):
    """A `paths` argument of the dense stage -> 4 or 8, checked against the options it goes with: 4 =
    down, up, left to right, right to left; 8 = those and the four diagonals, the reference tuner's "Full DP" trackbar
    (paths = 8 if tuner.full_dyn_prog else 4).  Anything else, and 8 with P2 > 8127, raises ValueError."""
    if isinstance(paths, bool) or not isinstance(paths, int) or paths not in (4, 8):
        raise ValueError("dense paths must be 4 or 8, got %r" % (paths,))
    if paths == 8 and DenseOptions.of(options).P2 > DENSE_MAX_P2_EIGHT_PATHS:
        raise ValueError("dense paths = 8 needs P2 <= %d, got %r" % (DENSE_MAX_P2_EIGHT_PATHS, DenseOptions.of(options).P2))
    return paths


DENSE_WIDE_MIN_DISPARITIES, DENSE_WIDE_MAX_DISPARITIES = 16, 256   # SOSVO_DENSE_WIDE_MIN / MAX_DISPARITIES


def dense_disparities(disparities, paths=4, options=None):
    """A `disparities` argument of the dense stage -> the number D of disparities searched from
    options.min_disparity on, checked together with the `paths` and the options it goes with (dense_paths): a multiple of 16
    in 16 .. 256, the reference tuner's num_of_disparities (disparities = tuner.num_of_disparities).  64 is the stage as it
    was (sosvo_dense_stereo / sosvo_dense_stereo_paths); every other value runs sosvo_dense_stereo_wide.  Anything else raises
    ValueError."""
    dense_paths(paths, options)
    if (isinstance(disparities, bool) or not isinstance(disparities, int) or disparities % 16 != 0
            or not DENSE_WIDE_MIN_DISPARITIES <= disparities <= DENSE_WIDE_MAX_DISPARITIES):
        raise ValueError("dense disparities must be a multiple of 16 in %d .. %d, got %r"
                         % (DENSE_WIDE_MIN_DISPARITIES, DENSE_WIDE_MAX_DISPARITIES, disparities))
    return disparities


class DenseOptions(namedtuple("DenseOptions", "min_disparity P1 P2 uniqueness lr_max cyclic")):
    """The settings of the dense stereo stage (sosvo_dense_stereo) as one checked value: min_disparity
    0 .. 1024 rows (the first of the 64 disparities searched), the smoothness penalties 0 <= P1 <= P2 <= 8191 (the reference's
    tuner passes P1 = P2 = 0: no smoothness), uniqueness 0 .. 99 per cent, lr_max the largest |k* difference| the left-right
    check lets pass (negative: no check, the reference's disp12MaxDiff = -1), cyclic: the census taps wrap around the
    panorama's seam.  A value out of range raises ValueError; nothing is rounded.  It is not a field of StepOptions: dense
    stereo is no step of the VO pair."""
    __slots__ = ()

    def __new__(cls, min_disparity=1, P1=8, P2=48, uniqueness=15, lr_max=1, cyclic=False):
        def integer(name, v, lo, hi):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or int(v) != v or not lo <= v <= hi:
                raise ValueError("dense %s must be an integer in %d .. %d, got %r" % (name, lo, hi, v))
            return int(v)
        d0 = integer("min_disparity", min_disparity, 0, DENSE_MAX_MIN_DISPARITY)
        p2 = integer("P2", P2, 0, DENSE_MAX_P2)
        p1 = integer("P1", P1, 0, DENSE_MAX_P2)
        if p1 > p2:
            raise ValueError("dense P1 must not exceed P2, got P1 %r, P2 %r" % (P1, P2))
        return super().__new__(cls, d0, p1, p2, integer("uniqueness", uniqueness, 0, 99),
                               integer("lr_max", lr_max, -(1 << 31), (1 << 31) - 1), bool(cyclic))

    @classmethod
    def of(cls, value):
        """An `options` argument (None: the defaults; a DenseOptions; a dict of its fields) -> the value."""
        if value is None or isinstance(value, cls):
            return cls() if value is None else value
        if not isinstance(value, dict):
            raise ValueError("options must be None, a DenseOptions or a dict of its fields, got %r" % (value,))
        if set(value) - set(cls._fields):
            raise ValueError("options: unknown settings %s" % sorted(set(value) - set(cls._fields)))
        return cls(**value)

    @property
    def flags(self):
        """The flags word of sosvo_dense_stereo / sosvo_census_9x7."""
        return DENSE_CYCLIC_COLUMNS if self.cyclic else 0


SPECKLE_MAX_DIFF = 32767           # sosvo_dense_speckle: max_diff is compared with a difference of two int16 values
SPECKLE_TUNER_SCALE = 16           # cv2.StereoSGBM compares 16 * speckleRange with its 1/16-pixel disparities


class SpeckleOptions(namedtuple("SpeckleOptions", "max_size max_diff cyclic")):
    """The settings of the speckle filter (sosvo_dense_speckle) as one checked value: max_size 0 ..
    2^31 - 1 pixels (a component of at most that many pixels is removed; 0 removes nothing), max_diff 0 .. 32767 in 1/16 row
    (two neighbours are joined when their d16 differ by at most that), cyclic: the last column is joined to the first.
    Integers only; a value out of range raises ValueError; nothing is rounded.  A value of its own: no field of DenseOptions
    and none of StepOptions."""
    __slots__ = ()

    def __new__(cls, max_size=100, max_diff=16, cyclic=False):
        def integer(name, v, hi):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or int(v) != v or not 0 <= v <= hi:
                raise ValueError("speckle %s must be an integer in 0 .. %d, got %r" % (name, hi, v))
            return int(v)
        if not isinstance(cyclic, (bool, int)) or cyclic not in (0, 1):
            raise ValueError("speckle cyclic must be a bool, got %r" % (cyclic,))
        return super().__new__(cls, integer("max_size", max_size, (1 << 31) - 1), integer("max_diff", max_diff, SPECKLE_MAX_DIFF),
                               bool(cyclic))

    @classmethod
    def of(cls, value):
        """A `speckle` argument (None: the filter is off, None comes back; a SpeckleOptions; a dict of its fields) -> the value."""
        if value is None or isinstance(value, cls):
            return value
        if not isinstance(value, dict):
            raise ValueError("speckle must be None, a SpeckleOptions or a dict of its fields, got %r" % (value,))
        if set(value) - set(cls._fields):
            raise ValueError("speckle: unknown settings %s" % sorted(set(value) - set(cls._fields)))
        return cls(**value)

    @classmethod
    def from_tuner(cls, speckle_window_size, speckle_range, cyclic=False):
        """The reference's two sliders (common_cv.StereoMatchTuner: "Speckle Window Size", "Speckle Range", handed to
        cv2.StereoSGBM as speckleWindowSize / speckleRange) -> the value: window 0 switches the filter off (None), and
        max_diff = 16 * speckle_range, the factor OpenCV applies to its 1/16-pixel disparities."""
        window = cls(max_size=speckle_window_size).max_size
        if isinstance(speckle_range, bool) or not isinstance(speckle_range, (int, float)) or int(speckle_range) != speckle_range:
            raise ValueError("speckle_range must be an integer, got %r" % (speckle_range,))
        return None if window == 0 else cls(window, SPECKLE_TUNER_SCALE * int(speckle_range), cyclic)

    @property
    def flags(self):
        """The flags word of sosvo_dense_speckle."""
        return DENSE_CYCLIC_COLUMNS if self.cyclic else 0


WLS_MAX_LAMBDA, WLS_MAX_ITERS, WLS_MAX_RADIUS, WLS_MAX_ROLL_PPM = 1.0e6, 8, 7, 1000000


class WlsOptions(namedtuple("WlsOptions", "lam sigma iters radius roll_ppm min_weight cyclic")):
    """The settings of the WLS disparity filter (sosvo_dense_confidence, sosvo_dense_wls in include/sosvo_dense_filter.h,
    DESIGN.md section 41) as one checked value: lam 0 .. 10^6 (the smoothing weight, the reference's "WLS lambda"), sigma > 0
    (two neighbours whose gray values differ by k have the affinity exp(-k / sigma); the reference's "WLS sigma" / 100), iters
    1 .. 8 passes of the row and the column solve, radius 0 .. 7 and roll_ppm 0 .. 10^6 of the confidence's variance window,
    min_weight > 0 (a pixel whose smoothed confidence stays below 255 * min_weight has no disparity), cyclic: the last column
    neighbours the first.  A value out of range raises ValueError; nothing is rounded.  A value of its own: no field of
    DenseOptions and none of StepOptions."""
    __slots__ = ()

    def __new__(cls, lam=8000.0, sigma=1.0, iters=3, radius=3, roll_ppm=1000, min_weight=2.0 ** -20, cyclic=False):
        def integer(name, v, lo, hi):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or int(v) != v or not lo <= v <= hi:
                raise ValueError("wls %s must be an integer in %d .. %d, got %r" % (name, lo, hi, v))
            return int(v)

        def number(name, v, ok, what):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float("inf"), -float("inf")) or not ok(v):
                raise ValueError("wls %s must be %s, got %r" % (name, what, v))
            return float(v)
        if not isinstance(cyclic, (bool, int)) or cyclic not in (0, 1):
            raise ValueError("wls cyclic must be a bool, got %r" % (cyclic,))
        return super().__new__(cls, number("lam", lam, lambda v: 0 <= v <= WLS_MAX_LAMBDA, "a number in 0 .. 10^6"),
                               number("sigma", sigma, lambda v: v > 0, "a finite number above 0"),
                               integer("iters", iters, 1, WLS_MAX_ITERS), integer("radius", radius, 0, WLS_MAX_RADIUS),
                               integer("roll_ppm", roll_ppm, 0, WLS_MAX_ROLL_PPM),
                               number("min_weight", min_weight, lambda v: v > 0, "a finite number above 0"), bool(cyclic))

    @classmethod
    def of(cls, value):
        """A `wls` argument (None: the filter is off, None comes back; a WlsOptions; a dict of its fields) -> the value."""
        if value is None or isinstance(value, cls):
            return value
        if not isinstance(value, dict):
            raise ValueError("wls must be None, a WlsOptions or a dict of its fields, got %r" % (value,))
        if set(value) - set(cls._fields):
            raise ValueError("wls: unknown settings %s" % sorted(set(value) - set(cls._fields)))
        return cls(**value)

    @classmethod
    def from_tuner(cls, use_WLS_filter, wls_lambda, wls_sigma, cyclic=False):
        """The reference's three controls (common_cv.StereoMatchTuner: "Use WLS filter", "WLS lambda", "WLS sigma") -> the
        value: the switch off gives None, and sigma = wls_sigma / 100 as common_cv.py:679 hands it to setSigmaColor."""
        if use_WLS_filter not in (0, 1):
            raise ValueError("use_WLS_filter must be a bool, got %r" % (use_WLS_filter,))
        if isinstance(wls_sigma, bool) or not isinstance(wls_sigma, (int, float)):
            raise ValueError("wls_sigma must be a number, got %r" % (wls_sigma,))
        value = cls(lam=wls_lambda, sigma=wls_sigma / 100.0, cyclic=cyclic)
        return value if use_WLS_filter else None

    def weight_table(self):
        """The 256 doubles sosvo_dense_wls takes: exp(-k / sigma) for the gray difference k, made here once so that the
        device and the numpy reference read the same table (the device evaluates no exponential)."""
        import math
        return [math.exp(-k / self.sigma) for k in range(256)]

    @property
    def flags(self):
        """The flags word of sosvo_dense_confidence / sosvo_dense_wls."""
        return DENSE_CYCLIC_COLUMNS if self.cyclic else 0


def rgbd_flags_detector(flags):
    """SOSVO_RGBD_DETECTOR_OF(flags)."""
    return (int(flags) & RGBD_DETECTOR_MASK) >> RGBD_DETECTOR_SHIFT


_lib = None


def declared_functions(header_path=HEADER_PATH):
    """Names of all functions declared in include/sosvo.h."""
    text = open(header_path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sosvo_[a-z0-9_]+)\s*\(", text)))


def load():
    """Load libsosvo.so (once).  Raises SosvoError loudly when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SosvoError(
            "libsosvo.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C vo_single_camera_sos_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    # torch must be imported first so that its bundled libamdhip64.so.7 is the HIP runtime
    # this library binds to (one runtime per process).
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise SosvoError("libsosvo.so does not export %s; rebuild it" % name)
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib
