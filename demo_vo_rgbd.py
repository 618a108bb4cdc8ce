#!/usr/bin/env python3
"""Frame-to-frame visual odometry on an RGB-D sequence -- same entry point and arguments as the reference's
demo_vo_rgbd.py, running the hot path on the MI355X through libsosvo.

    python demo_vo_rgbd.py <sequence_path> [<sequence_path> ...] --is_synthetic true [--hand_eye_transformation file]

<sequence_path>/rgbd/rgb/*.png and <sequence_path>/rgbd/depth/*.png (16-bit, millimetres) are the frames; results
go to <sequence_path>/results-rgbd/; <sequence_path>/rgbd/gt_TUM.txt is used as ground truth when present.
Several sequence paths (the same camera) are tracked together as the lanes of one engine (run_VO_many)."""
import fnmatch
import os.path as osp
import sys
from argparse import ArgumentParser
from os import listdir

import numpy as np

ROOT = osp.dirname(osp.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    from vo_single_camera_sos_amd.omnistereo.common_tools import add_f2f_tracker_arguments, str2bool
    parser = ArgumentParser(description="Demo of frame-to-frame visual odometry for RGB-D images.")
    parser.register("type", "bool", str2bool)
    parser.add_argument("sequence_path", nargs="+", help="The path to the sequence where the rgbd folder is located (several "
                        "paths: sequences of the same camera, tracked together).")
    parser.add_argument("--lanes", default=-1, type=int,
                        help="several sequence paths: how many are tracked concurrently (-1 = all)")
    parser.add_argument("--is_synthetic", type="bool", default=True,
                        help="Synthetic data (radial depth, POV-Ray intrinsics) or real data (Z depth, 525 px)")
    parser.add_argument("--hand_eye_transformation", default="rgbd_hand_eye_transformation.txt", type=str)
    parser.add_argument("--visualize_VO", default=False, type="bool", help="not built, must stay false")
    parser.add_argument("--first_image_index", default=0, type=int)
    parser.add_argument("--last_image_index", default=-1, type=int)
    parser.add_argument("--step", default=1, type=int)
    parser.add_argument("--use_multithreads_for_VO", default=True, type="bool")
    parser.add_argument("--frame_window", default=-1, type=int,
                        help="sequence mode: frames per batched front-end pass on the GPU (-1 = default 32; 0 = the per-frame "
                             "mirror path).  The pose file does not depend on the window size.")
    parser.add_argument("--detection_method", default="GFT", choices=("GFT", "ORB", "FAST", "AGAST"), type=str.upper,
                        help="keypoint detector of the tracker and its frames (GFT: the reference's default)")
    parser.add_argument("--cross_check", action="store_true",
                        help="mutual matches only (cv2.BFMatcher's crossCheck) in the frame-to-frame matcher; default: off")
    parser.add_argument("--gated_matching", action="store_true",
                        help="the frame-to-frame matcher searches among the keypoints within the tracker's |du| gate; default: off")
    parser.add_argument("--gated_max_distance", default=None, type=int,
                        help="with --gated_matching: a match whose Hamming distance exceeds this (1 .. 256) is no match; default: no cap")
    parser.add_argument("--ratio_test", action="store_true",
                        help="Lowe's ratio rule in the frame-to-frame matcher, on the GPU; needs --ratio; default: off")
    parser.add_argument("--ratio", default=None, type=float,
                        help="with --ratio_test: keep a match iff its distance is below this times the runner-up's; a multiple "
                             "of 1/64 in (0, 1), e.g. 0.75")
    parser.add_argument("--subpix_refine", action="store_true",
                        help="move the detected keypoints to their sub-pixel positions (cornerSubPix, on the GPU) before the "
                             "static-stereo matching; default: off (an RGB-D camera reads depth at integer pixels: refused)")
    parser.add_argument("--subpix_half", default=None, type=int,
                        help="with --subpix_refine: the window half-size 2 .. 5; default: 5")
    add_f2f_tracker_arguments(parser)
    return parser


def main_rgbd_vo(argv=None):
    from vo_single_camera_sos_amd.omnistereo.common_tools import f2f_tracker_arguments, get_poses_from_file, make_sure_path_exists
    parser = build_parser()
    args = parser.parse_args(argv)

    from vo_single_camera_sos_amd.omnistereo.camera_models import RGBDCamModel
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import driver_VO, driver_VO_many
    from vo_single_camera_sos_amd.omnistereo.transformations import rotation_matrix
    hand_eye_T = None
    if args.is_synthetic:   # demo_vo_rgbd.py:66-84
        fx = fy = 554.256258
        depth_is_Z = False
        hand_eye_T = rotation_matrix(-np.pi / 2.0, [1, 0, 0])
    else:                   # :85-94
        fx = fy = 525.0
        depth_is_Z = True
        fn = osp.realpath(osp.expanduser(args.hand_eye_transformation))
        if osp.isfile(fn):
            hand_eye_T = get_poses_from_file(poses_filename=fn, input_units="m", output_working_units="m", indices=None,
                                             pose_format="tum", zero_up_wrt_origin=False, initial_T=None)[1][0]
    scenes = []
    for path in args.sequence_path:
        scene_path = osp.realpath(osp.expanduser(path))
        scene_path_rgbd = osp.join(scene_path, "rgbd")
        rgb_template = osp.join(scene_path_rgbd, "rgb", "*.png")
        depth_template = osp.join(scene_path_rgbd, "depth", "*.png")
        num_scene_images = len(fnmatch.filter(listdir(osp.join(scene_path_rgbd, "rgb")), "*.png"))
        results = osp.join(scene_path, "results-rgbd")
        make_sure_path_exists(results)
        _, scene_name = osp.split(scene_path)
        scenes.append(dict(scene_path=scene_path_rgbd, scene_path_vo_results=results, scene_img_filename_template=rgb_template,
                           depth_filename_template=depth_template, num_scene_images=num_scene_images,
                           thread_name="%s-%s" % (scene_name, "RGB-D")))
    cam = RGBDCamModel(fx=fx, fy=fy, center_x=319.5, center_y=239.5, scaling_factor=1. / 1000.0, do_undistortion=False,
                       depth_is_Z=depth_is_Z, focal_length_m=1. / 1000.0)
    cam.T_Cest_wrt_Rgt = hand_eye_T
    if len(scenes) > 1:
        out = driver_VO_many(camera_model=cam, scenes=scenes, visualize_VO=args.visualize_VO, step_for_scene_images=args.step,
                             first_image_index=args.first_image_index, last_image_index=args.last_image_index,
                             frame_window=None if args.frame_window < 0 else args.frame_window,
                             detection_method=args.detection_method, cross_check=True if args.cross_check else None,
                             gated_matching=True if args.gated_matching else None, gated_max_distance=args.gated_max_distance,
                             ratio_test=True if args.ratio_test else None, ratio=args.ratio,
                             subpix_refine=True if args.subpix_refine else None, subpix_half=args.subpix_half, **f2f_tracker_arguments(args),
                             lanes=None if args.lanes < 0 else args.lanes)
        print("GOODBYE!")
        return out
    out = driver_VO(camera_model=cam, scene_path=scene_path_rgbd, scene_path_vo_results=results,
                    scene_img_filename_template=rgb_template, depth_filename_template=depth_template,
                    num_scene_images=num_scene_images, visualize_VO=args.visualize_VO,
                    use_multithreads_for_VO=args.use_multithreads_for_VO, step_for_scene_images=args.step,
                    first_image_index=args.first_image_index, last_image_index=args.last_image_index,
                    thread_name="%s-%s" % (scene_name, "RGB-D"),
                    frame_window=None if args.frame_window < 0 else args.frame_window,
                    detection_method=args.detection_method, cross_check=True if args.cross_check else None,
                    gated_matching=True if args.gated_matching else None, gated_max_distance=args.gated_max_distance,
                    ratio_test=True if args.ratio_test else None, ratio=args.ratio,
                    subpix_refine=True if args.subpix_refine else None, subpix_half=args.subpix_half, **f2f_tracker_arguments(args))
    print("GOODBYE!")
    return out


if __name__ == "__main__":
    main_rgbd_vo()
