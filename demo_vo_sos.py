#!/usr/bin/env python3
"""Frame-to-frame visual odometry on a single-camera omnistereo (SOS) sequence -- same entry point and arguments
as the reference's demo_vo_sos.py, running the hot path on the MI355X through libsosvo.

    python demo_vo_sos.py <sequence_path> [<sequence_path> ...] --calibrated_gums_file gums-calibrated.json [--visualize_VO false]

<sequence_path>/omni/image-*.png are the omni frames; results go to <sequence_path>/results-omni/
(estimated_frame_poses_TUM.txt, gt_associated_frame_poses_TUM.txt, keyframe_ids.txt, printed_messages.log);
<sequence_path>/omni/gt_TUM.txt is used as ground truth when present.  The calibrated rig is a JSON document
(vo_single_camera_sos_amd.omnistereo.gum.save_gums_json) instead of the reference's pickle of live objects.
Several sequence paths (recorded with the same rig) are tracked together as the lanes of one engine (run_VO_many); each
gets the result files it would get on its own."""
import fnmatch
import os.path as osp
import sys
from argparse import ArgumentParser
from os import listdir

ROOT = osp.dirname(osp.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    from vo_single_camera_sos_amd.omnistereo.common_tools import add_f2f_tracker_arguments, add_stereo_refine_arguments, str2bool
    parser = ArgumentParser(description="Demo of frame-to-frame visual odometry for the Single-camera SOS images.")
    parser.register("type", "bool", str2bool)
    parser.add_argument("sequence_path", nargs="+", help="The path to the sequence where the omni folder is located (several "
                        "paths: sequences of the same rig, tracked together).")
    parser.add_argument("--lanes", default=-1, type=int,
                        help="several sequence paths: how many are tracked concurrently (-1 = all)")
    parser.add_argument("--calibrated_gums_file", default="gums-calibrated.json", type=str,
                        help="Complete path and name of the calibrated GUMS file (JSON)")
    parser.add_argument("--visualize_VO", default=False, type="bool",
                        help="(Optional) 3-D visualisation of the trajectory: not built, must stay false")
    parser.add_argument("--first_image_index", default=0, type=int)
    parser.add_argument("--last_image_index", default=-1, type=int, help="-1 for up to the last one")
    parser.add_argument("--step", default=1, type=int)
    parser.add_argument("--use_multithreads_for_VO", default=True, type="bool")
    parser.add_argument("--frame_window", default=-1, type=int,
                        help="sequence mode: frames per batched front-end pass on the GPU (-1 = default 32; 0 = the per-frame "
                             "mirror path).  The pose file does not depend on the window size.")
    parser.add_argument("--detection_method", default="GFT", choices=("GFT", "ORB", "FAST", "AGAST"), type=str.upper,
                        help="keypoint detector of the tracker and its frames (GFT: the reference's default)")
    parser.add_argument("--cross_check", nargs="?", const="both", default=None, choices=("both", "stereo", "f2f"),
                        help="mutual matches only (cv2.BFMatcher's crossCheck): in both matchers when given without a value, "
                             "or in the static-stereo / the frame-to-frame matcher alone; default: off")
    parser.add_argument("--gated_matching", nargs="?", const="both", default=None, choices=("both", "stereo", "f2f"),
                        help="the matchers search among the candidates that pass their pixel gates: both matchers when given "
                             "without a value, or the static-stereo / the frame-to-frame matcher alone; default: off")
    parser.add_argument("--gated_max_distance", default=None, type=int,
                        help="with --gated_matching: a match whose Hamming distance exceeds this (1 .. 256) is no match; default: no cap")
    parser.add_argument("--ratio_test", nargs="?", const="both", default=None, choices=("both", "stereo", "f2f"),
                        help="Lowe's ratio rule in the matchers, on the GPU: both matchers when given without a value, or the "
                             "static-stereo / the frame-to-frame matcher alone; needs --ratio; default: off")
    parser.add_argument("--ratio", default=None, type=float,
                        help="with --ratio_test: keep a match iff its distance is below this times the runner-up's; a multiple "
                             "of 1/64 in (0, 1), e.g. 0.75")
    parser.add_argument("--subpix_refine", action="store_true",
                        help="move the detected keypoints to their sub-pixel positions (cornerSubPix, on the GPU) before the "
                             "static-stereo matching; default: off")
    parser.add_argument("--subpix_half", default=None, type=int,
                        help="with --subpix_refine: the window half-size 2 .. 5; default: 5")
    add_f2f_tracker_arguments(parser)
    add_stereo_refine_arguments(parser)
    parser.add_argument("--cyclic_columns", action="store_true",
                        help="the panoramas are full circles: the frame-to-frame |du| gate (and, with --f2f_tracker lk, the pyramids "
                             "and the tracker) go across the seam between the last and the first column; default: off")
    parser.add_argument("--seam_free", action="store_true",
                        help="--cyclic_columns plus the seam-free front end: keypoints and stereo points up to the seam (the image "
                             "stages run on panoramas padded by 40 cyclic columns on either side); default: off")
    return parser


def main_sos_vo(argv=None):
    from vo_single_camera_sos_amd.omnistereo.common_tools import f2f_tracker_arguments, make_sure_path_exists, stereo_refine_arguments
    parser = build_parser()
    args = parser.parse_args(argv)

    from vo_single_camera_sos_amd.omnistereo.gum import load_gums_json
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import driver_VO, driver_VO_many
    gums_file = osp.realpath(osp.expanduser(args.calibrated_gums_file))
    scene_prefix_filename = "image-*.png"
    scenes = []
    for path in args.sequence_path:
        scene_path = osp.realpath(osp.expanduser(path))
        scene_path_omni = osp.join(scene_path, "omni")
        template = osp.join(scene_path_omni, scene_prefix_filename)
        num_scene_images = len(fnmatch.filter(listdir(scene_path_omni), scene_prefix_filename))
        results = osp.join(scene_path, "results-omni")
        make_sure_path_exists(results)
        _, scene_name = osp.split(scene_path)
        scenes.append(dict(scene_path=scene_path_omni, scene_path_vo_results=results, scene_img_filename_template=template,
                           depth_filename_template=None, num_scene_images=num_scene_images,
                           thread_name="%s-%s" % (scene_name, "SOS")))
    gums_calibrated = load_gums_json(gums_file)
    cross_check = None if args.cross_check is None else (True if args.cross_check == "both" else args.cross_check)
    gated = dict(gated_matching=None if args.gated_matching is None else (True if args.gated_matching == "both" else args.gated_matching),
                 gated_max_distance=args.gated_max_distance,
                 ratio_test=None if args.ratio_test is None else (True if args.ratio_test == "both" else args.ratio_test),
                 ratio=args.ratio, subpix_refine=True if args.subpix_refine else None, subpix_half=args.subpix_half, **f2f_tracker_arguments(args),
                 **stereo_refine_arguments(args), cyclic_columns="seam_free" if args.seam_free else (True if args.cyclic_columns else None))
    if len(scenes) > 1:
        out = driver_VO_many(camera_model=gums_calibrated, scenes=scenes, visualize_VO=args.visualize_VO,
                             step_for_scene_images=args.step, first_image_index=args.first_image_index,
                             last_image_index=args.last_image_index, frame_window=None if args.frame_window < 0 else args.frame_window,
                             detection_method=args.detection_method, cross_check=cross_check,
                             lanes=None if args.lanes < 0 else args.lanes, **gated)
        print("GOODBYE!")
        return out
    out = driver_VO(camera_model=gums_calibrated, scene_path=scene_path_omni, scene_path_vo_results=results,
                    scene_img_filename_template=template, depth_filename_template=None, num_scene_images=num_scene_images,
                    visualize_VO=args.visualize_VO, use_multithreads_for_VO=args.use_multithreads_for_VO,
                    step_for_scene_images=args.step, first_image_index=args.first_image_index,
                    last_image_index=args.last_image_index, thread_name="%s-%s" % (scene_name, "SOS"),
                    frame_window=None if args.frame_window < 0 else args.frame_window,
                    detection_method=args.detection_method, cross_check=cross_check, **gated)
    print("GOODBYE!")
    return out


if __name__ == "__main__":
    main_sos_vo()
