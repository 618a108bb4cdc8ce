#!/usr/bin/env python3
"""Live frame-to-frame visual odometry on the single-camera omnistereo (SOS) rig -- the entry point and arguments of the
reference's demo_vo_sos_live.py (:47-109), running the hot path on the MI355X through libsosvo.

    python demo_vo_sos_live.py <results_path> --calibrated_gums_file gums-calibrated.json [--frames 'dir/image-*.png']

The reference opens camera 0 through its OpenCV wrapper (WebcamLive, a GUI class that is out of scope here) and hands
a camera thread to driver_VO_live.  This entry point wraps the SAME driver over any frame source: by default
`--frames` names recorded omni frames that are replayed as a camera would deliver them (ImageSequenceCam); a host
application passes its own object with get_single_frame() to main_sos_vo_live(frame_source=...).
Results go to <results_path>/results-omni/ (estimated_frame_poses_TUM.txt, keyframe_ids.txt, printed_messages.log)."""
import os.path as osp
import sys
from argparse import ArgumentParser

ROOT = osp.dirname(osp.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    from vo_single_camera_sos_amd.omnistereo.common_tools import add_f2f_tracker_arguments, add_stereo_refine_arguments, str2bool
    parser = ArgumentParser(description="Live demo of frame-to-frame visual odometry for the Single-camera SOS rig.")
    parser.register("type", "bool", str2bool)
    parser.add_argument("results_path", nargs=1, help="The path where the results will be saved into.")
    parser.add_argument("--calibrated_gums_file", default="gums-calibrated.json", type=str,
                        help="Complete path and name of the calibrated GUMS file (JSON)")
    parser.add_argument("--visualize_VO", default=False, type="bool",
                        help="(Optional) 3-D visualisation of the trajectory: not built, must stay false")
    parser.add_argument("--frames", default=None, type=str,
                        help="glob of recorded omni frames replayed as the camera (needed unless a frame_source is passed in)")
    parser.add_argument("--lockstep", default=True, type="bool",
                        help="deliver every frame exactly once (reproducible runs); false = newest frame wins, as a camera")
    parser.add_argument("--use_multithreads_for_VO", default=True, type="bool")
    parser.add_argument("--frame_window", default=-1, type=int,
                        help="frames per batched front-end pass (-1 = 1 for a live source; 0 = the per-frame mirror path)")
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


def main_sos_vo_live(argv=None, frame_source=None):
    from vo_single_camera_sos_amd.omnistereo.common_tools import f2f_tracker_arguments, make_sure_path_exists, stereo_refine_arguments
    parser = build_parser()
    args = parser.parse_args(argv)

    from vo_single_camera_sos_amd.omnistereo.gum import load_gums_json
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import driver_VO_live
    from vo_single_camera_sos_amd.omnistereo.webcam_live import FrameSourceThread, ImageSequenceCam
    scene_path = osp.realpath(osp.expanduser(args.results_path[0]))
    results = osp.join(scene_path, "results-omni")
    make_sure_path_exists(results)
    if frame_source is None:
        if not args.frames:
            parser.error("no camera wrapper is built in: give --frames <glob> or call main_sos_vo_live(frame_source=...)")
        frame_source = ImageSequenceCam(osp.expanduser(args.frames))
    cam_working_thread = FrameSourceThread(frame_source, lockstep=args.lockstep)
    gums_calibrated = load_gums_json(osp.realpath(osp.expanduser(args.calibrated_gums_file)))
    out = driver_VO_live(gums_calibrated, results, cam_working_thread, visualize_VO=args.visualize_VO,
                         use_multithreads_for_VO=args.use_multithreads_for_VO, thread_name="LIVE-SOS",
                         frame_window=None if args.frame_window < 0 else args.frame_window,
                         cross_check=None if args.cross_check is None else (True if args.cross_check == "both" else args.cross_check),
                         gated_matching=None if args.gated_matching is None else (True if args.gated_matching == "both" else args.gated_matching),
                         gated_max_distance=args.gated_max_distance,
                         ratio_test=None if args.ratio_test is None else (True if args.ratio_test == "both" else args.ratio_test),
                         ratio=args.ratio,
                         subpix_refine=True if args.subpix_refine else None, subpix_half=args.subpix_half, **f2f_tracker_arguments(args),
                         **stereo_refine_arguments(args), cyclic_columns="seam_free" if args.seam_free else (True if args.cyclic_columns else None))
    print("GOODBYE!")
    return out


if __name__ == "__main__":
    main_sos_vo_live()
