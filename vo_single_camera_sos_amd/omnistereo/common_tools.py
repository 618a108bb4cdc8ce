"""Host-side mirror of the helpers of omnistereo/common_tools.py that the VO loop uses: unit conversion, the
TUM pose-file reader / writer, path creation, attribute copying (keyframes).  Pinned by tests/golden/transforms.npz."""
import errno
import os

import numpy as np

from . import transformations as tr

_UNIT_IN_M = {"mm": 0.001, "cm": 0.01, "m": 1.0}
_EXACT = {("cm", "mm"): 10.0, ("cm", "m"): 0.01, ("mm", "cm"): 0.1, ("mm", "m"): 0.001, ("m", "mm"): 1000.0,
          ("m", "cm"): 100.0}


def get_length_units_conversion_factor(input_units, output_units):
    """common_tools.py:580-597 (the same literal factors; unknown pairs -> 1.0)."""
    return _EXACT.get((input_units, output_units), 1.0)


def make_sure_path_exists(path):
    """common_tools.py:86-92"""
    try:
        os.makedirs(path)
    except OSError as exception:
        if exception.errno != errno.EEXIST:
            raise


def str2bool(v):
    return str(v).lower() in ("yes", "true", "t", "1")


def add_f2f_tracker_arguments(parser):
    """The demos' flags for where the frame-to-frame correspondences come from (run_VO's f2f_tracker / lk)."""
    parser.add_argument("--f2f_tracker", default=None, choices=("match", "lk"),
                        help="frame-to-frame correspondences from the descriptor matcher (match, the default) or by pyramidal "
                             "Lucas-Kanade tracking of the reference frame's stereo points (lk), on the GPU")
    parser.add_argument("--lk_half", default=None, type=int, help="with --f2f_tracker lk: the window half-size 2 .. 10; default: 10")
    parser.add_argument("--lk_levels", default=None, type=int, help="with --f2f_tracker lk: pyramid levels 1 .. 4; default: 3")
    parser.add_argument("--lk_max_iter", default=None, type=int, help="with --f2f_tracker lk: iterations per level 1 .. 30; default: 30")
    parser.add_argument("--lk_fb_max", default=None, type=float,
                        help="with --f2f_tracker lk: forward-backward check, the largest round-trip error in pixels; default: no check")


def f2f_tracker_arguments(args):
    """The parsed flags of add_f2f_tracker_arguments -> run_VO's f2f_tracker= / lk= (lk None: the tracker's defaults)."""
    lk = {name: getattr(args, "lk_" + name) for name in ("half", "levels", "max_iter", "fb_max") if getattr(args, "lk_" + name) is not None}
    return dict(f2f_tracker=args.f2f_tracker, lk=lk or None)


def add_stereo_refine_arguments(parser):
    """The demos' flags for the sub-pixel static stereo (run_VO's stereo_refine / stereo_lk)."""
    parser.add_argument("--stereo_refine", default=None, choices=("lk",),
                        help="lk: after the top / bottom matching the bottom keypoint of every matched pair is tracked from the top "
                             "panorama into the bottom one (one-level Lucas-Kanade from the matcher's partner), on the GPU; default: off")
    parser.add_argument("--stereo_lk_half", default=None, type=int, help="with --stereo_refine lk: the window half-size 2 .. 10; default: 4")
    parser.add_argument("--stereo_lk_max_shift", default=None, type=float,
                        help="with --stereo_refine lk: a tracked position further than this from the matcher's partner on either axis "
                             "is reverted, in pixels; default: the window half-size")


def stereo_refine_arguments(args):
    """The parsed flags of add_stereo_refine_arguments -> run_VO's stereo_refine= / stereo_lk= (None: the defaults)."""
    o = {name: getattr(args, "stereo_lk_" + name) for name in ("half", "max_shift") if getattr(args, "stereo_lk_" + name) is not None}
    return dict(stereo_refine=args.stereo_refine, stereo_lk=o or None)


def copy_only_attributes(objfrom, objto, exclude_names=()):
    """common_tools.py:154-159: every non-dunder member of objfrom is set on objto."""
    for n in dir(objfrom):
        if "__" in n or n in exclude_names:
            continue
        v = getattr(objfrom, n)
        if callable(v) and hasattr(type(objto), n):
            continue  # methods come with the class
        setattr(objto, n, v)


def save_as_tum_poses_to_file(output_tum_filename, poses_7_list, input_units, input_format, output_units="m"):
    """common_tools.py:599-621: one line per pose, the line number as time stamp; input_format "tr" =
    [qw, qx, qy, qz, tx, ty, tz], "tum" = [tx, ty, tz, qx, qy, qz, qw]."""
    k = get_length_units_conversion_factor(input_units, output_units)
    with open(output_tum_filename, "w") as f:
        for stamp, pose in enumerate(poses_7_list):
            if "tr" in input_format.lower():
                qw, qi, qj, qk = pose[:4]
                tx, ty, tz = pose[4:]
            else:
                tx, ty, tz = pose[:3]
                qi, qj, qk, qw = pose[3:]
            print("%d %.9f %.9f %.9f %.9f %.9f %.9f %.9f" % (stamp, k * tx, k * ty, k * tz, qi, qj, qk, qw), file=f)


def get_poses_from_file(poses_filename, input_units="m", output_working_units="m", indices=None, pose_format="tum",
                        zero_up_wrt_origin=False, initial_T=None, delimiter=None):
    """common_tools.py:623-736.  pose_format "tum": stamp tx ty tz qx qy qz qw per line, blank-separated; "povray":
    tx, ty, tz, rot_x, rot_y, rot_z per line, comma-separated, angles in degrees about the static x, y, z axes in that
    order ('#' comments in both) -> (list of [tx, ty, tz, qx, qy, qz, qw] in output units, list of 4x4 matrices).
    With zero_up_wrt_origin the first valid pose becomes the identity (every pose is pre-multiplied by its inverse,
    `initial_T` post-multiplied); rows holding NaN give NaN entries."""
    fmt = pose_format.lower()
    if fmt not in ("tum", "povray"):
        raise ValueError("pose_format %r: 'tum' or 'povray'" % pose_format)
    if delimiter is None and fmt == "povray":
        delimiter = ","
    grid = np.loadtxt(poses_filename, delimiter=delimiter if delimiter and delimiter != " " else None,
                      usecols=tuple(range(8 if fmt == "tum" else 6)), comments="#", ndmin=2)
    if len(grid) == 0:
        raise ValueError("no poses in %s" % poses_filename)
    k = get_length_units_conversion_factor(input_units, output_working_units)
    if indices is None or len(indices) == 0:
        indices = range(len(grid))
    n = len(indices)
    poses7, mats = n * [None], n * [None]
    T_offset, have_offset = tr.identity_matrix(), False
    apply_init = initial_T is not None
    if initial_T is None:
        initial_T = tr.identity_matrix()
    for pose_number in indices:
        row = grid[pose_number]
        if np.any(np.isnan(row)):
            entry = 7 * [np.nan]
        elif fmt == "povray":
            qw, qx, qy, qz = tr.quaternion_from_euler(np.deg2rad(float(row[3])), np.deg2rad(float(row[4])),
                                                      np.deg2rad(float(row[5])), "sxyz")
            entry = [k * float(row[0]), k * float(row[1]), k * float(row[2]), qx, qy, qz, qw]
        else:
            entry = [k * float(row[1]), k * float(row[2]), k * float(row[3]), float(row[4]), float(row[5]), float(row[6]),
                     float(row[7])]
        poses7[pose_number] = entry
        T = tr.transform44_from_TUM_entry(entry, scale_translation=1.0, has_timestamp=False)
        mats[pose_number] = T
        if (zero_up_wrt_origin and not np.any(np.isnan(T))) or apply_init:
            if zero_up_wrt_origin and not have_offset:
                T_offset = tr.inverse_matrix(T)
                have_offset = True
            T = tr.concatenate_matrices(T_offset, T, initial_T)
            mats[pose_number] = T
            e = 7 * [0.0]
            if np.any(np.isnan(T)):
                e[3:] = 4 * [np.nan]
            else:
                e[6], e[3], e[4], e[5] = tr.quaternion_from_matrix(T, isprecise=False)
            e[:3] = tr.translation_from_matrix(T)
            poses7[pose_number] = e
    return poses7, mats
