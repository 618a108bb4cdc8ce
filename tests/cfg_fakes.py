"""What the CPU tests of the configuration layers (test_*_cfg.py) share: sosvo_batch_cfg / sosvo_rgbd_batch_cfg values for the
workspace queries, and stand-ins for the device side of run_VO's engine choice -- a recorder in place of an engine, a tracker
with the reference's settings and no camera, a rig and an RGB-D camera that hold matchers and no device."""
import numpy as np
import pytest

from vo_single_camera_sos_amd import _lib
from vo_single_camera_sos_amd.omnistereo.camera_models import FeatureMatcher


def lib_or_skip():
    try:
        return _lib.load()
    except Exception as e:  # noqa: BLE001 -- the library is not built on this machine
        pytest.skip("libsosvo.so does not load here: %s" % e)


def cfg(flags=0, detector=0, n_pairs=4, kp_cap=1024):
    c = _lib.BatchCfg()
    c.n_pairs, c.H, c.W, c.rows, c.cols, c.nmask = n_pairs, 480, 640, 300, 1200, 12
    c.kp_cap, c.frame_cap, c.median_ksize, c.max_corners, c.edge = kp_cap, 2048, 11, 1000, 31
    c.detector, c.ransac_flags = detector, flags
    return c


def rgbd_cfg(flags=0, method="GFT", n_pairs=4, kp_cap=1088):
    c = _lib.RgbdBatchCfg()
    c.n_pairs, c.rows, c.cols, c.kp_cap, c.frame_cap, c.max_corners, c.edge = n_pairs, 480, 640, kp_cap, kp_cap, 1000, 31
    c.flags = _lib.FLAG_EPNP | _lib.rgbd_detector_flags(method) | flags
    return c


class Engine(object):
    """Records what an engine is built with and how often it is reset."""

    def __init__(self, *args, **kwargs):
        self.args, self.kwargs, self.resets = args, kwargs, 0
        self._error, self._live = None, 0

    def reset(self):
        self.resets += 1

    def reset_counters(self):
        self.resets += 1


class Matcher(object):
    """A matcher that only names its detector (no matcher option is set on it)."""

    def __init__(self, method):
        self.feature_detection_method = method


def tracker(rgbd, method=None):
    """A TrackerSE3 with the reference's settings; method: its detection method, None for the default."""
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import TrackerSE3
    t = TrackerSE3.__new__(TrackerSE3)
    t.set_global_parameters_for_tracking()
    if method is not None:
        t.detection_method = method
    t.num_features_detection_for_static_stereo = 1000
    t.max_horizontal_diff_f2f_matches = 37.5
    if not rgbd:
        t.cam_rotations = np.array([np.identity(3), np.identity(3)])
        t.cam_offsets = np.array([[0.0, 0.0, 10.0], [0.0, 0.0, -10.0]])
    return t


class _Pano(object):
    cols, rows, pixel_size, cyl_height_max = 1200, 300, 0.01, 1.0


class _Mirror(object):
    def __init__(self, z):
        self.F = np.array([[0.0], [0.0], [z], [1.0]])
        self.panorama = _Pano()


class Rig(object):
    """stereo_matcher: the static-stereo matcher, by default a FeatureMatcher like the one for motion."""
    units = "mm"

    def __init__(self, stereo_matcher=None):
        self.top_model, self.bot_model = _Mirror(10.0), _Mirror(-10.0)
        self.current_omni_img = None
        self.feature_matcher_for_static_stereo = stereo_matcher or FeatureMatcher("GFT", "BF", 1)
        self.feature_matcher_for_motion = FeatureMatcher("GFT", "BF", 1)
        self.model = object()

    def _device_model(self):
        return self.model

    def _context(self):
        return "ctx"


def rgbd_cam(matcher=None):
    from vo_single_camera_sos_amd.omnistereo.camera_models import RGBDCamModel
    cam = RGBDCamModel()
    cam.feature_matcher_for_motion = matcher or FeatureMatcher("GFT", "BF", 1)
    cam._context = lambda: "ctx"
    return cam


class ScriptedRig(object):
    """A rig for run_VO's per-frame loop (frame_window 0) with ScriptedTracker and ScriptedFrame in place of TrackerStereoSE3
    and StereoPanoramicFrame: it only counts the images it is handed.  script: one entry per frame of the run,
    (T_frame_wrt_tracking_ref_frame, num_tracked_correspondences, inlier ratio, num_valid_keypoints, True or the failure
    message); the first frame is not tracked, only its num_valid_keypoints is read."""
    units = "mm"

    def __init__(self, script, T_Cest_wrt_Rgt=None):
        self.script, self.position, self.T_Cest_wrt_Rgt = list(script), -1, T_Cest_wrt_Rgt

    def set_current_omni_image(self, img, **kwargs):
        self.position += 1


class ScriptedFrame(object):
    def __init__(self, stereo_camera_model, frame_id, parent_id=-1):
        self.frame_id, self.parent_id = frame_id, parent_id
        self.T_frame_wrt_tracking_ref_frame = np.identity(4)
        self.num_valid_keypoints = stereo_camera_model.script[stereo_camera_model.position][3]


class ScriptedTracker(object):
    """What run_VO reads of a tracker; track_frame replays the rig's script entry of the current frame and chains the pose as
    TrackerStereoSE3 does."""

    def __init__(self, camera_model, show_3D_points=False, **kwargs):
        self.camera_model, self.number_of_cams = camera_model, 2
        self.T_C_wrt_S_init, self.T_C_curr_frame_wrt_S_est = np.identity(4), np.identity(4)
        self.num_tracked_correspondences, self.inlier_tracked_correspondences_ratio = 0, 0.
        self.T_Ckey_wrt_S_est_list = []

    def track_frame(self, reference_frame, current_frame):
        T, n, ratio, _, ok = self.camera_model.script[self.camera_model.position]
        if ok is not True:
            return False, ok
        self.num_tracked_correspondences, self.inlier_tracked_correspondences_ratio = n, ratio
        current_frame.T_frame_wrt_tracking_ref_frame = T
        self.T_C_curr_frame_wrt_S_est = self.T_Ckey_wrt_S_est_list[-1].dot(T)
        return True, "tracking used %d inlier point correspondences" % n
