"""CPU: the detector selection of the batch and sequence entry points -- sosvo_batch_cfg.detector (the former `reserved`
field) and bits 8-9 of sosvo_rgbd_batch_cfg.flags -- keeps both structs' layout, never reaches the solver flags, grows the
workspace only for ORB, and sequence_engine_for / rgbd_sequence_engine_for build an engine per method (device calls
replaced by a recorder)."""
import ctypes

import numpy as np
import pytest

from vo_single_camera_sos_amd import _lib
from vo_single_camera_sos_amd.frontend import default_kp_cap, mirror_kp_cap
from vo_single_camera_sos_amd.pipeline import rgbd_kp_cap, rgbd_solver_flags

METHODS = ("GFT", "ORB", "FAST", "AGAST")


def test_batch_cfg_layout_is_unchanged():
    assert ctypes.sizeof(_lib.BatchCfg) == 104
    assert _lib.BatchCfg.detector.offset == 100 and _lib.BatchCfg.ransac_flags.offset == 96
    assert [f[0] for f in _lib.BatchCfg._fields_][-1] == "detector"
    assert ctypes.sizeof(_lib.RgbdBatchCfg) == 104 and _lib.RgbdBatchCfg.flags.offset == 44
    assert _lib.DETECTORS == {"GFT": 0, "ORB": 1, "FAST": 2, "AGAST": 3}


def test_header_declares_the_enum_and_the_flag_bits():
    text = open(_lib.HEADER_PATH).read()
    assert "SOSVO_DETECTOR_GFT = 0, SOSVO_DETECTOR_ORB = 1, SOSVO_DETECTOR_FAST = 2, SOSVO_DETECTOR_AGAST = 3" in text
    assert "#define SOSVO_RGBD_DETECTOR(d) ((d) << SOSVO_RGBD_DETECTOR_SHIFT)" in text
    assert "#define SOSVO_RGBD_DETECTOR_SHIFT 8" in text
    assert "int32_t detector;" in text and "int32_t reserved;        /* 0 */" not in text


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("solver", ["EPNP", "KNEIP", "GAO", "GP3P", "TWOPT"])
def test_rgbd_detector_bits_round_trip_and_stay_out_of_the_solver_flags(method, solver):
    s = rgbd_solver_flags(solver)
    flags = s | _lib.rgbd_detector_flags(method)
    assert _lib.rgbd_flags_detector(flags) == _lib.DETECTORS[method]
    solver_bits = _lib.FLAG_EPNP | _lib.FLAG_GP3P | _lib.FLAG_TWOPT   # what the C code passes to sosvo_ransac_abs_pose
    assert flags & solver_bits == s and not (_lib.RGBD_DETECTOR_MASK & solver_bits)
    assert _lib.rgbd_detector_flags(method.lower()) == _lib.rgbd_detector_flags(method)


def test_unknown_detectors_raise():
    for bad in ("SIFT", "SURF", "BRISK", "KAZE", ""):
        with pytest.raises(NotImplementedError):
            _lib.detector_code(bad)


def test_capacity_rules():
    assert default_kp_cap("GFT", 1000) == 1024 and default_kp_cap("ORB", 1000) == 1280 and default_kp_cap("FAST", 10) == 2048
    assert mirror_kp_cap("GFT", 1000) == 1024 and mirror_kp_cap("ORB", 1000) == 1280 and mirror_kp_cap("AGAST", 1000) == 1024
    assert rgbd_kp_cap("GFT", 1000) == 1088 and rgbd_kp_cap("GFT", 2000) == 2048     # unchanged GFT rule
    assert rgbd_kp_cap("ORB", 1000) == 1280 and rgbd_kp_cap("ORB", 5000) == 2048 and rgbd_kp_cap("FAST", 50) == 4096


def _lib_or_skip():
    try:
        return _lib.load()
    except Exception as e:  # noqa: BLE001 -- the library is not built on this machine
        pytest.skip("libsosvo.so does not load here: %s" % e)


def _cfg(detector, kp_cap=1024):
    c = _lib.BatchCfg()
    c.n_pairs, c.H, c.W, c.rows, c.cols, c.nmask = 4, 480, 640, 300, 1200, 12
    c.kp_cap, c.frame_cap, c.median_ksize, c.max_corners, c.edge = kp_cap, 2048, 11, 1000, 31
    c.detector = detector
    return c


def _rgbd_cfg(method, kp_cap=1088):
    c = _lib.RgbdBatchCfg()
    c.n_pairs, c.rows, c.cols, c.kp_cap, c.frame_cap, c.max_corners, c.edge = 4, 480, 640, kp_cap, kp_cap, 1000, 31
    c.flags = _lib.FLAG_EPNP | _lib.rgbd_detector_flags(method)
    return c


def test_workspace_sizes():
    lib = _lib_or_skip()
    ws = lambda c: lib.sosvo_frame_pair_batch_workspace(ctypes.byref(c))  # noqa: E731
    seq = lambda c: lib.sosvo_sequence_workspace(ctypes.byref(c), 8, 17)  # noqa: E731
    g = _cfg(0)
    # GFT: the size a zero `reserved` field gave before (the layout of the GFT buffers is untouched)
    assert ws(g) > 0 and ws(_cfg(2)) == ws(g) == ws(_cfg(3)) and seq(_cfg(2)) == seq(g) > 0
    assert ws(_cfg(1)) > ws(g) and seq(_cfg(1)) > seq(g)
    assert lib.sosvo_frame_pair_batch_streams_workspace(ctypes.byref(_cfg(1)), 2) > \
        lib.sosvo_frame_pair_batch_streams_workspace(ctypes.byref(g), 2) > 0
    for bad in (_cfg(4), _cfg(-1), _cfg(1, kp_cap=2112)):
        assert ws(bad) == 0 and seq(bad) == 0
    assert ws(_cfg(2, kp_cap=4096)) > 0
    rws = lambda c: lib.sosvo_rgbd_pair_batch_workspace(ctypes.byref(c))  # noqa: E731
    rseq = lambda c: lib.sosvo_rgbd_sequence_workspace(ctypes.byref(c), 8, 17)  # noqa: E731
    rg = _rgbd_cfg("GFT")
    assert rws(rg) > 0 and rws(_rgbd_cfg("FAST")) == rws(rg) == rws(_rgbd_cfg("AGAST")) and rseq(_rgbd_cfg("FAST")) == rseq(rg)
    assert rws(_rgbd_cfg("ORB")) > rws(rg) and rseq(_rgbd_cfg("ORB")) > rseq(rg)
    assert rws(_rgbd_cfg("ORB", kp_cap=2112)) == 0 and rseq(_rgbd_cfg("ORB", kp_cap=2112)) == 0
    # the solver bits alone do not change the size
    c = _rgbd_cfg("GFT")
    c.flags = _lib.FLAG_GP3P
    assert rws(c) == rws(rg)


# ---- engine choice (device calls replaced by a recorder) ---------------------------------------------------------------
class _Engine(object):
    def __init__(self, *args, **kwargs):
        self.args, self.kwargs, self.resets = args, kwargs, 0

    def reset(self):
        self.resets += 1


class _Matcher(object):
    def __init__(self, method):
        self.feature_detection_method = method


def _tracker(method, rgbd):
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import TrackerSE3
    t = TrackerSE3.__new__(TrackerSE3)
    t.set_global_parameters_for_tracking()
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


class _Rig(object):
    units = "mm"

    def __init__(self, method="GFT"):
        self.top_model, self.bot_model = _Mirror(10.0), _Mirror(-10.0)
        self.current_omni_img = None
        self.feature_matcher_for_static_stereo = _Matcher(method)
        self.model = object()

    def _device_model(self):
        return self.model

    def _context(self):
        return "ctx"


class _Cam(object):
    fx = fy = 525.0
    center_x, center_y, focal_length_m, depth_is_Z = 319.5, 239.5, 1e-3, True

    def __init__(self, method="GFT"):
        self.feature_matcher_for_motion = _Matcher(method)

    def _context(self):
        return "ctx"


def test_sequence_engine_for_builds_one_engine_per_method(monkeypatch):
    from vo_single_camera_sos_amd import pipeline
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    monkeypatch.setattr(pipeline, "SequenceEngine", _Engine)
    rig = _Rig()
    engines = {}
    for method in METHODS:
        t = _tracker(method, rgbd=False)
        rig.feature_matcher_for_static_stereo = _Matcher(method)
        eng = pet.sequence_engine_for(t, rig, np.zeros((4, 4, 3), np.uint8), 32)
        assert isinstance(eng, _Engine) and eng.kwargs["detection_method"] == method, method
        assert eng.kwargs["kp_cap"] == mirror_kp_cap(method, 1000)
        engines[method] = eng
    keys = list(rig._sequence_engines)
    assert len(keys) == 1 and keys[0][0] == "AGAST"          # one engine per rig: the method is part of the key
    again = pet.sequence_engine_for(_tracker("AGAST", False), rig, None, 32)
    assert again is engines["AGAST"] and again.resets == 1
    assert pet.sequence_engine_for(_tracker("ORB", False), rig, None, 32) is not engines["ORB"]   # (AGAST's was dropped)
    # no batched counterpart: another detector, or frames that would detect with another method than the tracker
    assert pet.sequence_engine_for(_tracker("SIFT", False), rig, None, 32) is None
    rig.feature_matcher_for_static_stereo = _Matcher("GFT")
    assert pet.sequence_engine_for(_tracker("ORB", False), rig, None, 32) is None


def test_rgbd_sequence_engine_for_builds_one_engine_per_method(monkeypatch):
    from vo_single_camera_sos_amd import pipeline
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    monkeypatch.setattr(pipeline, "RGBDSequenceEngine", _Engine)
    cam = _Cam()
    img = np.zeros((480, 640, 3), np.uint8)
    seen = []
    for method in METHODS:
        cam.feature_matcher_for_motion = _Matcher(method)
        eng = pet.rgbd_sequence_engine_for(_tracker(method, rgbd=True), cam, img, 8)
        assert isinstance(eng, _Engine) and eng.kwargs["detection_method"] == method
        seen.append(eng)
        assert list(cam._sequence_engines)[0][0] == method
    assert len(set(map(id, seen))) == 4
    assert pet.rgbd_sequence_engine_for(_tracker("SURF", rgbd=True), cam, img, 8) is None


def test_set_detection_method_updates_the_tracker_and_its_matchers():
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    t = _tracker("GFT", rgbd=False)
    t.camera_model = _Rig()
    t.camera_model.feature_matcher_for_motion = _Matcher("GFT")
    pet.set_detection_method(t, None)
    assert t.detection_method == "GFT"
    pet.set_detection_method(t, "orb")
    assert t.detection_method == "ORB"
    assert t.camera_model.feature_matcher_for_static_stereo.feature_detection_method == "ORB"
    assert t.camera_model.feature_matcher_for_motion.feature_detection_method == "ORB"
