"""CPU: the detector selection of the batch and sequence entry points -- sosvo_batch_cfg.detector (the former `reserved`
field) and bits 8-9 of sosvo_rgbd_batch_cfg.flags -- keeps both structs' layout, never reaches the solver flags, grows the
workspace only for ORB, and sequence_engine_for / rgbd_sequence_engine_for build an engine per method (device calls
replaced by a recorder)."""
import ctypes
import itertools

import numpy as np
import pytest

from cfg_fakes import Engine, Matcher, Rig, cfg, lib_or_skip, rgbd_cam, rgbd_cfg, tracker
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


def test_workspace_sizes():
    lib = lib_or_skip()
    ws = lambda c: lib.sosvo_frame_pair_batch_workspace(ctypes.byref(c))  # noqa: E731
    seq = lambda c: lib.sosvo_sequence_workspace(ctypes.byref(c), 8, 17)  # noqa: E731
    g = cfg(detector=0)
    # GFT: the size a zero `reserved` field gave before (the layout of the GFT buffers is untouched)
    assert ws(g) > 0 and ws(cfg(detector=2)) == ws(g) == ws(cfg(detector=3)) and seq(cfg(detector=2)) == seq(g) > 0
    assert ws(cfg(detector=1)) > ws(g) and seq(cfg(detector=1)) > seq(g)
    assert lib.sosvo_frame_pair_batch_streams_workspace(ctypes.byref(cfg(detector=1)), 2) > \
        lib.sosvo_frame_pair_batch_streams_workspace(ctypes.byref(g), 2) > 0
    for bad in (cfg(detector=4), cfg(detector=-1), cfg(detector=1, kp_cap=2112)):
        assert ws(bad) == 0 and seq(bad) == 0
    assert ws(cfg(detector=2, kp_cap=4096)) > 0
    rws = lambda c: lib.sosvo_rgbd_pair_batch_workspace(ctypes.byref(c))  # noqa: E731
    rseq = lambda c: lib.sosvo_rgbd_sequence_workspace(ctypes.byref(c), 8, 17)  # noqa: E731
    rg = rgbd_cfg(method="GFT")
    assert rws(rg) > 0 and rws(rgbd_cfg(method="FAST")) == rws(rg) == rws(rgbd_cfg(method="AGAST")) and rseq(rgbd_cfg(method="FAST")) == rseq(rg)
    assert rws(rgbd_cfg(method="ORB")) > rws(rg) and rseq(rgbd_cfg(method="ORB")) > rseq(rg)
    assert rws(rgbd_cfg(method="ORB", kp_cap=2112)) == 0 and rseq(rgbd_cfg(method="ORB", kp_cap=2112)) == 0
    # the solver bits alone do not change the size
    c = rgbd_cfg(method="GFT")
    c.flags = _lib.FLAG_GP3P
    assert rws(c) == rws(rg)


# workspace sizes of the build before the carve functions of pipeline.hip were merged (one per engine family): the layout
# inside a workspace is private, its size is what a host allocates
# (detector, median_ksize, n_pairs): (pair batch, 2 streams, 3 streams, sequence 8 / 17, sequence 32 / 65); _cfg otherwise
_OMNI_SIZES = {
    (0, 7, 4): (35383040, 35386880, 35390720, 38184704, 148204032),
    (0, 7, 64): (566076160, 566078464, 566083072, 56137472, 166156800),
    (0, 11, 4): (18103040, 18106880, 18110720, 20904704, 79084032),
    (0, 11, 64): (289596160, 289598464, 289603072, 38857472, 97036800),
    (1, 7, 4): (48232448, 57153536, 66074624, 51034112, 172849920),
    (1, 7, 64): (637907968, 646827520, 655749376, 68986880, 190802688),
    (1, 11, 4): (30952448, 39873536, 48794624, 33754112, 103729920),
    (1, 11, 64): (361427968, 370347520, 379269376, 51706880, 121682688),
    (2, 7, 4): (35383040, 35386880, 35390720, 38184704, 148204032),
    (2, 7, 64): (566076160, 566078464, 566083072, 56137472, 166156800),
    (2, 11, 4): (18103040, 18106880, 18110720, 20904704, 79084032),
    (2, 11, 64): (289596160, 289598464, 289603072, 38857472, 97036800),
    (3, 7, 4): (35383040, 35386880, 35390720, 38184704, 148204032),
    (3, 7, 64): (566076160, 566078464, 566083072, 56137472, 166156800),
    (3, 11, 4): (18103040, 18106880, 18110720, 20904704, 79084032),
    (3, 11, 64): (289596160, 289598464, 289603072, 38857472, 97036800),
}
# (method, n_pairs): (pair batch, sequence 8 / 17, sequence 32 / 65); _rgbd_cfg otherwise
_RGBD_SIZES = {
    ("GFT", 4): (3875584, 4737280, 17750528),
    ("GFT", 64): (61968640, 9253888, 22267136),
    ("ORB", 4): (7852032, 8713728, 22249216),
    ("ORB", 64): (68556288, 13230336, 26765824),
    ("FAST", 4): (3875584, 4737280, 17750528),
    ("FAST", 64): (61968640, 9253888, 22267136),
    ("AGAST", 4): (3875584, 4737280, 17750528),
    ("AGAST", 64): (61968640, 9253888, 22267136),
}


def test_workspace_sizes_are_those_of_the_four_layout_build():
    lib = lib_or_skip()
    for (det, median, n_pairs), want in _OMNI_SIZES.items():
        c = cfg(detector=det)
        c.median_ksize, c.n_pairs = median, n_pairs
        r = ctypes.byref(c)
        got = (lib.sosvo_frame_pair_batch_workspace(r), lib.sosvo_frame_pair_batch_streams_workspace(r, 2),
               lib.sosvo_frame_pair_batch_streams_workspace(r, 3), lib.sosvo_sequence_workspace(r, 8, 17),
               lib.sosvo_sequence_workspace(r, 32, 65))
        assert got == want, (det, median, n_pairs)
    for (method, n_pairs), want in _RGBD_SIZES.items():
        c = rgbd_cfg(method=method)
        c.n_pairs = n_pairs
        r = ctypes.byref(c)
        got = (lib.sosvo_rgbd_pair_batch_workspace(r), lib.sosvo_rgbd_sequence_workspace(r, 8, 17),
               lib.sosvo_rgbd_sequence_workspace(r, 32, 65))
        assert got == want, (method, n_pairs)


def test_a_pair_batch_is_the_sequence_layout_with_two_frames_per_pair():
    """window = slots = 2 * n_pairs: the same set of buffers, so the same size (every slice is rounded on its own, so the
    order of the slices does not enter)."""
    lib = lib_or_skip()
    n = 0
    for B, det, cap, nmask, median, (rows, cols) in itertools.product(
            (1, 3, 64, 256), range(4), (512, 1024, 2048), (1, 12, 32), (0, 3, 7, 11), ((146, 1440), (300, 1200))):
        c = cfg(detector=det, kp_cap=cap)
        c.n_pairs, c.nmask, c.median_ksize, c.rows, c.cols = B, nmask, median, rows, cols
        r = ctypes.byref(c)
        assert lib.sosvo_frame_pair_batch_workspace(r) == lib.sosvo_sequence_workspace(r, 2 * B, 2 * B) > 0, \
            (B, det, cap, nmask, median, rows, cols)
        n += 1
    for B, method, cap in itertools.product((1, 3, 64, 256), METHODS, (512, 1088, 2048)):
        c = rgbd_cfg(method=method, kp_cap=cap)
        c.n_pairs = B
        r = ctypes.byref(c)
        assert lib.sosvo_rgbd_pair_batch_workspace(r) == lib.sosvo_rgbd_sequence_workspace(r, 2 * B, 2 * B) > 0, (B, method, cap)
        n += 1
    assert n == 1152 + 48


def _fields(c):
    return {name: getattr(c, name) for name, _ in c._fields_}


def test_batch_cfg_builder_fills_every_field():
    from types import SimpleNamespace
    from vo_single_camera_sos_amd.pipeline import batch_cfg
    model = SimpleNamespace(H=480, W=640, rows=146, cols=1440, nmask=24)
    kw = dict(num_of_features=700, kp_cap=None, frame_cap=1536, median_win_size=5, quality=0.02, min_distance=7.5, edge=29,
              thr=None, max_iter=333, adaptive=True, lm_iter=17, ransac_solver="gp3p", detection_method="orb")
    c = batch_cfg(model, 6, seed=12345678901, **kw)
    assert _fields(c) == dict(
        n_pairs=6, H=480, W=640, rows=146, cols=1440, nmask=24, kp_cap=896, frame_cap=1536, median_ksize=5, max_corners=700,
        edge=29, ransac_max_iter=333, ransac_adaptive=1, lm_max_iter=17, quality=0.02, min_distance=7.5,
        ransac_threshold=0.003805301908254455, seed=12345678901, cos_a=0.9998477101325989, sin_a=-0.017452405765652657,
        ransac_flags=4, detector=1)
    assert set(_fields(c)) == {name for name, _ in _lib.BatchCfg._fields_} and len(_fields(c)) == 22
    # an explicit capacity and threshold, any solver but GP3P is P3P, adaptive off
    d = batch_cfg(model, 6, seed=0, **dict(kw, kp_cap=640, thr=0.25, adaptive=False, ransac_solver="P3P", detection_method="GFT"))
    assert (d.kp_cap, d.ransac_threshold, d.ransac_adaptive, d.ransac_flags, d.detector) == (640, 0.25, 0, 0, _lib.DETECTOR_GFT)
    # the pair batch and the sequence engine hand the library the same bytes once n_pairs and seed agree
    a, b = batch_cfg(model, 5, seed=9, **kw), batch_cfg(model, 32, seed=0, **kw)
    assert bytes(a) != bytes(b)
    a.n_pairs, a.seed = 32, 0
    assert bytes(a) == bytes(b)
    with pytest.raises(NotImplementedError):
        batch_cfg(model, 6, seed=0, **dict(kw, detection_method="SIFT"))


def test_rgbd_batch_cfg_builder_fills_every_field():
    from types import SimpleNamespace
    from vo_single_camera_sos_amd.pipeline import rgbd_batch_cfg
    cam = SimpleNamespace(pct_good_matches=0.75, f2f_max_hdiff=37.5)
    kw = dict(image_shape=(240, 320), num_of_features=900, kp_cap=None, frame_cap=None, median_win_size=3, quality=0.02,
              min_distance=7.5, edge=29, thr=0.125, max_iter=333, adaptive=False, lm_iter=17, pose_est_algorithm="TWOPT",
              detection_method="AGAST")
    c = rgbd_batch_cfg(cam, 6, seed=12345678901, **kw)
    assert _fields(c) == dict(
        n_pairs=6, rows=240, cols=320, kp_cap=4096, frame_cap=4096, median_ksize=3, max_corners=900, edge=29,
        ransac_max_iter=333, ransac_adaptive=0, lm_max_iter=17, flags=8 | 768,
        quality=0.02, min_distance=7.5, ransac_threshold=0.125, pct_good_matches=0.75, f2f_max_hdiff=37.5, seed=12345678901,
        cos_a=0.9998477101325989, sin_a=-0.017452405765652657)
    assert len(_fields(c)) == len(_lib.RgbdBatchCfg._fields_) == 20
    d = rgbd_batch_cfg(cam, 6, seed=0, **dict(kw, kp_cap=512, frame_cap=300, thr=None, adaptive=True, pose_est_algorithm="EPNP",
                                              detection_method="ORB"))
    assert (d.kp_cap, d.frame_cap, d.ransac_threshold, d.ransac_adaptive) == (512, 300, 0.003805301908254455, 1)
    assert d.flags == _lib.FLAG_EPNP | _lib.rgbd_detector_flags("ORB")
    assert rgbd_batch_cfg(cam, 6, seed=0, **dict(kw, detection_method="ORB")).kp_cap == 1152
    a, b = rgbd_batch_cfg(cam, 5, seed=9, **kw), rgbd_batch_cfg(cam, 32, seed=0, **kw)
    assert bytes(a) != bytes(b)
    a.n_pairs, a.seed = 32, 0
    assert bytes(a) == bytes(b)
    with pytest.raises(ValueError):
        rgbd_batch_cfg(cam, 6, seed=0, **dict(kw, pose_est_algorithm="DLS"))


# ---- engine choice (device calls replaced by a recorder) ---------------------------------------------------------------
def test_sequence_engine_for_builds_one_engine_per_method(monkeypatch):
    from vo_single_camera_sos_amd import pipeline
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    monkeypatch.setattr(pipeline, "SequenceEngine", Engine)
    rig = Rig(Matcher("GFT"))
    engines = {}
    for method in METHODS:
        t = tracker(False, method)
        rig.feature_matcher_for_static_stereo = Matcher(method)
        eng = pet.sequence_engine_for(t, rig, np.zeros((4, 4, 3), np.uint8), 32)
        assert isinstance(eng, Engine) and eng.kwargs["detection_method"] == method, method
        assert eng.kwargs["kp_cap"] == mirror_kp_cap(method, 1000)
        engines[method] = eng
    keys = list(rig._sequence_engines)
    assert len(keys) == 1 and keys[0][0] == "AGAST"          # one engine per rig: the method is part of the key
    again = pet.sequence_engine_for(tracker(False, "AGAST"), rig, None, 32)
    assert again is engines["AGAST"] and again.resets == 1
    assert pet.sequence_engine_for(tracker(False, "ORB"), rig, None, 32) is not engines["ORB"]   # (AGAST's was dropped)
    # no batched counterpart: another detector, or frames that would detect with another method than the tracker
    assert pet.sequence_engine_for(tracker(False, "SIFT"), rig, None, 32) is None
    rig.feature_matcher_for_static_stereo = Matcher("GFT")
    assert pet.sequence_engine_for(tracker(False, "ORB"), rig, None, 32) is None


def test_rgbd_sequence_engine_for_builds_one_engine_per_method(monkeypatch):
    from vo_single_camera_sos_amd import pipeline
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    monkeypatch.setattr(pipeline, "RGBDSequenceEngine", Engine)
    cam = rgbd_cam(Matcher("GFT"))
    img = np.zeros((480, 640, 3), np.uint8)
    seen = []
    for method in METHODS:
        cam.feature_matcher_for_motion = Matcher(method)
        eng = pet.rgbd_sequence_engine_for(tracker(True, method), cam, img, 8)
        assert isinstance(eng, Engine) and eng.kwargs["detection_method"] == method
        seen.append(eng)
        assert list(cam._sequence_engines)[0][0] == method
    assert len(set(map(id, seen))) == 4
    assert pet.rgbd_sequence_engine_for(tracker(True, "SURF"), cam, img, 8) is None


def test_set_detection_method_updates_the_tracker_and_its_matchers():
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    t = tracker(False, "GFT")
    t.camera_model = Rig(Matcher("GFT"))
    t.camera_model.feature_matcher_for_motion = Matcher("GFT")
    pet.set_detection_method(t, None)
    assert t.detection_method == "GFT"
    pet.set_detection_method(t, "orb")
    assert t.detection_method == "ORB"
    assert t.camera_model.feature_matcher_for_static_stereo.feature_detection_method == "ORB"
    assert t.camera_model.feature_matcher_for_motion.feature_detection_method == "ORB"
