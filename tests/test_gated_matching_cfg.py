"""CPU: the gated-matching switches -- SOSVO_FLAG_GATED_STEREO / _F2F and SOSVO_GATED_MAX_DIST in sosvo_batch_cfg.ransac_flags
and sosvo_rgbd_batch_cfg.flags, the stage entry sosvo_match_hamming_gated, FeatureMatcher(gated=True), run_VO's
gated_matching / gated_max_distance arguments -- keep both structs' layout, collide with no other bit, never reach the solver
flags, leave every workspace size alone (the gated search needs no buffer of its own), and are part of what keys the engine
kept with a camera model (device calls replaced by a recorder)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from cfg_fakes import Engine, Rig, cfg, lib_or_skip, rgbd_cam, rgbd_cfg, tracker
from vo_single_camera_sos_amd import _lib
from vo_single_camera_sos_amd.omnistereo.camera_models import FeatureMatcher
from vo_single_camera_sos_amd.pipeline import batch_cfg, rgbd_batch_cfg, rgbd_solver_flags

STEREO, F2F, SHIFT, MASK = 0x4000, 0x8000, 16, 0x1FF << 16
CC_STEREO, CC_F2F = 0x1000, 0x2000


def test_header_declares_the_macros_and_the_prototype():
    text = open(_lib.HEADER_PATH).read()
    for line in ("#define SOSVO_FLAG_GATED_STEREO 0x4000", "#define SOSVO_FLAG_GATED_F2F 0x8000",
                 "#define SOSVO_GATED_MAX_DIST_SHIFT 16", "#define SOSVO_GATED_MAX_DIST(d) ((d) << SOSVO_GATED_MAX_DIST_SHIFT)"):
        assert line in text, line
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert ("int32_t sosvo_match_hamming_gated(sosvo_ctx* ctx, const uint8_t* q_desc, const uint8_t* t_desc, const float* q_pos, "
            "const float* t_pos, const int32_t* nq, const int32_t* nt, const int32_t* q_slot, const int32_t* t_slot, "
            "int32_t nprob, int32_t n_forward, int32_t q_stride, int32_t t_stride, double min_dv, double max_du, "
            "int32_t max_distance, uint32_t* keys);") in flat
    assert (_lib.FLAG_GATED_STEREO, _lib.FLAG_GATED_F2F, _lib.GATED_MAX_DIST_SHIFT, _lib.GATED_MAX_DIST_MASK) == (STEREO, F2F, SHIFT, MASK)
    assert "sosvo_match_hamming_gated" in _lib.SIGNATURES and "sosvo_match_hamming_gated" in _lib.declared_functions()
    restype, argtypes = _lib.SIGNATURES["sosvo_match_hamming_gated"]
    assert restype is _lib.c_i32 and len(argtypes) == 17
    assert [a is _lib.c_i32 for a in argtypes] == [False] * 9 + [True] * 4 + [False] * 2 + [True, False]
    assert argtypes[13] is _lib.c_f64 and argtypes[14] is _lib.c_f64


def test_the_bits_overlap_no_other_flag_and_never_reach_the_solver():
    mine = STEREO | F2F | MASK
    others = (_lib.FLAG_CAM_ROT_IDENTITY | _lib.FLAG_EPNP | _lib.FLAG_GP3P | _lib.FLAG_TWOPT | _lib.RGBD_DETECTOR_MASK
              | _lib.FLAG_CROSS_CHECK_STEREO | _lib.FLAG_CROSS_CHECK_F2F)
    assert mine & others == 0 and STEREO & F2F == 0 and (STEREO | F2F) & MASK == 0 and mine < 2 ** 31
    assert MASK >> SHIFT >= 256                               # the field holds 1 .. 256
    assert _lib.gated_flags() == 0 and _lib.gated_flags(True, False) == STEREO and _lib.gated_flags(False, True) == F2F
    assert _lib.gated_flags(True, True, 80) == STEREO | F2F | (80 << SHIFT)
    assert _lib.gated_flags(True, True, 256) == STEREO | F2F | (256 << SHIFT)
    assert _lib.gated_flags(False, False, 80) == 0            # the cap belongs to the gated search
    for bad in (0, 257, -1, 64.5):
        with pytest.raises(ValueError, match="gated_max_distance"):
            _lib.gated_flags(True, False, bad)
    # what the C code hands sosvo_ransac_abs_pose: (ransac_flags & GP3P) | CAM_ROT_IDENTITY, (flags & (EPNP | GP3P | TWOPT))
    for s in (0, _lib.FLAG_GP3P):
        assert (s | mine) & _lib.FLAG_GP3P == s
    solver_bits = _lib.FLAG_EPNP | _lib.FLAG_GP3P | _lib.FLAG_TWOPT
    for solver in ("EPNP", "KNEIP", "GAO", "GP3P", "TWOPT"):
        for method in ("GFT", "ORB", "FAST", "AGAST"):
            flags = rgbd_solver_flags(solver) | _lib.rgbd_detector_flags(method) | F2F | MASK
            assert flags & solver_bits == rgbd_solver_flags(solver)
            assert _lib.rgbd_flags_detector(flags) == _lib.DETECTORS[method]


def test_the_cfg_layouts_are_unchanged():
    assert ctypes.sizeof(_lib.BatchCfg) == 104 and ctypes.sizeof(_lib.RgbdBatchCfg) == 104
    assert len(_lib.BatchCfg._fields_) == 22 and len(_lib.RgbdBatchCfg._fields_) == 20 and _lib.RgbdBatchCfg.flags.offset == 44


def test_the_cfg_builders_set_the_bits():
    from types import SimpleNamespace
    model = SimpleNamespace(H=480, W=640, rows=146, cols=1440, nmask=24)
    kw = dict(num_of_features=700, kp_cap=None, frame_cap=1536, median_win_size=5, quality=0.02, min_distance=7.5, edge=29,
              thr=None, max_iter=333, adaptive=True, lm_iter=17, detection_method="GFT")
    off = batch_cfg(model, 6, seed=3, ransac_solver="GP3P", **kw)
    assert off.ransac_flags == _lib.FLAG_GP3P
    assert bytes(batch_cfg(model, 6, seed=3, ransac_solver="GP3P", gated_stereo=False, gated_f2f=False, gated_max_distance=80, **kw)) \
        == bytes(off)
    for st, ff, cap in ((True, False, None), (False, True, 64), (True, True, 100)):
        c = batch_cfg(model, 6, seed=3, ransac_solver="GP3P", cross_check_f2f=True, gated_stereo=st, gated_f2f=ff,
                      gated_max_distance=cap, **kw)
        assert c.ransac_flags == _lib.FLAG_GP3P | CC_F2F | (STEREO if st else 0) | (F2F if ff else 0) | ((cap or 0) << SHIFT)
        c.ransac_flags = off.ransac_flags
        assert bytes(c) == bytes(off)                        # nothing else moves
    cam = SimpleNamespace(pct_good_matches=0.75, f2f_max_hdiff=37.5)
    rkw = dict(image_shape=(240, 320), num_of_features=900, kp_cap=None, frame_cap=None, median_win_size=3, quality=0.02,
               min_distance=7.5, edge=29, thr=0.125, max_iter=333, adaptive=False, lm_iter=17, pose_est_algorithm="EPNP",
               detection_method="ORB")
    r_off = rgbd_batch_cfg(cam, 6, seed=1, **rkw)
    r_on = rgbd_batch_cfg(cam, 6, seed=1, gated_f2f=True, gated_max_distance=80, **rkw)
    assert r_off.flags == _lib.FLAG_EPNP | _lib.rgbd_detector_flags("ORB") and r_on.flags == r_off.flags | F2F | (80 << SHIFT)
    with pytest.raises(ValueError, match="gated_max_distance"):
        rgbd_batch_cfg(cam, 6, seed=1, gated_f2f=True, gated_max_distance=300, **rkw)


def test_workspaces_do_not_depend_on_the_bits():
    """The gated search reads the keypoint positions the stores hold anyway and writes the keys the plain search writes:
    with the cross-check bits clear every workspace keeps its size, and combined with them it is the size cross-check alone
    asks for (the reverse problems' keys and slot tables)."""
    lib = lib_or_skip()
    r = ctypes.byref
    queries = (lambda c: lib.sosvo_frame_pair_batch_workspace(r(c)),
               lambda c: lib.sosvo_frame_pair_batch_streams_workspace(r(c), 2),
               lambda c: lib.sosvo_sequence_workspace(r(c), 8, 17))
    gated = (STEREO, F2F, STEREO | F2F, STEREO | F2F | (80 << SHIFT), 256 << SHIFT)
    for det in (0, 1):
        for q in queries:
            base = q(cfg(0, det))
            assert base > 0
            for g in gated:
                assert q(cfg(g, det)) == base, (det, hex(g))
                for cc in (CC_STEREO, CC_F2F, CC_STEREO | CC_F2F):
                    assert q(cfg(g | cc, det)) == q(cfg(cc, det)) > base, (det, hex(g), hex(cc))
    rqueries = (lambda c: lib.sosvo_rgbd_pair_batch_workspace(r(c)), lambda c: lib.sosvo_rgbd_sequence_workspace(r(c), 8, 17))
    for method in ("GFT", "ORB"):
        for q in rqueries:
            base = q(rgbd_cfg(0, method))
            assert base > 0 and q(rgbd_cfg(F2F, method)) == base and q(rgbd_cfg(F2F | (64 << SHIFT), method)) == base
            assert q(rgbd_cfg(F2F | CC_F2F, method)) == q(rgbd_cfg(CC_F2F, method)) > base
            # an RGB-D camera has no static stereo: SOSVO_ERR_ARG in the calls, 0 here
            assert q(rgbd_cfg(STEREO, method)) == 0 and q(rgbd_cfg(STEREO | F2F, method)) == 0


def test_the_stage_entry_refuses_a_null_context():
    lib = lib_or_skip()
    # (with a context, NULL buffers are SOSVO_ERR_ARG -- tests/test_gpu_abi_errors.py walks it)
    rc = lib.sosvo_match_hamming_gated(None, None, None, None, None, None, None, None, None, 1, 1, 8, 8, 1.0, 2.5, 256, None)
    assert rc == -1, rc


# ---- FeatureMatcher ------------------------------------------------------------------------------------------------------------
def test_feature_matcher_refuses_what_gating_is_not_defined_for():
    fm = FeatureMatcher("ORB", "BF", 1, gated=True, gated_max_distance=80)
    assert fm.gated is True and fm.gated_max_distance == 80
    plain = FeatureMatcher("ORB", "BF", 1)
    assert plain.gated is False and plain.gated_max_distance is None
    with pytest.raises(ValueError, match="k_best"):
        FeatureMatcher("ORB", "BF", 2, gated=True)
    with pytest.raises(ValueError, match="radius"):
        FeatureMatcher("ORB", "BF", 1, gated=True, use_radius_match=True)
    with pytest.raises(ValueError, match="binary"):
        FeatureMatcher("SIFT", "BF", 1, gated=True)
    with pytest.raises(ValueError, match="max_distance"):
        FeatureMatcher("ORB", "BF", 1, gated=True, gated_max_distance=300)
    d8, pts = np.zeros((4, 32), np.uint8), np.zeros((4, 2), np.float32)
    f32 = np.zeros((4, 64), np.float32)
    with pytest.raises(ValueError, match="float"):          # (all refused before any device call)
        plain.match_gated(f32, f32, pts, pts, 1.0, 2.5)
    with pytest.raises(ValueError, match="float"):
        plain.match_gated(d8, f32, pts, pts, 1.0, 2.5)
    with pytest.raises(ValueError, match="k_best"):
        FeatureMatcher("ORB", "BF", 2).match_gated(d8, d8, pts, pts, 1.0, 2.5)
    with pytest.raises(ValueError, match="radius"):
        FeatureMatcher("ORB", "BF", 1, use_radius_match=True).match_gated(d8, d8, pts, pts, 1.0, 2.5)
    with pytest.raises(ValueError, match="max_distance"):
        plain.match_gated(d8, d8, pts, pts, 1.0, 2.5, max_distance=257)
    sig = inspect.signature(FeatureMatcher.match_gated).parameters
    assert list(sig)[1:] == ["query_desc", "train_desc", "query_pts", "train_pts", "min_dv", "max_du", "max_distance"]
    assert sig["max_distance"].default is None


# ---- run_VO's arguments, the trackers' matchers, the engine cache (device calls replaced by a recorder) -----------------------
def test_every_driver_and_engine_takes_the_arguments():
    from vo_single_camera_sos_amd import pipeline
    from vo_single_camera_sos_amd.device import Context
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    for fn in (pet.run_VO, pet.run_VO_many, pet.run_VO_live, pet.driver_VO, pet.driver_VO_many, pet.driver_VO_live):
        p = inspect.signature(fn).parameters
        assert p["gated_matching"].default is None and p["gated_max_distance"].default is None, fn.__name__
    for cls in (pipeline.FramePairPipeline, pipeline.OverlappedFramePairs, pipeline.FramePairBatch, pipeline.SequenceEngine,
                pipeline.MultiSequenceEngine):
        p = inspect.signature(cls.__init__).parameters
        assert p["gated_stereo"].default is False and p["gated_f2f"].default is False, cls.__name__
        assert p["gated_max_distance"].default is None, cls.__name__
    for cls in (pipeline.RGBDPairPipeline, pipeline.RGBDPairBatch, pipeline.RGBDSequenceEngine, pipeline.RGBDMultiSequenceEngine):
        p = inspect.signature(cls.__init__).parameters
        assert p["gated_f2f"].default is False and p["gated_max_distance"].default is None and "gated_stereo" not in p, cls.__name__
    assert "match_hamming_gated" in dir(Context)


def test_set_gated_matching_switches_the_matchers():
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    t = tracker(rgbd=False)
    assert (t.gated_static_stereo, t.gated_for_motion, t.gated_max_distance) == (False, False, None)
    t.camera_model = rig = Rig()
    fms, fmm = rig.feature_matcher_for_static_stereo, rig.feature_matcher_for_motion
    pet.set_gated_matching(t, None, 80)                      # None: the tracker's own setting, whatever the cap says
    assert (fms.gated, fmm.gated, fms.gated_max_distance) == (False, False, None)
    for value, want in ((True, (True, True)), ("stereo", (True, False)), ("f2f", (False, True)), ("both", (True, True)),
                        (False, (False, False))):
        pet.set_gated_matching(t, value, 64)
        assert (fms.gated, fmm.gated) == want and (t.gated_static_stereo, t.gated_for_motion) == want, value
        assert fms.gated_max_distance == fmm.gated_max_distance == t.gated_max_distance == 64
    pet.set_gated_matching(t, True)
    assert fms.gated_max_distance is None and t.gated_max_distance is None      # None means no cap
    for bad in ("yes", "", 1, 2.0):
        with pytest.raises(ValueError, match="gated_matching"):
            pet.set_gated_matching(t, bad)
    for bad in (0, 257, 12.5):
        with pytest.raises(ValueError, match="gated_max_distance"):
            pet.set_gated_matching(t, True, bad)
    pet.set_gated_matching(t, "stereo", 64)

    def state():
        return (fms.gated, fmm.gated, fms.gated_max_distance, fmm.gated_max_distance, t.gated_static_stereo, t.gated_for_motion,
                t.gated_max_distance)
    before = state()
    assert before == (True, False, 64, 64, True, False, 64)
    fmm.use_radius_match = True                              # the second matcher refuses: the first one and the tracker stay as they were
    for value, cap in (("f2f", None), (True, 80)):
        with pytest.raises(ValueError, match="radius"):
            pet.set_gated_matching(t, value, cap)
        assert state() == before
    fmm.use_radius_match, fmm.k_best = False, 2
    with pytest.raises(ValueError, match="k_best"):
        pet.set_gated_matching(t, "f2f")
    assert state() == before
    r = tracker(rgbd=True)
    r.camera_model = cam = rgbd_cam()
    pet.set_gated_matching(r, True, 100)                     # both matchers = the one an RGB-D tracker has
    assert cam.feature_matcher_for_motion.gated is True and cam.feature_matcher_for_motion.gated_max_distance == 100
    assert r.gated_static_stereo is False
    with pytest.raises(ValueError, match="static-stereo"):
        pet.set_gated_matching(r, "stereo")


def test_the_engine_cache_key_distinguishes_the_settings(monkeypatch):
    from vo_single_camera_sos_amd import pipeline
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    monkeypatch.setattr(pipeline, "SequenceEngine", Engine)
    monkeypatch.setattr(pipeline, "MultiSequenceEngine", Engine)
    t = tracker(rgbd=False)
    t.camera_model = rig = Rig()
    img = np.zeros((4, 4, 3), np.uint8)
    seen, keys = [], set()
    settings = [(False, None), ("stereo", None), ("f2f", None), (True, None), (True, 80), (True, 64), ("f2f", 80)]
    for value, cap in settings:
        pet.set_gated_matching(t, value, cap)
        eng = pet.sequence_engine_for(t, rig, img, 32)
        want = pet.parse_cross_check(value)
        assert (eng.kwargs["gated_stereo"], eng.kwargs["gated_f2f"]) == want, value
        assert eng.kwargs["gated_max_distance"] == (cap if any(want) else None)
        assert (eng.kwargs["cross_check_stereo"], eng.kwargs["cross_check_f2f"]) == (False, False)
        assert pet.sequence_engine_for(t, rig, img, 32) is eng and eng.resets == 1     # the same settings: the same engine
        seen.append(eng)
        keys.add(pet._sos_engine_settings(t, rig, img)[2])
        multi, key = pet.multi_sequence_engine_for(t, rig, img, 32, 2)
        assert (multi.kwargs["gated_stereo"], multi.kwargs["gated_f2f"], multi.kwargs["gated_max_distance"]) == \
            (eng.kwargs["gated_stereo"], eng.kwargs["gated_f2f"], eng.kwargs["gated_max_distance"]) and key in keys
    assert len(set(map(id, seen))) == len(settings) and len(keys) == len(settings)
    pet.set_cross_check(t, True)                             # the two features' switches are independent parts of the key
    assert pet._sos_engine_settings(t, rig, img)[2] not in keys
    both = pet.sequence_engine_for(t, rig, img, 32)
    assert both.kwargs["cross_check_stereo"] and both.kwargs["gated_f2f"] and not both.kwargs["gated_stereo"]


def test_the_rgbd_engine_cache_key_distinguishes_the_settings(monkeypatch):
    from vo_single_camera_sos_amd import pipeline
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    monkeypatch.setattr(pipeline, "RGBDSequenceEngine", Engine)
    monkeypatch.setattr(pipeline, "RGBDMultiSequenceEngine", Engine)
    t = tracker(rgbd=True)
    t.camera_model = cam = rgbd_cam()
    img = np.zeros((480, 640, 3), np.uint8)
    off = pet.rgbd_sequence_engine_for(t, cam, img, 8)
    assert off.kwargs["gated_f2f"] is False and off.kwargs["gated_max_distance"] is None
    keys = {pet._rgbd_engine_settings(t, cam, img)[2]}
    for cap in (None, 80):
        pet.set_gated_matching(t, True, cap)
        on = pet.rgbd_sequence_engine_for(t, cam, img, 8)
        assert on is not off and on.kwargs["gated_f2f"] is True and on.kwargs["gated_max_distance"] == cap
        assert pet.rgbd_sequence_engine_for(t, cam, img, 8) is on and on.resets == 1
        multi, key = pet.multi_sequence_engine_for(t, cam, img, 8, 2)
        assert multi.kwargs["gated_f2f"] is True and key == pet._rgbd_engine_settings(t, cam, img)[2]
        keys.add(key)
    assert len(keys) == 3


def test_the_demos_take_the_options():
    for name in ("demo_vo_sos.py", "demo_vo_rgbd.py", "demo_vo_sos_live.py"):
        text = open(os.path.join(os.path.dirname(os.path.dirname(_lib.HEADER_PATH)), name)).read()
        assert '"--gated_matching"' in text and '"--gated_max_distance"' in text and "gated_matching=" in text, name
