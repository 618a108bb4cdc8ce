"""CPU: the mutual-consistency (cross-check) switches -- SOSVO_FLAG_CROSS_CHECK_STEREO / _F2F in sosvo_batch_cfg.ransac_flags
and sosvo_rgbd_batch_cfg.flags, the stage entry sosvo_cross_check_matches, FeatureMatcher(cross_check=True), run_VO's
cross_check argument -- keep both structs' layout, never reach the solver flags, grow the workspaces only when set, and are
part of what keys the engine kept with a camera model (device calls replaced by a recorder)."""
import ctypes
import os
import re

import numpy as np
import pytest

from cfg_fakes import Engine, Rig, cfg, lib_or_skip, rgbd_cam, rgbd_cfg, tracker
from vo_single_camera_sos_amd import _lib
from vo_single_camera_sos_amd.omnistereo.camera_models import FeatureMatcher
from vo_single_camera_sos_amd.pipeline import batch_cfg, rgbd_batch_cfg, rgbd_solver_flags

STEREO, F2F = 0x1000, 0x2000


def test_header_declares_the_macros_and_the_prototype():
    text = open(_lib.HEADER_PATH).read()
    assert "#define SOSVO_FLAG_CROSS_CHECK_STEREO 0x1000" in text and "#define SOSVO_FLAG_CROSS_CHECK_F2F 0x2000" in text
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert ("int32_t sosvo_cross_check_matches(sosvo_ctx* ctx, const uint32_t* keys_fwd, const uint32_t* keys_rev, "
            "const int32_t* nq, const int32_t* nt, const int32_t* q_slot, const int32_t* t_slot, int32_t nprob, "
            "int32_t q_stride, int32_t t_stride, uint32_t* keys_out, int32_t* n_kept);") in flat
    assert "camera_models.py:401" in text
    assert _lib.FLAG_CROSS_CHECK_STEREO == STEREO and _lib.FLAG_CROSS_CHECK_F2F == F2F
    assert "sosvo_cross_check_matches" in _lib.SIGNATURES and "sosvo_cross_check_matches" in _lib.declared_functions()
    restype, argtypes = _lib.SIGNATURES["sosvo_cross_check_matches"]
    assert restype is _lib.c_i32 and len(argtypes) == 12
    assert [a is _lib.c_i32 for a in argtypes] == [False] * 7 + [True] * 3 + [False] * 2


def test_the_bits_overlap_no_other_flag_and_never_reach_the_solver():
    both = STEREO | F2F
    others = _lib.FLAG_CAM_ROT_IDENTITY | _lib.FLAG_EPNP | _lib.FLAG_GP3P | _lib.FLAG_TWOPT | _lib.RGBD_DETECTOR_MASK
    assert both & others == 0 and STEREO & F2F == 0
    assert _lib.cross_check_flags() == 0 and _lib.cross_check_flags(True, False) == STEREO
    assert _lib.cross_check_flags(False, True) == F2F and _lib.cross_check_flags(True, True) == both
    # what the C code hands sosvo_ransac_abs_pose: (ransac_flags & GP3P) | CAM_ROT_IDENTITY, (flags & (EPNP | GP3P | TWOPT))
    for solver in ("P3P", "GP3P"):
        s = _lib.FLAG_GP3P if solver == "GP3P" else 0
        assert (s | both) & _lib.FLAG_GP3P == s
    solver_bits = _lib.FLAG_EPNP | _lib.FLAG_GP3P | _lib.FLAG_TWOPT
    for solver in ("EPNP", "KNEIP", "GAO", "GP3P", "TWOPT"):
        for method in ("GFT", "ORB", "FAST", "AGAST"):
            flags = rgbd_solver_flags(solver) | _lib.rgbd_detector_flags(method) | F2F
            assert flags & solver_bits == rgbd_solver_flags(solver)
            assert _lib.rgbd_flags_detector(flags) == _lib.DETECTORS[method]


def test_the_cfg_layouts_are_unchanged():
    assert ctypes.sizeof(_lib.BatchCfg) == 104 and ctypes.sizeof(_lib.RgbdBatchCfg) == 104
    assert [f[0] for f in _lib.BatchCfg._fields_][-1] == "detector" and len(_lib.BatchCfg._fields_) == 22
    assert len(_lib.RgbdBatchCfg._fields_) == 20 and _lib.RgbdBatchCfg.flags.offset == 44


def test_the_cfg_builders_set_the_bits():
    from types import SimpleNamespace
    model = SimpleNamespace(H=480, W=640, rows=146, cols=1440, nmask=24)
    kw = dict(num_of_features=700, kp_cap=None, frame_cap=1536, median_win_size=5, quality=0.02, min_distance=7.5, edge=29,
              thr=None, max_iter=333, adaptive=True, lm_iter=17, detection_method="GFT")
    off = batch_cfg(model, 6, seed=3, ransac_solver="GP3P", **kw)
    assert off.ransac_flags == _lib.FLAG_GP3P
    assert bytes(batch_cfg(model, 6, seed=3, ransac_solver="GP3P", cross_check_stereo=False, cross_check_f2f=False, **kw)) == bytes(off)
    for st, ff in ((True, False), (False, True), (True, True)):
        c = batch_cfg(model, 6, seed=3, ransac_solver="GP3P", cross_check_stereo=st, cross_check_f2f=ff, **kw)
        assert c.ransac_flags == _lib.FLAG_GP3P | (STEREO if st else 0) | (F2F if ff else 0)
        c.ransac_flags = off.ransac_flags
        assert bytes(c) == bytes(off)                        # nothing else moves
    cam = SimpleNamespace(pct_good_matches=0.75, f2f_max_hdiff=37.5)
    rkw = dict(image_shape=(240, 320), num_of_features=900, kp_cap=None, frame_cap=None, median_win_size=3, quality=0.02,
               min_distance=7.5, edge=29, thr=0.125, max_iter=333, adaptive=False, lm_iter=17, pose_est_algorithm="EPNP",
               detection_method="ORB")
    r_off, r_on = rgbd_batch_cfg(cam, 6, seed=1, **rkw), rgbd_batch_cfg(cam, 6, seed=1, cross_check=True, **rkw)
    assert r_off.flags == _lib.FLAG_EPNP | _lib.rgbd_detector_flags("ORB") and r_on.flags == r_off.flags | F2F


def test_workspaces_grow_only_with_a_switch_set():
    lib = lib_or_skip()
    r = ctypes.byref
    queries = (lambda c: lib.sosvo_frame_pair_batch_workspace(r(c)),
               lambda c: lib.sosvo_frame_pair_batch_streams_workspace(r(c), 2),
               lambda c: lib.sosvo_sequence_workspace(r(c), 8, 17))
    for det in (0, 1):
        for q in queries:
            base = q(cfg(0, det))
            assert base > 0 and q(cfg(_lib.FLAG_GP3P, det)) == base          # the solver bit alone changes nothing
            sizes = [q(cfg(f, det)) for f in (STEREO, F2F, STEREO | F2F)]
            assert all(s >= base for s in sizes) and sizes[0] > base and sizes[1] > base
            assert sizes[2] - base == (sizes[0] - base) + (sizes[1] - base)   # the two switches' buffers are independent
    # what a switch adds to the pair batch: the reverse keys (one u32 per forward key) and two slot tables of 2 n i32
    c = cfg(0)
    F, B = 2 * c.n_pairs, c.n_pairs
    pad = lambda n: (n + 255) & ~255  # noqa: E731
    h = F * c.nmask
    ws = queries[0]
    assert ws(cfg(STEREO)) - ws(c) == pad(2 * h * c.kp_cap * 4) - pad(h * c.kp_cap * 4) + 2 * pad(2 * h * 4)
    assert ws(cfg(F2F)) - ws(c) == 2 * (pad(2 * B * c.frame_cap * 4) - pad(B * c.frame_cap * 4)) + 2 * pad(2 * B * 4)
    rqueries = (lambda c: lib.sosvo_rgbd_pair_batch_workspace(r(c)), lambda c: lib.sosvo_rgbd_sequence_workspace(r(c), 8, 17))
    for method in ("GFT", "ORB"):
        for q in rqueries:
            base = q(rgbd_cfg(0, method))
            assert q(rgbd_cfg(F2F, method)) > base > 0
            # an RGB-D camera has no static stereo: SOSVO_ERR_ARG in the calls, 0 here
            assert q(rgbd_cfg(STEREO, method)) == 0 and q(rgbd_cfg(STEREO | F2F, method)) == 0


def test_the_stage_entry_refuses_null_arguments_before_touching_the_device():
    lib = lib_or_skip()
    # (a NULL context is refused first; with a context, NULL keys are SOSVO_ERR_ARG -- tests/test_gpu_abi_errors.py walks it)
    rc = lib.sosvo_cross_check_matches(None, None, None, None, None, None, None, 1, 8, 8, None, None)
    assert rc == -1, rc


# ---- FeatureMatcher ------------------------------------------------------------------------------------------------------------
def test_feature_matcher_refuses_what_cross_check_is_not_defined_for():
    fm = FeatureMatcher("ORB", "BF", 1, cross_check=True)
    assert fm.cross_check is True and FeatureMatcher("ORB", "BF", 1).cross_check is False
    with pytest.raises(ValueError, match="k_best"):
        FeatureMatcher("ORB", "BF", 2, cross_check=True)
    with pytest.raises(ValueError, match="radius"):
        FeatureMatcher("ORB", "BF", 1, cross_check=True, use_radius_match=True)
    with pytest.raises(ValueError, match="binary"):
        FeatureMatcher("SIFT", "BF", 1, cross_check=True)
    q = np.zeros((4, 64), np.float32)
    with pytest.raises(ValueError, match="float"):          # (refused before any device call)
        fm.match(q, q)
    with pytest.raises(ValueError, match="float"):
        fm.match_arrays(np.zeros((4, 32), np.uint8), q)
    # the switch set on an existing matcher is checked when it matches
    late = FeatureMatcher("ORB", "BF", 2)
    late.cross_check = True
    with pytest.raises(ValueError, match="k_best"):
        late.match(np.zeros((4, 32), np.uint8), np.zeros((4, 32), np.uint8))


# ---- run_VO's argument, the trackers' matchers, the engine cache (device calls replaced by a recorder) -------------------------
def test_run_vo_cross_check_values():
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import parse_cross_check
    assert parse_cross_check(None) is None
    assert parse_cross_check(True) == (True, True) and parse_cross_check(False) == (False, False)
    assert parse_cross_check(np.bool_(True)) == (True, True)
    assert parse_cross_check("stereo") == (True, False) and parse_cross_check("f2f") == (False, True)
    assert parse_cross_check("STEREO") == (True, False) and parse_cross_check("both") == (True, True)
    for bad in ("yes", "", 1, 0, 2.0, ("stereo",)):
        with pytest.raises(ValueError, match="cross_check"):
            parse_cross_check(bad)


def test_every_driver_takes_cross_check():
    import inspect
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    for fn in (pet.run_VO, pet.run_VO_many, pet.run_VO_live, pet.driver_VO, pet.driver_VO_many, pet.driver_VO_live):
        assert inspect.signature(fn).parameters["cross_check"].default is None, fn.__name__
    from vo_single_camera_sos_amd import pipeline
    for cls in (pipeline.FramePairPipeline, pipeline.OverlappedFramePairs, pipeline.FramePairBatch, pipeline.SequenceEngine,
                pipeline.MultiSequenceEngine):
        p = inspect.signature(cls.__init__).parameters
        assert p["cross_check_stereo"].default is False and p["cross_check_f2f"].default is False, cls.__name__
    for cls in (pipeline.RGBDPairPipeline, pipeline.RGBDPairBatch, pipeline.RGBDSequenceEngine, pipeline.RGBDMultiSequenceEngine):
        assert inspect.signature(cls.__init__).parameters["cross_check"].default is False, cls.__name__


def test_the_trackers_start_with_the_switches_off():
    t = tracker(rgbd=False)
    assert t.cross_check_static_stereo is False and t.cross_check_for_motion is False


def test_set_cross_check_switches_the_matchers():
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    t = tracker(rgbd=False)
    t.camera_model = rig = Rig()
    pet.set_cross_check(t, None)
    assert (rig.feature_matcher_for_static_stereo.cross_check, rig.feature_matcher_for_motion.cross_check) == (False, False)
    for value, want in ((True, (True, True)), ("stereo", (True, False)), ("f2f", (False, True)), (False, (False, False))):
        pet.set_cross_check(t, value)
        assert (rig.feature_matcher_for_static_stereo.cross_check, rig.feature_matcher_for_motion.cross_check) == want, value
        assert (t.cross_check_static_stereo, t.cross_check_for_motion) == want
    pet.set_cross_check(t, "stereo")
    rig.feature_matcher_for_motion.use_radius_match = True   # the second matcher refuses: the first one and the tracker stay as they were
    for value in ("f2f", True):
        with pytest.raises(ValueError, match="radius"):
            pet.set_cross_check(t, value)
        assert (rig.feature_matcher_for_static_stereo.cross_check, rig.feature_matcher_for_motion.cross_check) == (True, False)
        assert (t.cross_check_static_stereo, t.cross_check_for_motion) == (True, False)
    rig.feature_matcher_for_motion.use_radius_match, rig.feature_matcher_for_motion.k_best = False, 2
    with pytest.raises(ValueError, match="k_best"):
        pet.set_cross_check(t, "f2f")
    assert (rig.feature_matcher_for_static_stereo.cross_check, rig.feature_matcher_for_motion.cross_check) == (True, False)
    assert (t.cross_check_static_stereo, t.cross_check_for_motion) == (True, False)
    r = tracker(rgbd=True)
    r.camera_model = cam = rgbd_cam()
    pet.set_cross_check(r, True)                             # both matchers = the one an RGB-D tracker has
    assert cam.feature_matcher_for_motion.cross_check is True and r.cross_check_static_stereo is False
    with pytest.raises(ValueError, match="static-stereo"):
        pet.set_cross_check(r, "stereo")


def test_the_engine_cache_key_distinguishes_the_switches(monkeypatch):
    from vo_single_camera_sos_amd import pipeline
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    monkeypatch.setattr(pipeline, "SequenceEngine", Engine)
    monkeypatch.setattr(pipeline, "MultiSequenceEngine", Engine)
    t = tracker(rgbd=False)
    t.camera_model = rig = Rig()
    img = np.zeros((4, 4, 3), np.uint8)
    seen, keys = {}, set()
    for value in (False, "stereo", "f2f", True):
        pet.set_cross_check(t, value)
        eng = pet.sequence_engine_for(t, rig, img, 32)
        want = pet.parse_cross_check(value)
        assert (eng.kwargs["cross_check_stereo"], eng.kwargs["cross_check_f2f"]) == want, value
        assert pet.sequence_engine_for(t, rig, img, 32) is eng and eng.resets == 1     # the same settings: the same engine
        seen[value] = eng
        keys.add(pet._sos_engine_settings(t, rig, img)[2])
        multi, key = pet.multi_sequence_engine_for(t, rig, img, 32, 2)
        assert (multi.kwargs["cross_check_stereo"], multi.kwargs["cross_check_f2f"]) == want and key in keys
    assert len(set(map(id, seen.values()))) == 4 and len(keys) == 4
    pet.set_cross_check(t, False)
    assert pet.sequence_engine_for(t, rig, img, 32) is not seen[False]                  # (one engine per rig: it was replaced)


def test_the_rgbd_engine_cache_key_distinguishes_the_switch(monkeypatch):
    from vo_single_camera_sos_amd import pipeline
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    monkeypatch.setattr(pipeline, "RGBDSequenceEngine", Engine)
    monkeypatch.setattr(pipeline, "RGBDMultiSequenceEngine", Engine)
    t = tracker(rgbd=True)
    t.camera_model = cam = rgbd_cam()
    img = np.zeros((480, 640, 3), np.uint8)
    off = pet.rgbd_sequence_engine_for(t, cam, img, 8)
    assert off.kwargs["cross_check"] is False
    pet.set_cross_check(t, True)
    on = pet.rgbd_sequence_engine_for(t, cam, img, 8)
    assert on is not off and on.kwargs["cross_check"] is True
    assert pet.rgbd_sequence_engine_for(t, cam, img, 8) is on and on.resets == 1
    multi, key = pet.multi_sequence_engine_for(t, cam, img, 8, 2)
    assert multi.kwargs["cross_check"] is True and key == pet._rgbd_engine_settings(t, cam, img)[2]
    pet.set_cross_check(t, False)
    assert pet._rgbd_engine_settings(t, cam, img)[2] != key


def test_the_demos_take_the_option():
    for name, want in (("demo_vo_sos.py", '"--cross_check"'), ("demo_vo_rgbd.py", '"--cross_check"'),
                       ("demo_vo_sos_live.py", '"--cross_check"')):
        text = open(os.path.join(os.path.dirname(os.path.dirname(_lib.HEADER_PATH)), name)).read()
        assert want in text and "cross_check=" in text, name
