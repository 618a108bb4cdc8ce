"""CPU: the ratio-test switches -- SOSVO_FLAG_RATIO_STEREO / _F2F and SOSVO_RATIO_64THS in sosvo_batch_cfg.ransac_flags and
sosvo_rgbd_batch_cfg.flags, the stage entry sosvo_match_hamming_ratio, FeatureMatcher(ratio=...), run_VO's ratio_test / ratio
arguments -- keep both structs' layout, collide with no other bit, never reach the solver flags, leave every workspace size
alone while the switch bits are clear (with one set a workspace grows by that step's rivals), and are part of what keys the
engine kept with a camera model (device calls replaced by a recorder)."""
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

STEREO, F2F, SHIFT, MASK = 0x10, 0x20, 25, 0x3F << 25
CC_STEREO, CC_F2F, G_STEREO, G_F2F, G_SHIFT, G_MASK = 0x1000, 0x2000, 0x4000, 0x8000, 16, 0x1FF << 16


def R(r):
    return r << SHIFT


def test_header_declares_the_macros_and_the_prototype():
    text = open(_lib.HEADER_PATH).read()
    for line in ("#define SOSVO_FLAG_RATIO_STEREO 0x10", "#define SOSVO_FLAG_RATIO_F2F 0x20", "#define SOSVO_RATIO_64THS_SHIFT 25",
                 "#define SOSVO_RATIO_64THS_MASK (0x3F << SOSVO_RATIO_64THS_SHIFT)",
                 "#define SOSVO_RATIO_64THS(r) ((r) << SOSVO_RATIO_64THS_SHIFT)",
                 "#define SOSVO_RATIO_64THS_OF(flags) (((flags) & SOSVO_RATIO_64THS_MASK) >> SOSVO_RATIO_64THS_SHIFT)"):
        assert line in text, line
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert ("int32_t sosvo_match_hamming_ratio(sosvo_ctx* ctx, const uint8_t* q_desc, const uint8_t* t_desc, const float* q_pos, "
            "const float* t_pos, const int32_t* nq, const int32_t* nt, const int32_t* q_slot, const int32_t* t_slot, "
            "int32_t nprob, int32_t n_forward, int32_t q_stride, int32_t t_stride, double min_dv, double max_du, "
            "int32_t max_distance, int32_t ratio_64ths, uint32_t* keys, uint32_t* rivals);") in flat
    assert (_lib.FLAG_RATIO_STEREO, _lib.FLAG_RATIO_F2F, _lib.RATIO_64THS_SHIFT, _lib.RATIO_64THS_MASK) == (STEREO, F2F, SHIFT, MASK)
    assert "sosvo_match_hamming_ratio" in _lib.SIGNATURES and "sosvo_match_hamming_ratio" in _lib.declared_functions()
    restype, argtypes = _lib.SIGNATURES["sosvo_match_hamming_ratio"]
    assert restype is _lib.c_i32 and len(argtypes) == 19
    assert [a is _lib.c_i32 for a in argtypes] == [False] * 9 + [True] * 4 + [False] * 2 + [True, True, False, False]
    assert argtypes[13] is _lib.c_f64 and argtypes[14] is _lib.c_f64


def test_the_bits_overlap_no_other_flag_and_never_reach_the_solver():
    mine = STEREO | F2F | MASK
    others = (_lib.FLAG_CAM_ROT_IDENTITY | _lib.FLAG_EPNP | _lib.FLAG_GP3P | _lib.FLAG_TWOPT | _lib.RGBD_DETECTOR_MASK
              | _lib.FLAG_CROSS_CHECK_STEREO | _lib.FLAG_CROSS_CHECK_F2F | _lib.FLAG_GATED_STEREO | _lib.FLAG_GATED_F2F
              | _lib.GATED_MAX_DIST_MASK)
    assert mine & others == 0 and STEREO & F2F == 0 and (STEREO | F2F) & MASK == 0 and 0 < mine < 2 ** 31
    # the two detector masks: the RGB-D field above, and the omni struct's own `detector` member (no flag bits at all)
    assert _lib.RGBD_DETECTOR_MASK == 3 << 8 and max(_lib.DETECTORS.values()) <= 3
    assert MASK >> SHIFT == 63                                # the field holds 1 .. 63
    # what the C code hands sosvo_ransac_abs_pose: (ransac_flags & GP3P) | CAM_ROT_IDENTITY, (flags & (EPNP | GP3P | TWOPT))
    for s in (0, _lib.FLAG_GP3P):
        assert (s | mine) & _lib.FLAG_GP3P == s
    solver_bits = _lib.FLAG_EPNP | _lib.FLAG_GP3P | _lib.FLAG_TWOPT
    for solver in ("EPNP", "KNEIP", "GAO", "GP3P", "TWOPT"):
        for method in ("GFT", "ORB", "FAST", "AGAST"):
            flags = rgbd_solver_flags(solver) | _lib.rgbd_detector_flags(method) | F2F | MASK
            assert flags & solver_bits == rgbd_solver_flags(solver)
            assert _lib.rgbd_flags_detector(flags) == _lib.DETECTORS[method]
            assert flags & (_lib.GATED_MAX_DIST_MASK | _lib.FLAG_GATED_F2F | _lib.FLAG_CROSS_CHECK_F2F) == 0


def test_ratio_flags_encodes_and_refuses():
    assert _lib.ratio_flags() == 0
    assert _lib.ratio_flags(True, False, 0.75) == STEREO | R(48)
    assert _lib.ratio_flags(False, True, 0.75) == F2F | R(48)
    assert _lib.ratio_flags(True, True, 51 / 64.0) == STEREO | F2F | R(51)
    assert _lib.ratio_flags(True, True, 1 / 64.0) == STEREO | F2F | R(1)
    assert _lib.ratio_flags(True, True, 63 / 64.0) == STEREO | F2F | R(63)
    assert _lib.ratio_flags(False, False, 0.75) == 0          # the ratio belongs to the rule
    assert [_lib.ratio_64ths(v) for v in (0.75, 0.5, 0.90625, 1 / 64.0)] == [48, 32, 58, 1]
    with pytest.raises(ValueError, match="needs a ratio"):
        _lib.ratio_flags(True, False)
    # nothing is rounded: 0.7 and 0.8 are no 64ths, and the message names the two nearest admissible values
    with pytest.raises(ValueError, match=r"0\.6875 \(44/64\) and 0\.703125 \(45/64\)"):
        _lib.ratio_flags(True, False, 0.7)
    with pytest.raises(ValueError, match=r"0\.796875 \(51/64\) and 0\.8125 \(52/64\)"):
        _lib.ratio_64ths(0.8)
    for bad in (0.0, 1.0, -0.25, 1.5, 0.75 + 1e-9, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="ratio"):
            _lib.ratio_64ths(bad)
    with pytest.raises(ValueError, match="ratio"):            # checked even when no switch is set
        _lib.ratio_flags(False, False, 0.7)


def test_the_cfg_layouts_are_unchanged():
    assert ctypes.sizeof(_lib.BatchCfg) == 104 and ctypes.sizeof(_lib.RgbdBatchCfg) == 104
    assert len(_lib.BatchCfg._fields_) == 22 and len(_lib.RgbdBatchCfg._fields_) == 20 and _lib.RgbdBatchCfg.flags.offset == 44


def test_the_cfg_builders_set_exactly_the_bits():
    from types import SimpleNamespace
    model = SimpleNamespace(H=480, W=640, rows=146, cols=1440, nmask=24)
    kw = dict(num_of_features=700, kp_cap=None, frame_cap=1536, median_win_size=5, quality=0.02, min_distance=7.5, edge=29,
              thr=None, max_iter=333, adaptive=True, lm_iter=17, detection_method="GFT")
    off = batch_cfg(model, 6, seed=3, ransac_solver="GP3P", **kw)
    assert off.ransac_flags == _lib.FLAG_GP3P
    assert bytes(batch_cfg(model, 6, seed=3, ransac_solver="GP3P", ratio_stereo=False, ratio_f2f=False, ratio=0.75, **kw)) == bytes(off)
    for st, ff, r in ((True, False, 0.75), (False, True, 51 / 64.0), (True, True, 58 / 64.0)):
        c = batch_cfg(model, 6, seed=3, ransac_solver="GP3P", cross_check_f2f=True, gated_stereo=True, gated_max_distance=80,
                      ratio_stereo=st, ratio_f2f=ff, ratio=r, **kw)
        assert c.ransac_flags == (_lib.FLAG_GP3P | CC_F2F | G_STEREO | (80 << G_SHIFT) | (STEREO if st else 0) | (F2F if ff else 0)
                                  | R(int(r * 64)))
        c.ransac_flags = off.ransac_flags
        assert bytes(c) == bytes(off)                        # nothing else moves
    with pytest.raises(ValueError, match="ratio"):
        batch_cfg(model, 6, seed=3, ransac_solver="GP3P", ratio_f2f=True, **kw)
    cam = SimpleNamespace(pct_good_matches=0.75, f2f_max_hdiff=37.5)
    rkw = dict(image_shape=(240, 320), num_of_features=900, kp_cap=None, frame_cap=None, median_win_size=3, quality=0.02,
               min_distance=7.5, edge=29, thr=0.125, max_iter=333, adaptive=False, lm_iter=17, pose_est_algorithm="EPNP",
               detection_method="ORB")
    r_off = rgbd_batch_cfg(cam, 6, seed=1, **rkw)
    r_on = rgbd_batch_cfg(cam, 6, seed=1, ratio_f2f=True, ratio=0.75, **rkw)
    assert r_off.flags == _lib.FLAG_EPNP | _lib.rgbd_detector_flags("ORB") and r_on.flags == r_off.flags | F2F | R(48)
    assert rgbd_batch_cfg(cam, 6, seed=1, ratio=0.75, **rkw).flags == r_off.flags
    with pytest.raises(ValueError, match="ratio"):
        rgbd_batch_cfg(cam, 6, seed=1, ratio_f2f=True, ratio=0.7, **rkw)


def test_workspaces_change_only_with_a_switch_set():
    """With the switch bits clear -- the field set or not, the other features' switches set or not -- every workspace has
    the size it had; a switch with a ratio adds that step's rivals (one u32 per key of the step: doubled with the step's
    cross-check) and nothing else; a switch without a ratio, or the stereo switch for an RGB-D camera, is 0."""
    lib = lib_or_skip()
    r = ctypes.byref
    al = lambda n: (n + 255) & ~255                            # noqa: E731 -- the carver's alignment
    queries = ((lambda c: lib.sosvo_frame_pair_batch_workspace(r(c)), 2 * 4, 4),            # (query, frames of a window, pairs)
               (lambda c: lib.sosvo_sequence_workspace(r(c), 8, 17), 8, 4))
    others = (0, CC_STEREO, CC_F2F, CC_STEREO | CC_F2F, G_STEREO, G_F2F | (80 << G_SHIFT), CC_STEREO | CC_F2F | G_STEREO | G_F2F)
    for det in (0, 1):
        for q, window, pairs in queries:
            for o in others:
                base = q(cfg(o, det))
                assert base > 0
                assert q(cfg(o | R(48), det)) == base, (det, hex(o))            # the field alone is ignored
                n_stereo = (2 if o & CC_STEREO else 1) * window * 12 * 1024       # frames * nmask * kp_cap keys
                n_f2f = (2 if o & CC_F2F else 1) * pairs * 2048                   # pairs * frame_cap keys (one buffer, both views)
                assert q(cfg(o | STEREO | R(48), det)) == base + al(4 * n_stereo), (det, hex(o))
                assert q(cfg(o | F2F | R(1), det)) == base + al(4 * n_f2f), (det, hex(o))
                assert q(cfg(o | STEREO | F2F | R(63), det)) == base + al(4 * n_stereo) + al(4 * n_f2f), (det, hex(o))
                for sw in (STEREO, F2F, STEREO | F2F):                              # a switch needs a ratio
                    assert q(cfg(o | sw, det)) == 0, (det, hex(o), hex(sw))
        streams = lambda c: lib.sosvo_frame_pair_batch_streams_workspace(r(c), 2)    # noqa: E731
        base = streams(cfg(0, det))
        assert base > 0 and streams(cfg(R(48), det)) == base and streams(cfg(STEREO, det)) == 0
        assert streams(cfg(STEREO | F2F | R(48), det)) > base
    rqueries = (lambda c: lib.sosvo_rgbd_pair_batch_workspace(r(c)), lambda c: lib.sosvo_rgbd_sequence_workspace(r(c), 8, 17))
    for method in ("GFT", "ORB"):
        for q in rqueries:
            for o in (0, CC_F2F, G_F2F | (64 << G_SHIFT), CC_F2F | G_F2F):
                base = q(rgbd_cfg(o, method))
                assert base > 0 and q(rgbd_cfg(o | R(48), method)) == base
                n_f2f = (2 if o & CC_F2F else 1) * 4 * 1088
                assert q(rgbd_cfg(o | F2F | R(48), method)) == base + al(4 * n_f2f), (method, hex(o))
                assert q(rgbd_cfg(o | F2F, method)) == 0                         # a switch needs a ratio
                # an RGB-D camera has no static stereo: SOSVO_ERR_ARG in the calls, 0 here
                assert q(rgbd_cfg(o | STEREO | R(48), method)) == 0 and q(rgbd_cfg(o | STEREO | F2F | R(48), method)) == 0


def test_the_stage_entry_refuses_a_null_context():
    lib = lib_or_skip()
    # (with a context, NULL buffers are SOSVO_ERR_ARG -- tests/test_gpu_abi_errors.py walks it)
    rc = lib.sosvo_match_hamming_ratio(None, None, None, None, None, None, None, None, None, 1, 1, 8, 8, 1.0, 2.5, 256, 48, None, None)
    assert rc == -1, rc


# ---- FeatureMatcher ------------------------------------------------------------------------------------------------------------
def test_feature_matcher_refuses_what_the_ratio_is_not_defined_for():
    fm = FeatureMatcher("ORB", "BF", 1, ratio=0.75)
    assert fm.ratio == 0.75 and fm._check_ratio() == 48
    plain = FeatureMatcher("ORB", "BF", 1)
    assert plain.ratio is None and plain._check_ratio() == 0
    with pytest.raises(ValueError, match="k_best"):
        FeatureMatcher("ORB", "BF", 2, ratio=0.75)
    with pytest.raises(ValueError, match="radius"):
        FeatureMatcher("ORB", "BF", 1, ratio=0.75, use_radius_match=True)
    with pytest.raises(ValueError, match="binary"):
        FeatureMatcher("SIFT", "BF", 1, ratio=0.75)
    with pytest.raises(ValueError, match="nearest admissible"):
        FeatureMatcher("ORB", "BF", 1, ratio=0.7)
    FeatureMatcher("SIFT", "BF", 2)                          # (the reference-shaped host rule needs no ratio and stays)
    d8, pts = np.zeros((4, 32), np.uint8), np.zeros((4, 2), np.float32)
    f32 = np.zeros((4, 64), np.float32)
    for call in (lambda m: m.match(f32, f32), lambda m: m.match_arrays(d8, f32), lambda m: m.match_arrays_many([(f32, d8)]),
                 lambda m: m.match_gated(f32, f32, pts, pts, 1.0, 2.5), lambda m: m.match_gated_many([(d8, f32, pts, pts)], 1.0, 2.5)):
        with pytest.raises(ValueError, match="float"):      # (all refused before any device call)
            call(fm)
    late = FeatureMatcher("ORB", "BF", 1)
    late.ratio, late.k_best = 0.75, 2                        # (set after construction, as set_ratio_test does)
    for call in (lambda m: m.match(d8, d8), lambda m: m.match_arrays_many([(d8, d8)]), lambda m: m.match_gated(d8, d8, pts, pts, 1.0, 2.5)):
        with pytest.raises(ValueError, match="k_best"):
            call(late)
    late.k_best, late.use_radius_match = 1, True
    for call in (lambda m: m.match(d8, d8), lambda m: m.match_arrays_many([(d8, d8)]), lambda m: m.match_gated(d8, d8, pts, pts, 1.0, 2.5)):
        with pytest.raises(ValueError, match="radius"):
            call(late)
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
        assert p["ratio_test"].default is None and p["ratio"].default is None, fn.__name__
    for cls in (pipeline.FramePairPipeline, pipeline.OverlappedFramePairs, pipeline.FramePairBatch, pipeline.SequenceEngine,
                pipeline.MultiSequenceEngine):
        p = inspect.signature(cls.__init__).parameters
        assert p["ratio_stereo"].default is False and p["ratio_f2f"].default is False and p["ratio"].default is None, cls.__name__
    for cls in (pipeline.RGBDPairPipeline, pipeline.RGBDPairBatch, pipeline.RGBDSequenceEngine, pipeline.RGBDMultiSequenceEngine):
        p = inspect.signature(cls.__init__).parameters
        assert p["ratio_f2f"].default is False and p["ratio"].default is None and "ratio_stereo" not in p, cls.__name__
    for fn in (batch_cfg, rgbd_batch_cfg):
        p = inspect.signature(fn).parameters
        assert p["ratio_f2f"].default is False and p["ratio"].default is None, fn.__name__
    assert "match_hamming_ratio" in dir(Context)
    assert list(inspect.signature(pet.set_ratio_test).parameters) == ["tracker", "ratio_test", "ratio"]


def test_set_ratio_test_switches_the_matchers():
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    t = tracker(rgbd=False)
    assert (t.ratio_static_stereo, t.ratio_for_motion) == (None, None)
    t.camera_model = rig = Rig()
    fms, fmm = rig.feature_matcher_for_static_stereo, rig.feature_matcher_for_motion
    pet.set_ratio_test(t, None, 0.75)                        # None: the tracker's own setting, whatever the ratio says
    assert (fms.ratio, fmm.ratio) == (None, None)
    for value, want in ((True, (True, True)), ("stereo", (True, False)), ("f2f", (False, True)), ("both", (True, True)),
                        (False, (False, False))):
        pet.set_ratio_test(t, value, 0.75)
        assert (fms.ratio, fmm.ratio) == tuple(0.75 if w else None for w in want), value
        assert (t.ratio_static_stereo, t.ratio_for_motion) == (fms.ratio, fmm.ratio)
    for bad in ("yes", "", 1, 2.0):
        with pytest.raises(ValueError, match="ratio_test"):
            pet.set_ratio_test(t, bad, 0.75)
    with pytest.raises(ValueError, match="needs a ratio"):
        pet.set_ratio_test(t, True)
    for bad in (0.7, 0.0, 1.0, 48):
        with pytest.raises(ValueError, match="ratio"):
            pet.set_ratio_test(t, True, bad)
    assert (fms.ratio, fmm.ratio) == (None, None)            # (a refused setting changes nothing)
    pet.set_ratio_test(t, "stereo", 0.5)
    fmm.use_radius_match = True                              # the second matcher refuses: the first one and the tracker stay as they were
    with pytest.raises(ValueError, match="radius"):
        pet.set_ratio_test(t, True, 0.75)
    assert (fms.ratio, fmm.ratio, t.ratio_static_stereo, t.ratio_for_motion) == (0.5, None, 0.5, None)
    fmm.use_radius_match, fmm.k_best = False, 2
    with pytest.raises(ValueError, match="k_best"):
        pet.set_ratio_test(t, "f2f", 0.75)
    assert (fms.ratio, fmm.ratio, t.ratio_static_stereo, t.ratio_for_motion) == (0.5, None, 0.5, None)
    r = tracker(rgbd=True)
    r.camera_model = cam = rgbd_cam()
    pet.set_ratio_test(r, True, 0.75)                        # both matchers = the one an RGB-D tracker has
    assert cam.feature_matcher_for_motion.ratio == 0.75 and r.ratio_static_stereo is None and r.ratio_for_motion == 0.75
    with pytest.raises(ValueError, match="static-stereo"):
        pet.set_ratio_test(r, "stereo", 0.75)


def test_the_engine_cache_key_distinguishes_the_settings(monkeypatch):
    from vo_single_camera_sos_amd import pipeline
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    monkeypatch.setattr(pipeline, "SequenceEngine", Engine)
    monkeypatch.setattr(pipeline, "MultiSequenceEngine", Engine)
    t = tracker(rgbd=False)
    t.camera_model = rig = Rig()
    img = np.zeros((4, 4, 3), np.uint8)
    seen, keys = [], set()
    settings = [(False, 0.75), ("stereo", 0.75), ("f2f", 0.75), (True, 0.75), (True, 51 / 64.0), ("f2f", 58 / 64.0)]
    for value, ratio in settings:
        pet.set_ratio_test(t, value, ratio)
        eng = pet.sequence_engine_for(t, rig, img, 32)
        want = pet.parse_cross_check(value)
        assert (eng.kwargs["ratio_stereo"], eng.kwargs["ratio_f2f"]) == want, value
        assert eng.kwargs["ratio"] == (ratio if any(want) else None)
        assert (eng.kwargs["cross_check_stereo"], eng.kwargs["gated_f2f"]) == (False, False)
        assert pet.sequence_engine_for(t, rig, img, 32) is eng and eng.resets == 1     # the same settings: the same engine
        seen.append(eng)
        keys.add(pet._sos_engine_settings(t, rig, img)[2])
        multi, key = pet.multi_sequence_engine_for(t, rig, img, 32, 2)
        assert (multi.kwargs["ratio_stereo"], multi.kwargs["ratio_f2f"], multi.kwargs["ratio"]) == \
            (eng.kwargs["ratio_stereo"], eng.kwargs["ratio_f2f"], eng.kwargs["ratio"]) and key in keys
    assert len(set(map(id, seen))) == len(settings) and len(keys) == len(settings)
    pet.set_gated_matching(t, True, 80)                      # the features' switches are independent parts of the key
    assert pet._sos_engine_settings(t, rig, img)[2] not in keys
    both = pet.sequence_engine_for(t, rig, img, 32)
    assert both.kwargs["gated_stereo"] and both.kwargs["ratio_f2f"] and not both.kwargs["ratio_stereo"]
    # the engine has one ratio: matchers that were given two different ones have no batched counterpart
    rig.feature_matcher_for_static_stereo.ratio = 0.5
    assert pet._sos_engine_settings(t, rig, img) is None


def test_the_rgbd_engine_cache_key_distinguishes_the_settings(monkeypatch):
    from vo_single_camera_sos_amd import pipeline
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    monkeypatch.setattr(pipeline, "RGBDSequenceEngine", Engine)
    monkeypatch.setattr(pipeline, "RGBDMultiSequenceEngine", Engine)
    t = tracker(rgbd=True)
    t.camera_model = cam = rgbd_cam()
    img = np.zeros((480, 640, 3), np.uint8)
    off = pet.rgbd_sequence_engine_for(t, cam, img, 8)
    assert off.kwargs["ratio_f2f"] is False and off.kwargs["ratio"] is None
    keys = {pet._rgbd_engine_settings(t, cam, img)[2]}
    for ratio in (0.75, 51 / 64.0):
        pet.set_ratio_test(t, True, ratio)
        on = pet.rgbd_sequence_engine_for(t, cam, img, 8)
        assert on is not off and on.kwargs["ratio_f2f"] is True and on.kwargs["ratio"] == ratio
        assert pet.rgbd_sequence_engine_for(t, cam, img, 8) is on and on.resets == 1
        multi, key = pet.multi_sequence_engine_for(t, cam, img, 8, 2)
        assert multi.kwargs["ratio_f2f"] is True and key == pet._rgbd_engine_settings(t, cam, img)[2]
        keys.add(key)
    assert len(keys) == 3


def test_the_demos_take_the_options():
    for name in ("demo_vo_sos.py", "demo_vo_rgbd.py", "demo_vo_sos_live.py"):
        text = open(os.path.join(os.path.dirname(os.path.dirname(_lib.HEADER_PATH)), name)).read()
        assert '"--ratio_test"' in text and '"--ratio"' in text and "ratio_test=" in text and "ratio=args.ratio" in text, name
