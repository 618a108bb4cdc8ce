"""CPU: the sub-pixel refinement switch -- SOSVO_FLAG_SUBPIX and SOSVO_SUBPIX_HALF in sosvo_batch_cfg.ransac_flags, the stage
entry sosvo_refine_subpix, ImageFrontEnd(subpix=...), run_VO's subpix_refine / subpix_half arguments -- keeps both structs'
layout, collides with no other bit, never reaches the solver flags, leaves every workspace size alone (the stage needs no
workspace), is refused for an RGB-D camera, and is part of what keys the engine kept with a camera model (device calls
replaced by a recorder)."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from cfg_fakes import Engine, Rig, cfg, lib_or_skip, rgbd_cam, rgbd_cfg, tracker
from vo_single_camera_sos_amd import _lib
from vo_single_camera_sos_amd.pipeline import batch_cfg, rgbd_solver_flags

SUBPIX, SHIFT, MASK = 0x40, 10, 3 << 10


def H(h):
    return (h - 2) << SHIFT


def test_header_declares_the_macros_and_the_prototypes():
    text = open(_lib.HEADER_PATH).read()
    for line in ("#define SOSVO_FLAG_SUBPIX 0x40", "#define SOSVO_SUBPIX_HALF_SHIFT 10",
                 "#define SOSVO_SUBPIX_HALF_MASK (3 << SOSVO_SUBPIX_HALF_SHIFT)",
                 "#define SOSVO_SUBPIX_HALF(h) (((h) - 2) << SOSVO_SUBPIX_HALF_SHIFT)",
                 "#define SOSVO_SUBPIX_HALF_OF(flags) ((((flags) & SOSVO_SUBPIX_HALF_MASK) >> SOSVO_SUBPIX_HALF_SHIFT) + 2)"):
        assert line in text, line
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert ("int32_t sosvo_refine_subpix(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols, "
            "int32_t nmask, int32_t cap, float* kp, const int32_t* n, int32_t half, int32_t max_iter, double eps, "
            "const int32_t* row_range);") in flat
    assert "int32_t sosvo_subpix_weights(sosvo_ctx* ctx, int32_t half, int32_t* w_host);" in flat
    assert (_lib.FLAG_SUBPIX, _lib.SUBPIX_HALF_SHIFT, _lib.SUBPIX_HALF_MASK) == (SUBPIX, SHIFT, MASK)
    assert (_lib.SUBPIX_MAX_ITER, _lib.SUBPIX_EPS) == (10, 0.01)
    for name in ("sosvo_refine_subpix", "sosvo_subpix_weights"):
        assert name in _lib.SIGNATURES and name in _lib.declared_functions()
    restype, argtypes = _lib.SIGNATURES["sosvo_refine_subpix"]
    assert restype is _lib.c_i32 and len(argtypes) == 13 and argtypes[11] is _lib.c_f64
    assert [a is _lib.c_i32 for a in argtypes] == [False] * 2 + [True] * 5 + [False] * 2 + [True] * 2 + [False] * 2


def test_the_bits_overlap_no_other_flag_and_never_reach_the_solver():
    mine = SUBPIX | MASK
    others = (_lib.FLAG_CAM_ROT_IDENTITY | _lib.FLAG_EPNP | _lib.FLAG_GP3P | _lib.FLAG_TWOPT | _lib.RGBD_DETECTOR_MASK
              | _lib.FLAG_CROSS_CHECK_STEREO | _lib.FLAG_CROSS_CHECK_F2F | _lib.FLAG_GATED_STEREO | _lib.FLAG_GATED_F2F
              | _lib.GATED_MAX_DIST_MASK | _lib.FLAG_RATIO_STEREO | _lib.FLAG_RATIO_F2F | _lib.RATIO_64THS_MASK)
    assert mine & others == 0 and SUBPIX & MASK == 0 and 0 < mine < 2 ** 31
    assert MASK >> SHIFT == 3                                   # the field holds half - 2 = 0 .. 3
    # what the C code hands sosvo_ransac_abs_pose: (ransac_flags & GP3P) | CAM_ROT_IDENTITY, (flags & (EPNP | GP3P | TWOPT))
    for s in (0, _lib.FLAG_GP3P):
        assert (s | mine) & _lib.FLAG_GP3P == s
    solver_bits = _lib.FLAG_EPNP | _lib.FLAG_GP3P | _lib.FLAG_TWOPT
    for solver in ("EPNP", "KNEIP", "GAO", "GP3P", "TWOPT"):
        assert (rgbd_solver_flags(solver) | mine) & solver_bits == rgbd_solver_flags(solver)


def test_subpix_flags_round_trip_and_refuse():
    assert _lib.subpix_flags() == 0 and _lib.subpix_flags(None) == 0 and _lib.subpix_flags(False) == 0
    assert _lib.subpix_flags(True) == SUBPIX | H(5)
    for h in (2, 3, 4, 5):
        f = _lib.subpix_flags(h)
        assert f == SUBPIX | H(h) and _lib.subpix_half_of(f) == h and _lib.subpix_half(h) == h
        assert _lib.subpix_half_of(f | _lib.FLAG_GP3P | _lib.FLAG_RATIO_F2F | (48 << _lib.RATIO_64THS_SHIFT)) == h
        assert _lib.subpix_half_of(H(h)) is None               # the field belongs to the switch
    assert _lib.subpix_half(np.int64(3)) == 3 and _lib.subpix_half(4.0) == 4
    for bad in (0, 1, 6, -3, 2.5, 100):
        with pytest.raises(ValueError, match="subpix"):
            _lib.subpix_flags(bad)


def test_the_cfg_layouts_are_unchanged():
    assert ctypes.sizeof(_lib.BatchCfg) == 104 and ctypes.sizeof(_lib.RgbdBatchCfg) == 104
    assert len(_lib.BatchCfg._fields_) == 22 and len(_lib.RgbdBatchCfg._fields_) == 20 and _lib.RgbdBatchCfg.flags.offset == 44


def test_the_cfg_builder_sets_exactly_the_bits():
    model = SimpleNamespace(H=480, W=640, rows=146, cols=1440, nmask=24)
    kw = dict(num_of_features=700, kp_cap=None, frame_cap=1536, median_win_size=5, quality=0.02, min_distance=7.5, edge=29,
              thr=None, max_iter=333, adaptive=True, lm_iter=17, detection_method="GFT")
    off = batch_cfg(model, 6, seed=3, ransac_solver="GP3P", **kw)
    assert off.ransac_flags == _lib.FLAG_GP3P
    assert bytes(batch_cfg(model, 6, seed=3, ransac_solver="GP3P", subpix=None, **kw)) == bytes(off)
    for h in (2, 3, 5):
        c = batch_cfg(model, 6, seed=3, ransac_solver="GP3P", gated_stereo=True, ratio_f2f=True, ratio=0.75, subpix=h, **kw)
        assert c.ransac_flags == (_lib.FLAG_GP3P | _lib.FLAG_GATED_STEREO | _lib.FLAG_RATIO_F2F | (48 << _lib.RATIO_64THS_SHIFT)
                                  | SUBPIX | H(h))
        c.ransac_flags = off.ransac_flags
        assert bytes(c) == bytes(off)                          # nothing else moves
    with pytest.raises(ValueError, match="subpix"):
        batch_cfg(model, 6, seed=3, ransac_solver="GP3P", subpix=6, **kw)


def test_no_workspace_changes_and_rgbd_refuses():
    """The stage needs no workspace: with the switch set every omni workspace has the size it has with the switch clear,
    whatever the other features' switches; the field alone is ignored; in an RGB-D configuration the switch answers 0."""
    lib = lib_or_skip()
    r = ctypes.byref
    queries = (lambda c: lib.sosvo_frame_pair_batch_workspace(r(c)), lambda c: lib.sosvo_sequence_workspace(r(c), 8, 17),
               lambda c: lib.sosvo_frame_pair_batch_streams_workspace(r(c), 2))
    others = (0, _lib.FLAG_CROSS_CHECK_STEREO | _lib.FLAG_CROSS_CHECK_F2F, _lib.FLAG_GATED_STEREO | (80 << 16),
              _lib.FLAG_RATIO_STEREO | _lib.FLAG_RATIO_F2F | (48 << _lib.RATIO_64THS_SHIFT))
    for det in (0, 1, 2):
        for q in queries:
            for o in others:
                base = q(cfg(o, det))
                assert base > 0
                for h in (2, 3, 4, 5):
                    assert q(cfg(o | SUBPIX | H(h), det)) == base, (det, hex(o), h)
                    assert q(cfg(o | H(h), det)) == base, (det, hex(o), h)
    rqueries = (lambda c: lib.sosvo_rgbd_pair_batch_workspace(r(c)), lambda c: lib.sosvo_rgbd_sequence_workspace(r(c), 8, 17))
    for method in ("GFT", "ORB"):
        for q in rqueries:
            assert q(rgbd_cfg(0, method)) > 0
            # (bits 10-11 alone mean nothing there; the switch is SOSVO_ERR_ARG in the calls, 0 here)
            assert q(rgbd_cfg(SUBPIX, method)) == 0 and q(rgbd_cfg(SUBPIX | H(5), method)) == 0
            assert q(rgbd_cfg(SUBPIX | _lib.FLAG_CROSS_CHECK_F2F, method)) == 0


def test_the_stage_entry_refuses_a_null_context():
    lib = lib_or_skip()
    # (with a context, NULL buffers and bad ranges are SOSVO_ERR_ARG -- tests/test_gpu_subpix.py)
    assert lib.sosvo_refine_subpix(None, None, 2, 8, 8, 1, 4, None, None, 5, 10, 0.01, None) == -1


# ---- the Python layers ---------------------------------------------------------------------------------------------------------
class _Stop(Exception):
    pass


def test_every_driver_and_engine_takes_the_arguments():
    from vo_single_camera_sos_amd import frontend, pipeline
    from vo_single_camera_sos_amd.device import Context
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    for fn in (pet.run_VO, pet.run_VO_many, pet.run_VO_live, pet.driver_VO, pet.driver_VO_many, pet.driver_VO_live):
        p = inspect.signature(fn).parameters
        assert p["subpix_refine"].default is None and p["subpix_half"].default is None, fn.__name__
    for cls in (frontend.ImageFrontEnd, pipeline.FramePairPipeline, pipeline.OverlappedFramePairs, pipeline.FramePairBatch,
                pipeline.SequenceEngine, pipeline.MultiSequenceEngine):
        assert inspect.signature(cls.__init__).parameters["subpix"].default is None, cls.__name__
    for cls in (pipeline.RGBDPairPipeline, pipeline.RGBDPairBatch, pipeline.RGBDSequenceEngine, pipeline.RGBDMultiSequenceEngine):
        assert "subpix" not in inspect.signature(cls.__init__).parameters, cls.__name__
    assert inspect.signature(batch_cfg).parameters["subpix"].default is None
    assert "subpix" not in inspect.signature(pipeline.rgbd_batch_cfg).parameters
    assert "refine_subpix" in dir(Context)
    assert list(inspect.signature(Context.refine_subpix).parameters)[1:] == ["gray", "kp", "n", "nmask", "half", "max_iter", "eps",
                                                                              "row_range"]
    sig = inspect.signature(pet.set_subpixel_refinement).parameters
    assert list(sig) == ["tracker", "subpix", "half"] and sig["half"].default == 5


def test_every_constructor_hands_the_value_inward(monkeypatch):
    """ImageFrontEnd keeps it (on a stand-in context: host tensors); FramePairPipeline hands it to its front end; the one-call
    and sequence engines hand it, in their StepOptions, to the function behind batch_cfg (recorded, and the construction
    stopped there)."""
    from vo_single_camera_sos_amd import frontend, pipeline
    from vo_single_camera_sos_amd.device import Context
    model = SimpleNamespace(H=8, W=8, rows=4, cols=4, nmask=1, unwrap_table=object())
    monkeypatch.setattr(frontend, "Context", SimpleNamespace)
    fe = frontend.ImageFrontEnd(SimpleNamespace(device="cpu"), model, 2, subpix=3)
    assert fe.subpix == 3 and frontend.ImageFrontEnd(SimpleNamespace(device="cpu"), model, 2).subpix is None
    assert frontend.ImageFrontEnd(SimpleNamespace(device="cpu"), model, 2, subpix=True).subpix == 5
    with pytest.raises(ValueError, match="subpix"):
        frontend.ImageFrontEnd(SimpleNamespace(device="cpu"), model, 2, subpix=7)
    calls = []
    monkeypatch.setattr(fe.ctx, "refine_subpix", lambda *a, **k: calls.append((a, k)), raising=False)
    monkeypatch.setattr(fe, "_detect_describe", lambda: calls.append("detect"))
    fe.run_features()                                          # the refinement follows the descriptors, on the same buffers
    assert calls[0] == "detect" and calls[1][0][:4] == (fe.gray, fe.kp, fe.n, 1) and calls[1][1] == dict(half=3, row_range=None)
    fe.subpix, calls[:] = None, []
    fe.run_features()
    assert calls == ["detect"]

    ctx = Context.__new__(Context)

    class StopRig(object):
        def as_struct(self):
            raise _Stop()
    with pytest.raises(_Stop):
        pipeline.FramePairPipeline(ctx, StopRig(), 1, front_end=fe, subpix=4)
    assert fe.subpix == 4
    with pytest.raises(_Stop):
        pipeline.FramePairPipeline(ctx, StopRig(), 1, front_end=fe)        # None: the front end's own setting stays
    assert fe.subpix == 4
    with pytest.raises(ValueError, match="subpix"):
        pipeline.FramePairPipeline(ctx, StopRig(), 1, front_end=fe, subpix=9)
    with pytest.raises(ValueError, match="front end"):
        pipeline.FramePairPipeline(ctx, StopRig(), 1, subpix=4)

    seen = []

    def recorder(so, *args, **kwargs):      # (the engines hand their StepOptions to the function behind batch_cfg)
        seen.append(so.subpix if "subpix" not in kwargs else "twice")
        raise _Stop()
    monkeypatch.setattr(pipeline, "_batch_cfg", recorder)
    rig = SimpleNamespace(as_struct=lambda: None)
    for build in (lambda s: pipeline.FramePairBatch(ctx, model, rig, 2, subpix=s),
                  lambda s: pipeline.SequenceEngine(ctx, model, rig, window=2, subpix=s),
                  lambda s: pipeline.MultiSequenceEngine(ctx, model, rig, lanes=2, window=2, subpix=s)):
        for s in (None, 2, 5):
            with pytest.raises(_Stop):
                build(s)
            assert seen[-1] == s


def test_set_subpixel_refinement_switches_the_frames_and_the_tracker():
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    t = tracker(rgbd=False)
    assert t.subpix_half is None
    t.camera_model = rig = Rig()
    fms = rig.feature_matcher_for_static_stereo
    pet.set_subpixel_refinement(t, None, 3)                   # None: the tracker's own setting, whatever half says
    assert getattr(fms, "subpix_half", None) is None and t.subpix_half is None
    for value, half, want in ((True, 5, 5), (True, None, 5), (True, 2, 2), (False, 3, None), (True, 3, 3)):
        pet.set_subpixel_refinement(t, value, half)
        assert fms.subpix_half == want and t.subpix_half == want, (value, half)
    pet.set_subpixel_refinement(t, True)
    assert fms.subpix_half == 5
    for bad in (1, 6, 2.5):
        with pytest.raises(ValueError, match="subpix"):
            pet.set_subpixel_refinement(t, True, bad)
    for bad in ("yes", 1, "stereo"):
        with pytest.raises(ValueError, match="subpix_refine"):
            pet.set_subpixel_refinement(t, bad)
    assert fms.subpix_half == 5 and t.subpix_half == 5         # (a refused setting changes nothing)
    r = tracker(rgbd=True)
    r.camera_model = rgbd_cam()
    pet.set_subpixel_refinement(r, False)
    pet.set_subpixel_refinement(r, None)
    with pytest.raises(ValueError, match="integer pixels"):
        pet.set_subpixel_refinement(r, True)
    assert r.subpix_half is None


def test_the_engine_cache_key_distinguishes_the_settings(monkeypatch):
    from vo_single_camera_sos_amd import pipeline
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    monkeypatch.setattr(pipeline, "SequenceEngine", Engine)
    monkeypatch.setattr(pipeline, "MultiSequenceEngine", Engine)
    t = tracker(rgbd=False)
    t.camera_model = rig = Rig()
    img = np.zeros((4, 4, 3), np.uint8)
    seen, keys = [], set()
    settings = [(False, None, None), (True, None, 5), (True, 2, 2), (True, 3, 3)]
    for value, half, want in settings:
        pet.set_subpixel_refinement(t, value, half)
        eng = pet.sequence_engine_for(t, rig, img, 32)
        assert eng.kwargs["subpix"] == want and eng.kwargs["ratio_f2f"] is False
        assert pet.sequence_engine_for(t, rig, img, 32) is eng and eng.resets == 1     # the same settings: the same engine
        seen.append(eng)
        keys.add(pet._sos_engine_settings(t, rig, img)[2])
        multi, key = pet.multi_sequence_engine_for(t, rig, img, 32, 2)
        assert multi.kwargs["subpix"] == want and key in keys
    assert len(set(map(id, seen))) == len(settings) and len(keys) == len(settings)
    pet.set_ratio_test(t, "f2f", 0.75)                         # the features' switches are independent parts of the key
    assert pet._sos_engine_settings(t, rig, img)[2] not in keys
    both = pet.sequence_engine_for(t, rig, img, 32)
    assert both.kwargs["subpix"] == 3 and both.kwargs["ratio_f2f"]


def test_the_mirror_path_keys_its_front_end_by_the_setting(monkeypatch):
    """GUMStereo._front_end / _detect_both: one ImageFrontEnd per (method, features, median, subpix), and the detection cache
    of an omni image does not outlive a change of the setting."""
    from vo_single_camera_sos_amd import frontend
    from vo_single_camera_sos_amd.omnistereo.gum import GUMStereo
    built = []
    monkeypatch.setattr(frontend, "ImageFrontEnd", lambda *a, **k: built.append(k) or SimpleNamespace(**k))
    rig = GUMStereo.__new__(GUMStereo)
    rig._front_ends, rig._context, rig._device_model = {}, lambda: None, lambda: None
    rig.feature_matcher_for_static_stereo = fm = SimpleNamespace()
    a = rig._front_end("GFT", 100, 11)
    fm.subpix_half = 3
    b = rig._front_end("GFT", 100, 11)
    assert a is not b and rig._front_end("gft", 100, 11) is b and (a.subpix, b.subpix) == (None, 3) and len(built) == 2
    fm.subpix_half = None
    assert rig._front_end("GFT", 100, 11) is a


def test_run_VO_refuses_bad_arguments_before_any_frame(tmp_path):
    from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
    cam = rgbd_cam()
    frames = lambda: iter(())                                  # noqa: E731
    with pytest.raises(ValueError, match="integer pixels"):
        pet.run_VO(None, cam, results_path=str(tmp_path), _live_frames=frames, subpix_refine=True)
    with pytest.raises(ValueError, match="subpix"):
        pet.run_VO(None, cam, results_path=str(tmp_path), _live_frames=frames, subpix_refine="on")


def test_the_demos_and_the_c_example_name_the_option():
    root = os.path.dirname(os.path.dirname(_lib.HEADER_PATH))
    for name in ("demo_vo_sos.py", "demo_vo_rgbd.py", "demo_vo_sos_live.py"):
        text = open(os.path.join(root, name)).read()
        assert '"--subpix_refine"' in text and '"--subpix_half"' in text and "subpix_refine=" in text \
            and "subpix_half=args.subpix_half" in text, name
    assert "SOSVO_FLAG_SUBPIX" in open(os.path.join(root, "examples", "c_abi_batch.c")).read()
