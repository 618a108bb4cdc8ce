"""CPU: the configuration layers of the sub-pixel static stereo (sosvo_refine_stereo_lk, SOSVO_FLAG_LK_STEREO) -- the header
and the bindings, the options' validation, the workspace sizes with the bit clear (constants) and set, what the pair pipeline
and the engines ask of their context with the option off (what they asked before) and on, the RGB-D refusals, run_VO's layers
and the demos' flags."""
import ctypes
import inspect
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cfg_fakes
from cfg_fakes import cfg, lib_or_skip
from test_lk_layers_cfg import OMNI, SIZES_BEFORE, SMALL, _drive, _model, _record, _Recorder, _rig, _sizes, _tensors, host_only  # noqa: F401
from vo_single_camera_sos_amd import _lib, pipeline
from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet

SLK = dict(half=3, max_iter=12, max_shift=1.5)


class _Rec(_Recorder):
    def set_stereo_lk_options(self, stereo_lk=None):
        self.stereo_lk_options = _lib.StereoLKOptions.of(stereo_lk)
        self.calls.append(("set_stereo_lk_options", self.stereo_lk_options))


for _name in ("match_1nn_two_launch", "sort_matches", "stereo_assemble", "refine_stereo_lk"):
    setattr(_Rec, _name, _record(_name))


# ---- the header and the bindings ---------------------------------------------------------------------------------------------
def test_header_declares_the_stage_and_the_bindings_match():
    text = open(_lib.HEADER_PATH).read()
    assert "#define SOSVO_FLAG_LK_STEREO 0x100" in text and _lib.FLAG_LK_STEREO == 0x100
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert ("typedef struct sosvo_stereo_lk_options { int32_t half, max_iter; double eps, min_eig, max_shift; } "
            "sosvo_stereo_lk_options;") in flat
    assert "int32_t sosvo_set_stereo_lk_options(sosvo_ctx* ctx, const sosvo_stereo_lk_options* options);" in flat
    assert ("int32_t sosvo_refine_stereo_lk(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols, "
            "const int32_t* row_range, int32_t nmask, int32_t cap, const float* kp_top, const int32_t* n_top, float* kp_bot, "
            "const int32_t* n_bot, const uint32_t* keys, double stereo_min_disp, double stereo_max_hdiff, "
            "const sosvo_stereo_lk_options* options, uint8_t* status);") in flat
    i, f, p = _lib.c_i32, _lib.c_f64, _lib.c_p
    assert _lib.SIGNATURES["sosvo_refine_stereo_lk"] == (i, [p, p, i, i, i, p, i, i, p, p, p, p, p, f, f, p, p])
    assert _lib.SIGNATURES["sosvo_set_stereo_lk_options"] == (i, [p, p])
    assert {"sosvo_refine_stereo_lk", "sosvo_set_stereo_lk_options"} <= set(_lib.declared_functions())
    S = _lib.StereoLkOptionsStruct
    assert ctypes.sizeof(S) == 32
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("half", 0), ("max_iter", 4), ("eps", 8), ("min_eig", 16),
                                                                 ("max_shift", 24)]
    assert "#define SOSVO_STEREO_LK_OPTIONS_DEFAULT {4, 30, 0.01, 1e-4, 0.0}" in text           # ... StereoLKOptions' defaults
    d = S.of(_lib.StereoLKOptions())
    assert (d.half, d.max_iter, d.eps, d.min_eig, d.max_shift) == (4, 30, 0.01, 1e-4, 0.0)        # (None -> 0: half)
    st = S.of(_lib.StereoLKOptions(**SLK))
    assert (st.half, st.max_iter, st.eps, st.min_eig, st.max_shift) == (3, 12, 0.01, 1e-4, 1.5)
    lib = lib_or_skip()
    assert lib.sosvo_set_stereo_lk_options(None, None) == -1
    assert lib.sosvo_refine_stereo_lk(None, None, 2, 8, 8, None, 1, 4, None, None, None, None, None, 1.0, 2.5, None, None) == -1


def test_the_bit_collides_with_no_omni_option():
    """Bits 8 - 9 belong to the detector in the RGB-D word only; every option of the omni word lies elsewhere."""
    omni = (_lib.FLAG_CAM_ROT_IDENTITY | _lib.FLAG_EPNP | _lib.FLAG_GP3P | _lib.FLAG_TWOPT | _lib.FLAG_CROSS_CHECK_STEREO |
            _lib.FLAG_CROSS_CHECK_F2F | _lib.FLAG_GATED_STEREO | _lib.FLAG_GATED_F2F | _lib.GATED_MAX_DIST_MASK | _lib.FLAG_RATIO_STEREO |
            _lib.FLAG_RATIO_F2F | _lib.RATIO_64THS_MASK | _lib.FLAG_SUBPIX | _lib.SUBPIX_HALF_MASK | _lib.FLAG_LK_F2F)
    assert omni & _lib.FLAG_LK_STEREO == 0
    assert _lib.RGBD_DETECTOR_MASK & _lib.FLAG_LK_STEREO                  # (why the RGB-D word cannot carry it)
    for kw in (dict(), dict(subpix=5), dict(ratio_stereo=True, ratio_f2f=True, ratio=63 / 64.0), dict(gated_stereo=True, gated_max_distance=256),
               dict(lk=_lib.LKOptions())):
        c = pipeline.batch_cfg(_model(), 2, 20, 32, 64, 11, 0.01, 5.0, 31, None, 100, False, 0, 5, "GP3P", "GFT", **kw)
        assert c.ransac_flags & _lib.FLAG_LK_STEREO == 0
        on = pipeline.batch_cfg(_model(), 2, 20, 32, 64, 11, 0.01, 5.0, 31, None, 100, False, 0, 5, "GP3P", "GFT",
                                stereo_lk=_lib.StereoLKOptions(), **kw)
        assert on.ransac_flags == c.ransac_flags | _lib.FLAG_LK_STEREO


# ---- the options ---------------------------------------------------------------------------------------------------------------
def test_option_validation():
    O = _lib.StereoLKOptions
    assert tuple(O()) == (4, 30, 0.01, 1e-4, None) and O().bound == 4.0 and O(half=7, max_shift=0).bound == 7.0
    assert O(max_shift=0.25).bound == 0.25 and O.of(None) == O() and O.of(SLK) == O(**SLK) and O.of(O(**SLK)) is not None
    for bad in (dict(half=1), dict(half=11), dict(half=4.5), dict(half=True), dict(half="4"), dict(max_iter=0), dict(max_iter=31),
                dict(eps=-1e-9), dict(eps=float("nan")), dict(eps=float("inf")), dict(min_eig=-1.0), dict(min_eig=float("inf")),
                dict(max_shift=-0.1), dict(max_shift=float("nan")), dict(max_shift=float("inf")), dict(max_shift=True),
                dict(max_shift="1")):
        with pytest.raises(ValueError):
            O(**bad)
    for bad in (dict(window=4), 5, "lk"):
        with pytest.raises(ValueError):
            O.of(bad)
    assert O(half=10.0).half == 10 and isinstance(O(half=10.0).half, int)       # (an integral float is an integer; nothing is rounded)
    f = _lib.stereo_refine_options
    assert f(None, None) is None and f("lk", None) == O() and f("lk", SLK) == O(**SLK)
    for bad in (("flow", None), (None, SLK), ("lk", dict(half=1)), (True, None)):
        with pytest.raises(ValueError):
            f(*bad)
    with pytest.raises(ValueError):
        f("lk", None, rgbd=True)
    assert f(None, None, rgbd=True) is None


# ---- workspace sizes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,pair_bytes,seq_bytes", SIZES_BEFORE)
def test_workspace_sizes_with_the_bit_clear_are_those_of_before(kw, pair_bytes, seq_bytes):
    """The shapes and the numbers of test_lk_layers_cfg.py (the library before the tracker answered them): the layout has not
    moved.  With the bit set the workspace grows by the stage's status flags, [window * nmask, kp_cap] u8, and by nothing else."""
    lib = lib_or_skip()
    B = kw["n_pairs"]
    assert _sizes(lib, cfg(**kw), B) == (pair_bytes, seq_bytes)
    c = cfg(**dict(kw, flags=kw["flags"] | _lib.FLAG_LK_STEREO))
    on = _sizes(lib, c, B)
    pad = lambda n: (n + 255) & ~255  # noqa: E731
    assert on == (pair_bytes + pad(2 * B * c.nmask * c.kp_cap), seq_bytes + pad(B * c.nmask * c.kp_cap))
    for ns in (1, 2):
        assert lib.sosvo_frame_pair_batch_streams_workspace(ctypes.byref(c), ns) > 0
    both = cfg(**dict(kw, flags=(kw["flags"] & ~_lib.FLAG_CROSS_CHECK_F2F) | _lib.FLAG_LK_STEREO | _lib.FLAG_LK_F2F))
    assert all(v > 0 for v in _sizes(lib, both, B))


# ---- the pair pipeline -----------------------------------------------------------------------------------------------------------
def _front_end(F=4, nmask=3, cap=8):
    P = F * nmask
    z = lambda shape, dt: torch.zeros(shape, dtype=dt)  # noqa: E731
    v = dict(kp_top=z((P, cap, 2), torch.float32), kp_bot=z((P, cap, 2), torch.float32), desc_top=z((P, cap, 32), torch.uint8),
             desc_bot=z((P, cap, 32), torch.uint8), n_top=z((P,), torch.int32), n_bot=z((P,), torch.int32))
    return SimpleNamespace(F=F, model=SimpleNamespace(nmask=nmask), kp_cap=cap, view_arrays=lambda: v, subpix=None,
                           gray=z((2 * F, 10, 40), torch.uint8), keep_panoramas=False, gray_rows="rows")


def test_pair_pipeline_calls_the_stage_between_sort_and_assemble():
    before = ["match_1nn_two_launch", "sort_matches", "stereo_assemble"]
    runs = []
    for more in (dict(), dict(stereo_refine=None), dict(front_end=_front_end()), dict(front_end=_front_end(), subpix=3)):
        p = pipeline.FramePairPipeline(_Rec(), _rig(), 2, nmask=3, bucket_cap=8, frame_cap=64, **more)
        p.stereo()
        assert [c[0] for c in p.ctx.calls] == before and p.stereo_lk is None and not hasattr(p, "s_lk_status")
        runs.append(_tensors(p))
    assert runs[0] == runs[1] and runs[2] == runs[3]
    for opt in (None, SLK):
        p = pipeline.FramePairPipeline(_Rec(), _rig(), 2, frame_cap=64, front_end=_front_end(), stereo_refine="lk", stereo_lk=opt)
        p.stereo()
        assert [c[0] for c in p.ctx.calls] == before[:2] + ["refine_stereo_lk"] + before[2:]
        assert p.stereo_lk == _lib.StereoLKOptions.of(opt)
        extra = set(_tensors(p)) - set(runs[2])
        assert extra == {"s_lk_status"} and _tensors(p)["s_lk_status"] == ((12, 8), torch.uint8)
    for bad in (dict(stereo_refine="lk"), dict(stereo_refine="flow", front_end=_front_end()), dict(stereo_lk=SLK, front_end=_front_end()),
                dict(stereo_refine="lk", stereo_lk=dict(half=11), front_end=_front_end())):
        with pytest.raises(ValueError):
            pipeline.FramePairPipeline(_Rec(), _rig(), 2, nmask=3, bucket_cap=8, frame_cap=64, **bad)
    for bad in (dict(stereo_refine="flow"), dict(stereo_lk=SLK), dict(stereo_refine="lk", stereo_lk=dict(max_shift=-1))):
        with pytest.raises(ValueError):
            pipeline.OverlappedFramePairs(0, None, (12, 16), _rig(), 2, **bad)


# ---- the engines -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,kw", OMNI, ids=[c.__name__ for c, _ in OMNI])
def test_omni_constructors_take_the_option(cls, kw, host_only):  # noqa: F811
    new = lambda **more: cls(_Rec(), _model(), _rig(), **kw, **SMALL, **more)  # noqa: E731
    opt = lambda e: e.stereo_lk if cls is pipeline.FramePairBatch else e.fam.stereo_lk  # noqa: E731
    assert new().cfg.ransac_flags & _lib.FLAG_LK_STEREO == 0 and opt(new()) is None
    on = new(stereo_refine="lk", stereo_lk=SLK, f2f_tracker="lk", subpix=3, cross_check_stereo=True, gated_stereo=True, ratio_stereo=True,
             ratio=0.75)
    assert on.cfg.ransac_flags & _lib.FLAG_LK_STEREO and on.cfg.ransac_flags & _lib.FLAG_LK_F2F and on.cfg.ransac_flags & _lib.FLAG_SUBPIX
    assert opt(on) == _lib.StereoLKOptions(**SLK) and opt(new(stereo_refine="lk")) == _lib.StereoLKOptions()
    for bad in (dict(stereo_refine="flow"), dict(stereo_lk=SLK), dict(stereo_refine="lk", stereo_lk=dict(half=11)),
                dict(stereo_refine="lk", stereo_lk=dict(window=4)), dict(stereo_refine="lk", stereo_lk=5)):
        with pytest.raises(ValueError):
            new(**bad)


def test_with_the_option_off_an_engine_asks_what_it_asked_before(host_only):  # noqa: F811
    """The call list of test_with_the_matcher_an_engine_asks_what_it_asked_before: the same calls, flags and buffers, and no call
    that sets the stage's settings.  With the option on: the same calls under the bit, the settings set once, before the first."""
    want = ["sequence_workspace", "sequence_front_end", "sequence_track", "sequence_frame_counts", "sequence_front_end", "sequence_track",
            "sequence_track", "sequence_frame_counts", "sequence_copy_slot", "sequence_track"]
    runs = []
    for more in ({}, dict(stereo_refine=None)):
        eng = pipeline.SequenceEngine(_Rec(), _model(), _rig(), window=2, **SMALL, **more)
        calls = _drive(eng)
        assert [c[0] for c in calls] == want and {c[1] for c in calls} == {_lib.FLAG_GP3P}
        runs.append((calls, _tensors(eng), _tensors(eng.fam), eng.workspace.numel()))
    assert runs[0] == runs[1]
    eng = pipeline.SequenceEngine(_Rec(), _model(), _rig(), window=2, stereo_refine="lk", stereo_lk=SLK, **SMALL)
    calls = _drive(eng)
    assert [c[0] for c in calls] == ["set_stereo_lk_options"] + want
    assert {c[1] for c in calls if c[0] != "set_stereo_lk_options"} == {_lib.FLAG_GP3P | _lib.FLAG_LK_STEREO}
    assert (_tensors(eng), _tensors(eng.fam)) == runs[0][1:3]
    b = pipeline.FramePairBatch(_Rec(), _model(), _rig(), 2, **SMALL)
    b.step()
    b.enqueue()
    assert b.ctx.calls == [("frame_pair_batch_workspace", 0), ("frame_pair_batch", 0), ("frame_pair_batch", 0)] and b.stereo_lk is None
    # engines that share a context each refine with their own settings
    ctx = _Rec()
    a = pipeline.FramePairBatch(ctx, _model(), _rig(), 2, stereo_refine="lk", stereo_lk=SLK, **SMALL)
    d = pipeline.FramePairBatch(ctx, _model(), _rig(), 2, stereo_refine="lk", **SMALL)
    del ctx.calls[:]
    a.step()
    a.step()
    d.step()
    a.enqueue()
    assert [c[1].half if c[0] == "set_stereo_lk_options" else c[0] for c in ctx.calls] == \
        [3, "frame_pair_batch", "frame_pair_batch", 4, "frame_pair_batch", 3, "frame_pair_batch"]


def test_rgbd_constructors_refuse_the_option():
    cam = pipeline.RGBDCamConfig(fx=500.0, fy=500.0, center_x=8.0, center_y=6.0)
    for cls, kw in ((pipeline.RGBDPairBatch, dict(n_pairs=2)), (pipeline.RGBDSequenceEngine, dict(window=2)),
                    (pipeline.RGBDMultiSequenceEngine, dict(lanes=2, window=2))):
        for bad in (dict(stereo_refine="lk"), dict(stereo_refine="lk", stereo_lk=SLK), dict(stereo_lk=SLK), dict(stereo_refine="flow")):
            with pytest.raises(ValueError):
                cls(_Rec(), cam, image_shape=(12, 16), **kw, **bad)


# ---- run_VO's layers -------------------------------------------------------------------------------------------------------------
def test_set_stereo_refinement_and_the_engine_key():
    t, rig, img = cfg_fakes.tracker(rgbd=False), cfg_fakes.Rig(), np.zeros((480, 640, 3), np.uint8)
    t.camera_model = rig
    fm = rig.feature_matcher_for_static_stereo
    off = pet._sos_engine_settings(t, rig, img)
    assert "stereo_refine" not in off[1] and "stereo_lk" not in off[1]   # the engine is built with what it was built with before
    pet.set_stereo_refinement(t, None)
    assert getattr(fm, "stereo_lk_options", None) is None
    pet.set_stereo_refinement(t, "lk", SLK)
    assert t.stereo_lk_options == fm.stereo_lk_options == _lib.StereoLKOptions(**SLK)
    on = pet._sos_engine_settings(t, rig, img)
    assert on[1]["stereo_refine"] == "lk" and on[1]["stereo_lk"] == _lib.StereoLKOptions(**SLK) and on[2] != off[2]
    pet.set_stereo_refinement(t, "lk", dict(SLK, half=5))
    assert pet._sos_engine_settings(t, rig, img)[2] not in (on[2], off[2])
    pet.set_stereo_refinement(t, "lk")
    assert t.stereo_lk_options == _lib.StereoLKOptions()
    pet.set_stereo_refinement(t, False)
    assert t.stereo_lk_options is None and fm.stereo_lk_options is None and pet._sos_engine_settings(t, rig, img)[2] == off[2]
    for bad in (("flow", None), (None, SLK), (False, SLK), ("lk", dict(half=1))):
        with pytest.raises(ValueError):
            pet.set_stereo_refinement(t, *bad)
    r = cfg_fakes.tracker(rgbd=True)
    r.camera_model = cfg_fakes.rgbd_cam()
    with pytest.raises(ValueError):
        pet.set_stereo_refinement(r, "lk")
    pet.set_stereo_refinement(r, False)
    for fn in (pet.run_VO, pet.run_VO_many, pet.run_VO_live, pet.driver_VO, pet.driver_VO_many, pet.driver_VO_live):
        p = inspect.signature(fn).parameters
        assert p["stereo_refine"].default is None and p["stereo_lk"].default is None, fn.__name__


def test_the_demos_accept_the_flags():
    import demo_vo_sos
    import demo_vo_sos_live
    from vo_single_camera_sos_amd.omnistereo.common_tools import stereo_refine_arguments
    for demo in (demo_vo_sos, demo_vo_sos_live):
        parser = demo.build_parser()
        args = parser.parse_args(["somewhere", "--stereo_refine", "lk", "--stereo_lk_half", "3", "--stereo_lk_max_shift", "1.5"])
        assert stereo_refine_arguments(args) == dict(stereo_refine="lk", stereo_lk=dict(half=3, max_shift=1.5))
        assert stereo_refine_arguments(parser.parse_args(["somewhere"])) == dict(stereo_refine=None, stereo_lk=None)
        assert stereo_refine_arguments(parser.parse_args(["somewhere", "--stereo_refine", "lk"])) == dict(stereo_refine="lk", stereo_lk=None)
        with pytest.raises(SystemExit):
            parser.parse_args(["somewhere", "--stereo_refine", "flow"])
