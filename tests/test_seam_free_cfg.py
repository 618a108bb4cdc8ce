"""CPU (library and headers only, no GPU): the configuration layers of the seam-free front end -- the
header's defines and entry points against the ctypes table and the Context methods, SOSVO_FLAG_SEAM_FREE as the sign bit of
the omni word, workspace sizes with the flag clear (what they were), set and set with LK_F2F, every refusal as a size of 0, the
Python constructors' refusals before any device call (the recording fake context of tests/test_lk_layers_cfg.py), what the
pair pipeline and a sequence engine ask their context with the option off, StepOptions, the engine key, run_VO / the drivers /
the demos, and the RGB-D refusals."""
import ctypes
import inspect
import re
from types import SimpleNamespace

import numpy as np
import pytest

import cfg_fakes
from cfg_fakes import cfg, rgbd_cfg
from test_cyclic_cfg import _recorded, _same
from test_lk_layers_cfg import OMNI, SIZES_BEFORE, SMALL, _drive, _Recorder, _rig, _sizes, _tensors, host_only  # noqa: F401
from vo_single_camera_sos_amd import _lib, pipeline
from vo_single_camera_sos_amd.device import Context
from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet

CYC, SF, LK = _lib.FLAG_CYCLIC_F2F, _lib.FLAG_SEAM_FREE, _lib.FLAG_LK_F2F
STAGES = ("sosvo_unwrap_prepare_seam_free", "sosvo_mask_bits_seam_free", "sosvo_keypoints_unpad", "sosvo_gray_unpad")
LK2 = dict(half=4, levels=2, max_iter=10, fb_max=0.5)      # (the fakes' panoramas have 40 columns)


def _flat_header():
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S))


def test_the_header_declares_the_defines_and_the_entry_points():
    text, flat = open(_lib.HEADER_PATH).read(), _flat_header()
    assert re.search(r"^#define SOSVO_SEAM_HALO 40\s*$", text, flags=re.M) and _lib.SEAM_HALO == 40
    assert "#define SOSVO_FLAG_SEAM_FREE ((int32_t)(-2147483647 - 1))" in text
    for proto in ("int32_t sosvo_unwrap_prepare_seam_free(sosvo_ctx* ctx, const uint8_t* masks, const float* map_x, const float* map_y, "
                  "int32_t H, int32_t W, int32_t rows, int32_t cols, uint32_t* table);",
                  "int32_t sosvo_mask_bits_seam_free(sosvo_ctx* ctx, const uint32_t* mask_bits, int32_t nsets, int32_t rows, int32_t cols, "
                  "uint32_t* out);",
                  "int32_t sosvo_keypoints_unpad(sosvo_ctx* ctx, float* kp, const int32_t* n, int32_t nprob, int32_t cap, int32_t period);",
                  "int32_t sosvo_gray_unpad(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols, "
                  "const int32_t* row_range, uint8_t* out);"):
        assert proto in flat, proto
    declared = _lib.declared_functions()
    for name in STAGES:
        assert name in declared and name in _lib.SIGNATURES
        n_args = len(re.search(r"\b%s\(([^;]*?)\);" % name, flat).group(1).split(","))
        assert len(_lib.SIGNATURES[name][1]) == n_args and _lib.SIGNATURES[name][0] is _lib.c_i32
    assert _lib.SIGNATURES["sosvo_unwrap_prepare_seam_free"] == _lib.SIGNATURES["sosvo_unwrap_prepare"]
    # the comment says what the bit is and what comes next
    assert "sign bit" in text and "second word" in text


def test_the_flag_is_the_sign_bit_and_overlaps_nothing():
    assert SF == -2 ** 31 and ctypes.c_int32(SF).value == SF and ctypes.c_uint32(SF).value == 0x80000000
    others = 0
    for name in ("FLAG_CAM_ROT_IDENTITY", "FLAG_EPNP", "FLAG_GP3P", "FLAG_TWOPT", "FLAG_RATIO_STEREO", "FLAG_RATIO_F2F", "FLAG_SUBPIX",
                 "FLAG_LK_F2F", "FLAG_LK_STEREO", "FLAG_CYCLIC_F2F", "FLAG_CROSS_CHECK_STEREO", "FLAG_CROSS_CHECK_F2F",
                 "FLAG_GATED_STEREO", "FLAG_GATED_F2F", "SUBPIX_HALF_MASK", "GATED_MAX_DIST_MASK", "RATIO_64THS_MASK"):
        assert SF & getattr(_lib, name) == 0, name
        others |= getattr(_lib, name)
    assert others == 0x7FFFFFFF                                      # the word is full: the sign bit was its last free one
    assert len(_lib.BatchCfg._fields_) == 22                         # the struct has not grown
    c = cfg(flags=SF | CYC | (63 << _lib.RATIO_64THS_SHIFT))         # the fields beside it read as they did
    assert c.ransac_flags < 0 and (c.ransac_flags & _lib.RATIO_64THS_MASK) >> _lib.RATIO_64THS_SHIFT == 63


def test_the_library_exports_the_stages_and_they_refuse_null():
    lib = cfg_fakes.lib_or_skip()
    for name in STAGES:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.sosvo_unwrap_prepare_seam_free(None, None, None, None, 4, 4, 4, 48, None) == -1
    assert lib.sosvo_mask_bits_seam_free(None, None, 2, 4, 48, None) == -1
    assert lib.sosvo_keypoints_unpad(None, None, None, 1, 1, 48) == -1
    assert lib.sosvo_gray_unpad(None, None, 2, 4, 48, None, None) == -1


def test_the_context_has_the_four_methods():
    assert list(inspect.signature(Context.unwrap_prepare_seam_free).parameters) == list(inspect.signature(Context.unwrap_prepare).parameters)
    assert list(inspect.signature(Context.mask_bits_seam_free).parameters)[1:] == ["mask_bits", "out"]
    assert list(inspect.signature(Context.keypoints_unpad).parameters)[1:] == ["kp", "n", "period"]
    sig = inspect.signature(Context.gray_unpad).parameters
    assert list(sig)[1:] == ["gray", "cols", "row_range", "out"] and sig["row_range"].default is None


# ---- workspace sizes and refusals --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,pair_bytes,seq_bytes", SIZES_BEFORE)
def test_workspace_sizes_clear_set_and_with_the_tracker(kw, pair_bytes, seq_bytes):
    lib, B = cfg_fakes.lib_or_skip(), kw["n_pairs"]
    assert _sizes(lib, cfg(**kw), B) == (pair_bytes, seq_bytes)                     # flag clear: what they were
    if kw["detector"] == _lib.DETECTOR_ORB:                                         # (refused with the flag)
        assert _sizes(lib, cfg(**dict(kw, flags=kw["flags"] | CYC | SF)), B) == (0, 0)
        return
    c0 = cfg(**dict(kw, flags=kw["flags"] | CYC))
    c1 = cfg(**dict(kw, flags=kw["flags"] | CYC | SF))
    clear, on = _sizes(lib, c0, B), _sizes(lib, c1, B)
    assert clear == (pair_bytes, seq_bytes)
    # set: the gray panoramas of the window are 80 columns wider (2 * window images of `rows` rows)
    # (every buffer of the workspace is 256-byte aligned: the one buffer that changes moves the total by its bytes +- 255)
    assert on[0] > clear[0] and on[1] > clear[1]
    assert abs(on[0] - clear[0] - 4 * B * c0.rows * 80) < 256 and abs(on[1] - clear[1] - 2 * B * c0.rows * 80) < 256
    if kw["flags"] & _lib.FLAG_CROSS_CHECK_F2F:
        return
    lk0, lk1 = _sizes(lib, cfg(**dict(kw, flags=kw["flags"] | CYC | LK)), B), _sizes(lib, cfg(**dict(kw, flags=kw["flags"] | CYC | SF | LK)), B)
    assert lk1[0] > on[0] and lk1[1] > on[1]                                        # larger again with the tracker
    # a pair batch can no longer use the front end's buffer in place: it grows by one level 0 (and the wider gray)
    level0 = 4 * B * c0.rows * c0.cols
    assert abs(lk1[0] - lk0[0] - (level0 + 4 * B * c0.rows * 80)) < 512
    assert lk1[1] - lk0[1] == on[1] - clear[1]                                      # (a sequence store always had its own)
    for ns in (1, 2):
        assert lib.sosvo_frame_pair_batch_streams_workspace(ctypes.byref(c1), ns) > lib.sosvo_frame_pair_batch_streams_workspace(ctypes.byref(c0), ns) > 0


def test_every_refusal_has_no_workspace():
    lib = cfg_fakes.lib_or_skip()
    r48 = 48 << _lib.RATIO_64THS_SHIFT

    def sizes(flags, detector=0, cols=1200, edge=31):
        c = cfg(flags=flags, detector=detector)
        c.cols, c.edge = cols, edge
        return _sizes(lib, c, 4) + (lib.sosvo_frame_pair_batch_streams_workspace(ctypes.byref(c), 2),)
    assert all(v > 0 for v in sizes(SF | CYC))
    assert sizes(SF) == (0, 0, 0)                                                   # without SOSVO_FLAG_CYCLIC_F2F
    assert sizes(SF | CYC, detector=_lib.DETECTOR_ORB) == (0, 0, 0)
    for det in (_lib.DETECTOR_FAST, _lib.DETECTOR_AGAST):
        assert all(v > 0 for v in sizes(SF | CYC, detector=det))
    assert sizes(SF | CYC, edge=32) == (0, 0, 0) and all(v > 0 for v in sizes(SF | CYC, edge=16))
    assert all(v > 0 for v in sizes(CYC, edge=32))                                  # (the flag's rule, not the plain path's)
    assert sizes(SF | CYC, cols=39) == (0, 0, 0) and all(v > 0 for v in sizes(SF | CYC, cols=40))
    assert sizes(SF | CYC, cols=16305) == (0, 0, 0) and all(v > 0 for v in sizes(SF | CYC, cols=16304))
    # every refusal SOSVO_FLAG_CYCLIC_F2F already has
    assert sizes(SF | CYC | LK, cols=1444) == (0, 0, 0) and all(v > 0 for v in sizes(SF | CYC | LK, cols=1440))
    assert sizes(SF | CYC | _lib.FLAG_GATED_F2F | _lib.FLAG_RATIO_F2F | r48) == (0, 0, 0)
    assert sizes(SF | CYC | LK | _lib.FLAG_GATED_F2F) == (0, 0, 0)
    for ok in (_lib.FLAG_GATED_F2F, _lib.FLAG_SUBPIX, _lib.FLAG_LK_STEREO, _lib.FLAG_CROSS_CHECK_STEREO, _lib.FLAG_GP3P):
        assert all(v > 0 for v in sizes(SF | CYC | ok)), hex(ok)
    # RGB-D has no such bit
    c = rgbd_cfg(SF)
    assert lib.sosvo_rgbd_pair_batch_workspace(ctypes.byref(rgbd_cfg())) > 0


# ---- StepOptions ---------------------------------------------------------------------------------------------------------------
def test_step_options_normalise_and_round_trip():
    S = _lib.StepOptions
    assert S().cyclic is False and S(cyclic=1).cyclic is True and S(cyclic=0).cyclic is False and S(cyclic=None).cyclic is False
    assert S(cyclic="seam_free").cyclic == "seam_free" and S(cyclic="seam_free").seam_free and not S(cyclic=True).seam_free
    with pytest.raises(ValueError, match="seam_free"):
        S(cyclic="seamless")
    assert len(S()) == 5 and S._fields == ("match", "subpix", "lk", "stereo_lk", "cyclic")        # no sixth field
    assert S().flags() == 0 and S(cyclic=True).flags() == CYC and S(cyclic="seam_free").flags() == CYC | SF
    assert ctypes.c_int32(S(cyclic="seam_free").flags()).value == CYC | SF
    assert "cyclic_columns" not in S().kwargs() and S(cyclic=True).kwargs()["cyclic_columns"] is True
    assert S(cyclic="seam_free").kwargs()["cyclic_columns"] == "seam_free"
    for value in (False, True, "seam_free"):
        so = S.of(cyclic_columns=value, rig=(1440, 1440), subpix=3)
        assert so.cyclic == value and S.of(rig=(1440, 1440), **so.kwargs()) == so
    assert hash(S(cyclic="seam_free")) != hash(S(cyclic=True)) and S(cyclic="seam_free") != S(cyclic=True)
    # of() runs the new checks in the cyclic slot
    for bad, word in ((dict(rig=(39, 39)), "39"), (dict(rig=(16305, 16305)), "16305"), (dict(rig=(1440, 1448)), "one width"),
                      (dict(rig=(1440, 1440), detection_method="ORB"), "ORB"), (dict(rig=(1440, 1440), edge=32), "edge"),
                      (dict(rig=(1440, 1440), gray=False), "front end"),
                      (dict(rig=(1440, 1440), stereo_refine="lk", stereo_lk=dict(half=10, max_shift=24)), "max_shift"),
                      (dict(rig=(1442, 1442), f2f_tracker="lk"), "1442")):
        with pytest.raises(ValueError, match=word):
            S.of(cyclic_columns="seam_free", **bad)
        if word not in ("1442",):
            S.of(cyclic_columns=True, **{k: v for k, v in bad.items() if k not in ("detection_method", "edge", "gray")})
    assert S.of(cyclic_columns="seam_free", rig=(1440, 1440), stereo_refine="lk", stereo_lk=dict(half=10, max_shift=23)).seam_free
    for more in (dict(order=S.PAIR_ORDER, tracker_sees_match=False), dict(order=S.BATCH_ORDER)):   # (the settings parsed after / before)
        with pytest.raises(ValueError, match="max_shift"):
            S.of(cyclic_columns="seam_free", rig=(1440, 1440), stereo_refine="lk", stereo_lk=dict(half=10, max_shift=24), **more)
    with pytest.raises(ValueError, match="cyclic"):
        S.rgbd(cyclic_columns="seam_free")


# ---- the constructors ----------------------------------------------------------------------------------------------------------
def _model(cols=40):
    """The fakes' model with a seam-free form that asks nothing of the device."""
    form = SimpleNamespace(unwrap_table_run="TABLE+80", mask_bits_run="BITS+80")
    return SimpleNamespace(H=12, W=16, rows=10, cols=cols, nmask=3, unwrap_table="TABLE", mask_bits="BITS", pattern="PATTERN", omni_masks=None,
                           map_x=None, map_y=None, seam_free_form=lambda ctx: form)


@pytest.mark.parametrize("cls,kw", OMNI, ids=[c.__name__ for c, _ in OMNI])
def test_omni_constructors_take_and_refuse_the_option_before_the_device(cls, kw, host_only):  # noqa: F811
    new = lambda rig=None, **more: cls(_Recorder(), _model(), rig or _rig(), **kw, **SMALL, **more)  # noqa: E731
    assert new().cfg.ransac_flags & (SF | CYC) == 0 and new(cyclic_columns=True).cfg.ransac_flags & (SF | CYC) == CYC
    on = new(cyclic_columns="seam_free")
    assert on.cfg.ransac_flags & (SF | CYC) == SF | CYC and on.cfg.cols == 40              # cols stays the period
    assert new(cyclic_columns="seam_free", f2f_tracker="lk", lk=LK2).cfg.ransac_flags & LK
    for det in ("FAST", "AGAST"):
        assert new(cyclic_columns="seam_free", detection_method=det).cfg.ransac_flags & SF
    geo = lambda w: (w, 10.0, 0.005, 1.2)  # noqa: E731
    narrow = pipeline.RigConfig(geo(32.0), geo(32.0), (0, 0, 100.0), (0, 0, -100.0), 500.0, 7000.0)
    for rig, bad, word in ((None, dict(detection_method="ORB"), "ORB"), (None, dict(edge=32), "edge"), (narrow, {}, "32"),
                           (None, dict(stereo_refine="lk", stereo_lk=dict(half=10, max_shift=30)), "max_shift"),
                           (None, dict(gated_f2f=True, ratio_f2f=True, ratio=0.75), "ratio"),
                           (None, dict(f2f_tracker="lk", lk=dict(half=4, levels=3)), "40")):
        ctx = _Recorder()
        with pytest.raises(ValueError, match=word):
            cls(ctx, _model(), rig or _rig(), **kw, **SMALL, cyclic_columns="seam_free", **bad)
        assert ctx.calls == []                                       # nothing was asked of the device
    with pytest.raises(ValueError, match="seam_free"):
        new(cyclic_columns="seamless")


def test_a_batch_hands_the_padded_constants_only_with_the_option(host_only):  # noqa: F811
    seen = []

    class Ctx(_Recorder):
        def frame_pair_batch(self, rig, cfg_, omni, table, bits, pattern, ws, **kw):
            seen.append((table, bits, pattern, cfg_.ransac_flags & (SF | CYC)))

        def sequence_front_end(self, rig, cfg_, window, slots, omni, first, table, bits, pattern, ws):
            seen.append((table, bits, pattern, cfg_.ransac_flags & (SF | CYC)))
    for value, want in ((False, ("TABLE", "BITS", "PATTERN", 0)), (True, ("TABLE", "BITS", "PATTERN", CYC)),
                        ("seam_free", ("TABLE+80", "BITS+80", "PATTERN", SF | CYC))):
        del seen[:]
        b = pipeline.FramePairBatch(Ctx(), _model(), _rig(), 2, cyclic_columns=value, **SMALL)
        b.step()
        b.enqueue()
        eng = pipeline.SequenceEngine(Ctx(), _model(), _rig(), window=2, cyclic_columns=value, **SMALL)
        eng.push_window([np.zeros((12, 16, 3), np.uint8)] * 2)
        assert seen == [want] * 3, value


def test_overlapped_pairs_and_the_pair_pipeline_refuse_before_the_device():
    for bad in (dict(detection_method="ORB"), dict(stereo_refine="lk", stereo_lk=dict(half=10, max_shift=30))):
        with pytest.raises(ValueError, match="seam_free"):
            pipeline.OverlappedFramePairs(0, None, (12, 16), _rig(), 2, cyclic_columns="seam_free", **bad)
    from test_lk_cfg import _ctx, _front_end
    from test_lk_cfg import _rig as wide_rig
    with pytest.raises(ValueError, match="front end"):                               # no front end at all
        pipeline.FramePairPipeline(_ctx(), wide_rig(), 2, frame_cap=16, cyclic_columns="seam_free")
    with pytest.raises(ValueError, match="seam_free_form"):                          # a plain front end
        pipeline.FramePairPipeline(_ctx(), wide_rig(), 2, frame_cap=16, front_end=_front_end(), cyclic_columns="seam_free")
    fe = _front_end()
    fe.seam_free = True
    with pytest.raises(ValueError, match="seam_free_form"):                          # ... and the other way round
        pipeline.FramePairPipeline(_ctx(), wide_rig(), 2, frame_cap=16, front_end=fe, cyclic_columns=True)
    fe.method = "ORB"
    with pytest.raises(ValueError, match="ORB"):
        pipeline.FramePairPipeline(_ctx(), wide_rig(), 2, frame_cap=16, front_end=fe, cyclic_columns="seam_free")
    fe.method = "GFT"
    assert pipeline.FramePairPipeline(_ctx(), wide_rig(), 2, frame_cap=16, front_end=fe, cyclic_columns="seam_free").cyclic == "seam_free"


def test_the_pair_pipeline_unpads_after_its_stereo_step_and_tracks_on_the_interior():
    import torch
    from test_lk_cfg import _ctx, _front_end
    from test_lk_cfg import _rig as wide_rig
    fe, ctx, calls = _front_end(), _ctx(), []
    fe.seam_free, fe.method, fe.edge = True, "GFT", 31
    fe.run = lambda unpad=True: calls.append(("run", unpad))
    fe.unpad = lambda: calls.append(("unpad",))
    fe.gray_interior = lambda out=None: calls.append(("gray_interior", out)) or "INTERIOR"
    pipe = pipeline.FramePairPipeline(ctx, wide_rig(), 2, frame_cap=16, front_end=fe, cyclic_columns="seam_free", f2f_tracker="lk",
                                      lk=dict(half=4, levels=2), stereo_refine="lk")
    for name in ("match_1nn_two_launch", "sort_matches", "refine_stereo_lk", "stereo_assemble", "f2f_assemble_tracked", "ransac_abs_pose",
                 "refine_abs_pose"):
        setattr(ctx, name, lambda *a, _n=name, **k: calls.append((_n,)))
    ctx.gray_pyramid_cyclic = lambda gray, levels, **k: calls.append(("gray_pyramid_cyclic", gray)) or "CPYR"
    ctx.track_lk = lambda *a, **k: calls.append(("track_lk", a[0])) or k["out"]
    pipe._M2[0].copy_(torch.tensor([5, 6, 7, 8], dtype=torch.int32))
    pipe.step()
    assert [c[0] for c in calls] == ["run", "match_1nn_two_launch", "sort_matches", "refine_stereo_lk", "unpad", "stereo_assemble",
                                     "gray_interior", "gray_pyramid_cyclic", "track_lk", "f2f_assemble_tracked", "ransac_abs_pose",
                                     "refine_abs_pose"]
    assert calls[0] == ("run", False) and calls[7] == ("gray_pyramid_cyclic", "INTERIOR") and calls[8] == ("track_lk", "CPYR")
    del calls[:]
    pipe.step()
    assert ("gray_interior", "INTERIOR") in calls                                    # the buffer is reused


@pytest.mark.parametrize("kw", [{}, dict(gated_f2f=True, gated_max_distance=64), dict(f2f_tracker="lk", lk=dict(half=4, levels=2, fb_max=0.5))])
@pytest.mark.parametrize("value", [False, True])
def test_with_the_option_off_or_plain_the_pipeline_asks_what_it_asks_today(kw, value):
    """cyclic_columns False / True: the calls of the constructor that has never heard of "seam_free" (for True: of True itself,
    through the normalised value), argument for argument, and no seam-free stage among them."""
    a, calls_a = _recorded(dict(kw, **({"cyclic_columns": True} if value else {})))
    b, calls_b = _recorded(dict(kw, cyclic_columns=value))
    assert a.cyclic is value and b.cyclic is value
    assert [c[0] for c in calls_a] == [c[0] for c in calls_b]
    for (_, aa, ka), (_, ab, kb) in zip(calls_a, calls_b):
        assert _same(aa, ab) and _same(ka, kb)
    assert not hasattr(b, "_lk_gray")


def test_with_the_option_off_or_plain_an_engine_asks_what_it_asks_today(host_only):  # noqa: F811
    from test_lk_layers_cfg import _model as plain_model       # (a model that has never heard of a seam-free form)
    for value, flags in ((False, _lib.FLAG_GP3P), (True, _lib.FLAG_GP3P | CYC)):
        eng = pipeline.SequenceEngine(_Recorder(), plain_model(), _rig(), window=2, cyclic_columns=value, **SMALL)
        calls = _drive(eng)
        assert [c[0] for c in calls] == ["sequence_workspace", "sequence_front_end", "sequence_track", "sequence_frame_counts",
                                         "sequence_front_end", "sequence_track", "sequence_track", "sequence_frame_counts",
                                         "sequence_copy_slot", "sequence_track"]
        assert {c[1] for c in calls} == {flags} and eng.fam.consts() == (eng.model.unwrap_table, None, None)
    on = pipeline.SequenceEngine(_Recorder(), _model(), _rig(), window=2, cyclic_columns="seam_free", **SMALL)
    off = pipeline.SequenceEngine(_Recorder(), _model(), _rig(), window=2, **SMALL)
    assert {c[1] for c in _drive(on)} == {_lib.FLAG_GP3P | CYC | SF}
    assert (_tensors(on), _tensors(on.fam)) == (_tensors(off), _tensors(off.fam))      # no new Python-side buffers


# ---- the trackers' setters, the engine key, the drivers ------------------------------------------------------------------------------
def test_set_cyclic_columns_and_the_engine_key():
    t, rig, img = cfg_fakes.tracker(rgbd=False), cfg_fakes.Rig(), np.zeros((480, 640, 3), np.uint8)
    t.camera_model = rig
    off = pet._sos_engine_settings(t, rig, img)
    pet.set_cyclic_columns(t, True)
    plain = pet._sos_engine_settings(t, rig, img)
    pet.set_cyclic_columns(t, "seam_free")
    on = pet._sos_engine_settings(t, rig, img)
    assert rig.cyclic_columns == "seam_free" and t.cyclic_columns == "seam_free" and on[1]["cyclic_columns"] == "seam_free"
    assert len({off[2], plain[2], on[2]}) == 3 and plain[1]["cyclic_columns"] is True
    pet.set_cyclic_columns(t, False)
    assert rig.cyclic_columns is False and pet._sos_engine_settings(t, rig, img)[2] == off[2]
    with pytest.raises(ValueError, match="seam_free"):
        pet.set_cyclic_columns(t, "seamless")
    orb = cfg_fakes.tracker(rgbd=False, method="ORB")
    orb.camera_model = cfg_fakes.Rig()
    with pytest.raises(ValueError, match="ORB"):
        pet.set_cyclic_columns(orb, "seam_free")
    r = cfg_fakes.tracker(rgbd=True)
    r.camera_model = cfg_fakes.rgbd_cam()
    with pytest.raises(ValueError, match="cyclic"):
        pet.set_cyclic_columns(r, "seam_free")


def test_rgbd_constructors_refuse_the_option():
    cam = pipeline.RGBDCamConfig(fx=500.0, fy=500.0, center_x=8.0, center_y=6.0)
    for cls, kw in ((pipeline.RGBDPairBatch, dict(n_pairs=2)), (pipeline.RGBDSequenceEngine, dict(window=2)),
                    (pipeline.RGBDMultiSequenceEngine, dict(lanes=2, window=2))):
        ctx = _Recorder()
        with pytest.raises(ValueError, match="cyclic"):
            cls(ctx, cam, image_shape=(12, 16), cyclic_columns="seam_free", **kw)
        assert ctx.calls == []


def test_run_vo_the_drivers_and_the_demos_take_the_option():
    import demo_vo_sos
    import demo_vo_sos_live
    for fn in (pet.run_VO, pet.run_VO_many, pet.run_VO_live, pet.driver_VO, pet.driver_VO_many, pet.driver_VO_live):
        assert inspect.signature(fn).parameters["cyclic_columns"].default is None, fn.__name__
    assert '"seam_free"' in inspect.getsource(pet.set_cyclic_columns)
    for demo in (demo_vo_sos, demo_vo_sos_live):
        parser = demo.build_parser()
        args = parser.parse_args(["somewhere", "--seam_free"])
        assert args.seam_free is True and args.cyclic_columns is False                # (--seam_free implies the other)
        assert parser.parse_args(["somewhere"]).seam_free is False
        assert 'cyclic_columns="seam_free" if args.seam_free else' in inspect.getsource(demo)


def test_the_mirror_path_front_end_follows_the_camera_model():
    """GUMStereo._front_end: a front end of its own per setting, over the model's seam-free form when the option is set."""
    from vo_single_camera_sos_amd import frontend
    from vo_single_camera_sos_amd.omnistereo.gum import GUMStereo
    built = []
    rig = GUMStereo.__new__(GUMStereo)
    rig._front_ends, rig.feature_matcher_for_static_stereo = {}, None
    rig._context = lambda: "ctx"
    rig._device_model = lambda: SimpleNamespace(seam_free_form=lambda ctx: "FORM")
    real = frontend.ImageFrontEnd
    frontend.ImageFrontEnd = lambda ctx, model, n, **kw: built.append(model) or SimpleNamespace(model=model)
    try:
        plain = rig._front_end("GFT", 100, 11)
        rig.cyclic_columns = True
        assert rig._front_end("GFT", 100, 11) is plain
        rig.cyclic_columns = "seam_free"
        sf = rig._front_end("GFT", 100, 11)
        assert sf is not plain and sf.model == "FORM" and rig._front_end("GFT", 100, 11) is sf
        rig.cyclic_columns = False
        assert rig._front_end("GFT", 100, 11) is plain and len(built) == 2
    finally:
        frontend.ImageFrontEnd = real
