"""CPU: the configuration layers of Lucas-Kanade tracking in the one-call batches, the sequence engines and run_VO -- the
header and the bindings of sosvo_lk_options / sosvo_set_lk_options / SOSVO_FLAG_LK_F2F, the workspace sizes with the bit clear
(constants) and set (the store's images), the refused combinations, the constructors' validation, the engine key, the demos'
flags, and what an engine asks of its context with the tracker off (what it asked before) and on (device calls replaced by
a recorder on host tensors)."""
import ctypes
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cfg_fakes
from cfg_fakes import cfg, lib_or_skip, rgbd_cfg
from vo_single_camera_sos_amd import _lib, pipeline
from vo_single_camera_sos_amd.device import Context
from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet

LK = dict(half=4, levels=3, max_iter=10, fb_max=0.5)
# (flags, detector, n_pairs, kp_cap) -> sosvo_frame_pair_batch_workspace(cfg), sosvo_sequence_workspace(cfg, n_pairs, 2 n_pairs + 1)
# on cfg_fakes.cfg (640 x 480 frames, 300 x 1200 panoramas, 12 masks, frame_cap 2048).  The numbers are what the library of the
# commit BEFORE this option answered (a6afe2e, built from its tree and asked through ctypes): with the bit clear the layout
# must not move.
SIZES_BEFORE = [
    (dict(flags=0, detector=0, n_pairs=4, kp_cap=1024), 18103040, 11208448),
    (dict(flags=_lib.FLAG_CROSS_CHECK_F2F | _lib.FLAG_SUBPIX | _lib.FLAG_GP3P, detector=0, n_pairs=3, kp_cap=512), 10384384, 6913280),
    (dict(flags=_lib.FLAG_RATIO_STEREO | (48 << _lib.RATIO_64THS_SHIFT) | _lib.FLAG_GATED_STEREO, detector=1, n_pairs=2, kp_cap=1024),
     20133376, 15760128),
]


# ---- the header and the bindings ---------------------------------------------------------------------------------------------
def test_header_declares_the_option_and_the_bindings_match():
    text = open(_lib.HEADER_PATH).read()
    assert "#define SOSVO_FLAG_LK_F2F 0x80" in text and _lib.FLAG_LK_F2F == 0x80
    assert "#define SOSVO_LK_MAX_LEVELS 4" in text and _lib.LK_MAX_LEVELS == 4
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "typedef struct sosvo_lk_options { int32_t half, levels, max_iter, reserved; double eps, min_eig, fb_max; } sosvo_lk_options;" in flat
    assert "int32_t sosvo_set_lk_options(sosvo_ctx* ctx, const sosvo_lk_options* options);" in flat
    assert _lib.SIGNATURES["sosvo_set_lk_options"] == (_lib.c_i32, [_lib.c_p, _lib.c_p])
    assert "sosvo_set_lk_options" in _lib.declared_functions()
    S = _lib.LkOptionsStruct
    assert ctypes.sizeof(S) == 40
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("half", 0), ("levels", 4), ("max_iter", 8), ("reserved", 12),
                                                                 ("eps", 16), ("min_eig", 24), ("fb_max", 32)]
    st = S.of(_lib.LKOptions(**LK))
    assert (st.half, st.levels, st.max_iter, st.reserved, st.eps, st.min_eig, st.fb_max) == (4, 3, 10, 0, 0.01, 1e-4, 0.5)
    assert S.of(_lib.LKOptions()).fb_max == 0.0                    # None: no check
    # the bit is free: no other option of the flags word uses it
    others = (_lib.FLAG_CAM_ROT_IDENTITY | _lib.FLAG_EPNP | _lib.FLAG_GP3P | _lib.FLAG_TWOPT | _lib.FLAG_CROSS_CHECK_STEREO |
              _lib.FLAG_CROSS_CHECK_F2F | _lib.FLAG_GATED_STEREO | _lib.FLAG_GATED_F2F | _lib.GATED_MAX_DIST_MASK | _lib.FLAG_RATIO_STEREO |
              _lib.FLAG_RATIO_F2F | _lib.RATIO_64THS_MASK | _lib.FLAG_SUBPIX | _lib.SUBPIX_HALF_MASK | _lib.RGBD_DETECTOR_MASK)
    assert others & _lib.FLAG_LK_F2F == 0
    assert lib_or_skip().sosvo_set_lk_options(None, None) == -1
    assert "#define SOSVO_LK_OPTIONS_DEFAULT {10, 3, 30, 0, 0.01, 1e-4, 0.0}" in text           # ... which are LKOptions' defaults
    d = S.of(_lib.LKOptions())
    assert (d.half, d.levels, d.max_iter, d.reserved, d.eps, d.min_eig, d.fb_max) == (10, 3, 30, 0, 0.01, 1e-4, 0.0)


# ---- workspace sizes -----------------------------------------------------------------------------------------------------------
def _sizes(lib, c, n_pairs):
    return (lib.sosvo_frame_pair_batch_workspace(ctypes.byref(c)), lib.sosvo_sequence_workspace(ctypes.byref(c), n_pairs, 2 * n_pairs + 1))


@pytest.mark.parametrize("kw,pair_bytes,seq_bytes", SIZES_BEFORE)
def test_workspace_sizes_with_the_bit_clear_are_those_of_before(kw, pair_bytes, seq_bytes):
    assert _sizes(lib_or_skip(), cfg(**kw), kw["n_pairs"]) == (pair_bytes, seq_bytes)


@pytest.mark.parametrize("kw,pair_bytes,seq_bytes", SIZES_BEFORE[:2])
def test_workspace_grows_by_the_stores_images(kw, pair_bytes, seq_bytes):
    """Sequence store: level 0 of 2 * slots images and their three upper levels.  Pair batch: level 0 is the front end's gray
    buffer, which the workspace held before, so it grows by the upper levels (and the tracker's temporaries)."""
    lib = lib_or_skip()
    kw = dict(kw, flags=(kw["flags"] & ~_lib.FLAG_CROSS_CHECK_F2F) | _lib.FLAG_LK_F2F)
    c, B = cfg(**kw), kw["n_pairs"]
    off = _sizes(lib, cfg(**dict(kw, flags=kw["flags"] & ~_lib.FLAG_LK_F2F)), B)
    on = _sizes(lib, c, B)
    slots = 2 * B + 1
    assert on[1] - off[1] >= 2 * slots * c.rows * c.cols + _lib.gray_pyramid_bytes(2 * slots, c.rows, c.cols, 4)
    assert on[0] - off[0] >= _lib.gray_pyramid_bytes(4 * B, c.rows, c.cols, 4)
    assert on[0] - off[0] < 4 * B * c.rows * c.cols                # (... and not by another level 0)
    tmp = 4 * B * c.frame_cap * (8 + 1 + 4 + 8)                     # next, status, err, back
    assert on[1] - off[1] < 2 * slots * c.rows * c.cols * 1.34 + tmp + 64 * 256
    for ns in (1, 2):
        assert lib.sosvo_frame_pair_batch_streams_workspace(ctypes.byref(c), ns) > 0


def test_refused_combinations_have_no_workspace():
    lib = lib_or_skip()
    r48 = 48 << _lib.RATIO_64THS_SHIFT
    assert all(v > 0 for v in _sizes(lib, cfg(_lib.FLAG_LK_F2F), 4))
    for ok in (_lib.FLAG_CROSS_CHECK_STEREO, _lib.FLAG_GATED_STEREO, _lib.FLAG_RATIO_STEREO | r48, _lib.FLAG_SUBPIX, _lib.FLAG_GP3P):
        assert all(v > 0 for v in _sizes(lib, cfg(_lib.FLAG_LK_F2F | ok), 4)), hex(ok)
    for bad in (_lib.FLAG_CROSS_CHECK_F2F, _lib.FLAG_GATED_F2F, _lib.FLAG_RATIO_F2F | r48):
        c = cfg(_lib.FLAG_LK_F2F | bad)
        assert _sizes(lib, c, 4) == (0, 0), hex(bad)
        assert lib.sosvo_frame_pair_batch_streams_workspace(ctypes.byref(c), 2) == 0
    c = rgbd_cfg(_lib.FLAG_LK_F2F)
    assert lib.sosvo_rgbd_pair_batch_workspace(ctypes.byref(c)) == 0 and lib.sosvo_rgbd_sequence_workspace(ctypes.byref(c), 4, 9) == 0
    assert lib.sosvo_rgbd_pair_batch_workspace(ctypes.byref(rgbd_cfg())) > 0
    # the store's images are one pyramid set of 2 * slots images: at most 65535
    assert lib.sosvo_sequence_workspace(ctypes.byref(cfg(_lib.FLAG_LK_F2F)), 4, 32767) > 0
    assert lib.sosvo_sequence_workspace(ctypes.byref(cfg(_lib.FLAG_LK_F2F)), 4, 32768) == 0
    assert lib.sosvo_sequence_workspace(ctypes.byref(cfg()), 4, 32768) > 0


# ---- the constructors ----------------------------------------------------------------------------------------------------------
class _Recorder(Context):
    """A Context without a device: the calls an engine makes, by name, with the flags of the cfg they carried."""

    def __init__(self):
        self.device, self.calls, self.stream = torch.device("cpu"), [], None

    def __del__(self):
        pass

    def set_lk_options(self, lk=None):
        self.lk_options = _lib.LKOptions.of(lk)
        self.calls.append(("set_lk_options", self.lk_options))


def _record(name, result=None):
    def call(self, *args, **kwargs):
        c = [a for a in args if isinstance(a, _lib.BatchCfg)]
        self.calls.append((name, c[0].ransac_flags if c else None))
        return result(self, *args) if callable(result) else result
    return call


for _name, _result in (("sequence_workspace", 4096), ("frame_pair_batch_workspace", 4096), ("frame_pair_batch_streams_workspace", 4096),
                       ("sequence_front_end", None), ("sequence_front_end_slots", None), ("sequence_track", None),
                       ("sequence_track_seeds", None), ("sequence_copy_slot", None), ("sequence_copy_slots", None),
                       ("sequence_frame_counts", lambda self, cfg_, w, s, first, n, ws: [7] * n), ("synchronize", None),
                       ("frame_pair_batch", None)):
    setattr(_Recorder, _name, _record(_name, _result))


def _model():
    return SimpleNamespace(H=12, W=16, rows=10, cols=40, nmask=3, unwrap_table=object(), mask_bits=None, pattern=None, omni_masks=None,
                           map_x=None, map_y=None)


def _rig():
    geo = (40.0, 10.0, 0.005, 1.2)
    return pipeline.RigConfig(geo, geo, (0, 0, 100.0), (0, 0, -100.0), 500.0, 7000.0)


@pytest.fixture
def host_only(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self, *a, **k: self)
    ev = SimpleNamespace(record=lambda *a: None, elapsed_time=lambda *a: 0.0)
    monkeypatch.setattr(torch.cuda, "Event", lambda *a, **k: ev)


SMALL = dict(num_of_features=20, kp_cap=32, frame_cap=64)
OMNI = [(pipeline.FramePairBatch, dict(n_pairs=2)), (pipeline.SequenceEngine, dict(window=2)),
        (pipeline.MultiSequenceEngine, dict(lanes=2, window=2))]


@pytest.mark.parametrize("cls,kw", OMNI, ids=[c.__name__ for c, _ in OMNI])
def test_omni_constructors_validate_the_tracker(cls, kw, host_only):
    new = lambda **more: cls(_Recorder(), _model(), _rig(), **kw, **SMALL, **more)  # noqa: E731
    assert new().cfg.ransac_flags & _lib.FLAG_LK_F2F == 0 and new(f2f_tracker="match").cfg.ransac_flags & _lib.FLAG_LK_F2F == 0
    on = new(f2f_tracker="lk", lk=LK, subpix=3, cross_check_stereo=True, gated_stereo=True, ratio_stereo=True, ratio=0.75)
    assert on.cfg.ransac_flags & _lib.FLAG_LK_F2F and on.cfg.ransac_flags & _lib.FLAG_SUBPIX
    assert (on.lk if cls is pipeline.FramePairBatch else on.fam.lk) == _lib.LKOptions(**LK)
    assert (new(f2f_tracker="lk").lk if cls is pipeline.FramePairBatch else new(f2f_tracker="lk").fam.lk) == _lib.LKOptions()
    for bad in (dict(f2f_tracker="flow"), dict(lk=LK), dict(f2f_tracker="match", lk=LK), dict(f2f_tracker="lk", lk=dict(half=11)),
                dict(f2f_tracker="lk", lk=dict(window=4)), dict(f2f_tracker="lk", lk=5), dict(f2f_tracker="lk", cross_check_f2f=True),
                dict(f2f_tracker="lk", gated_f2f=True), dict(f2f_tracker="lk", ratio_f2f=True, ratio=0.75)):
        with pytest.raises(ValueError):
            new(**bad)


def test_overlapped_pairs_validate_before_they_touch_the_device():
    for bad in (dict(f2f_tracker="flow"), dict(lk=LK), dict(f2f_tracker="lk", cross_check_f2f=True), dict(f2f_tracker="lk", lk=dict(levels=5))):
        with pytest.raises(ValueError):
            pipeline.OverlappedFramePairs(0, None, (12, 16), _rig(), 2, **bad)


def test_rgbd_constructors_refuse_the_tracker():
    cam = pipeline.RGBDCamConfig(fx=500.0, fy=500.0, center_x=8.0, center_y=6.0)
    for cls, kw in ((pipeline.RGBDPairBatch, dict(n_pairs=2)), (pipeline.RGBDSequenceEngine, dict(window=2)),
                    (pipeline.RGBDMultiSequenceEngine, dict(lanes=2, window=2))):
        for bad in (dict(f2f_tracker="lk"), dict(f2f_tracker="lk", lk=LK), dict(lk=LK), dict(f2f_tracker="flow")):
            with pytest.raises(ValueError):
                cls(_Recorder(), cam, image_shape=(12, 16), **kw, **bad)


# ---- what an engine asks of its context ----------------------------------------------------------------------------------------
def _tensors(obj):
    return {k: (tuple(v.shape), v.dtype) for k, v in vars(obj).items() if isinstance(v, torch.Tensor)}


def _drive(eng):
    frames = [np.zeros((12, 16, 3), np.uint8)] * 4
    infos = eng.push_window(frames[:2])
    eng.promote(infos[1]["slot"])
    eng.push_window(frames[2:])
    eng.track(eng.key_slot, eng.last_slot, 3)
    return eng.ctx.calls


def test_with_the_matcher_an_engine_asks_what_it_asked_before(host_only):
    """Default arguments and f2f_tracker="match": the same calls with the same flags, the same buffers, and no call that sets
    tracker settings -- the call list is written out, it is what the engines made before the option existed."""
    want = ["sequence_workspace", "sequence_front_end", "sequence_track", "sequence_frame_counts", "sequence_front_end", "sequence_track",
            "sequence_track", "sequence_frame_counts", "sequence_copy_slot", "sequence_track"]
    runs = []
    for more in ({}, dict(f2f_tracker="match")):
        eng = pipeline.SequenceEngine(_Recorder(), _model(), _rig(), window=2, **SMALL, **more)
        calls = _drive(eng)
        assert [c[0] for c in calls] == want
        assert {c[1] for c in calls} == {_lib.FLAG_GP3P}
        assert eng.fam.lk is None
        runs.append((calls, _tensors(eng), _tensors(eng.fam), eng.workspace.numel()))
    assert runs[0] == runs[1]
    for more in ({}, dict(f2f_tracker="match")):
        b = pipeline.FramePairBatch(_Recorder(), _model(), _rig(), 2, **SMALL, **more)
        b.step()
        b.enqueue()
        assert b.ctx.calls == [("frame_pair_batch_workspace", 0), ("frame_pair_batch", 0), ("frame_pair_batch", 0)] and b.lk is None


def test_engines_that_share_a_context_each_track_with_their_own_settings(host_only):
    ctx = _Recorder()
    a = pipeline.SequenceEngine(ctx, _model(), _rig(), window=2, f2f_tracker="lk", lk=LK, **SMALL)
    b = pipeline.SequenceEngine(ctx, _model(), _rig(), window=2, f2f_tracker="lk", lk=dict(LK, half=10), **SMALL)
    m = pipeline.SequenceEngine(ctx, _model(), _rig(), window=2, **SMALL)
    frames = [np.zeros((12, 16, 3), np.uint8)] * 2
    del ctx.calls[:]
    a.push_window(frames)
    a.push_window(frames)                      # (the context still holds a's settings: not set again)
    m.push_window(frames)                      # (an engine that matches sets nothing)
    a.track(a.key_slot, a.last_slot, 1)
    b.push_window(frames)
    a.promote(a.last_slot)
    a.track(a.key_slot, a.last_slot, 1)        # the copy and the tracking call run under a's settings again
    sets = [(i, c[1].half) for i, c in enumerate(ctx.calls) if c[0] == "set_lk_options"]
    names = [c[0] for c in ctx.calls]
    assert [h for _, h in sets] == [4, 10, 4]
    assert sets[0][0] == 0 and names[sets[1][0] + 1] == "sequence_front_end" and names[sets[2][0] + 1] == "sequence_copy_slot"
    assert all(c[1] & _lib.FLAG_LK_F2F for c in ctx.calls if c[0] in ("sequence_front_end", "sequence_track") and c[1] != _lib.FLAG_GP3P)
    pb = pipeline.FramePairBatch(ctx, _model(), _rig(), 2, f2f_tracker="lk", lk=LK, **SMALL)
    del ctx.calls[:]
    pb.step()
    pb.step()
    assert [c[0] for c in ctx.calls] == ["frame_pair_batch", "frame_pair_batch"]           # a's settings are pb's
    ctx.set_lk_options(None)
    pb.enqueue()
    assert [c[0] for c in ctx.calls[-2:]] == ["set_lk_options", "frame_pair_batch"] and ctx.lk_options == _lib.LKOptions(**LK)


# ---- run_VO's layers -------------------------------------------------------------------------------------------------------------
def test_set_f2f_tracker_and_the_engine_key():
    t, rig, img = cfg_fakes.tracker(rgbd=False), cfg_fakes.Rig(), np.zeros((480, 640, 3), np.uint8)
    t.camera_model = rig
    assert t.lk_options is None
    off = pet._sos_engine_settings(t, rig, img)
    assert "f2f_tracker" not in off[1] and "lk" not in off[1]      # the engine is built with what it was built with before
    pet.set_f2f_tracker(t, None)
    assert t.lk_options is None
    pet.set_f2f_tracker(t, "lk", LK)
    assert t.lk_options == rig.lk_options == _lib.LKOptions(**LK)
    on = pet._sos_engine_settings(t, rig, img)
    assert on[1]["f2f_tracker"] == "lk" and on[1]["lk"] == _lib.LKOptions(**LK) and on[2] != off[2]
    pet.set_f2f_tracker(t, "lk", dict(LK, half=5))
    assert pet._sos_engine_settings(t, rig, img)[2] not in (on[2], off[2])
    pet.set_f2f_tracker(t, "lk")
    assert t.lk_options == _lib.LKOptions()
    pet.set_f2f_tracker(t, "match")
    assert t.lk_options is None and rig.lk_options is None and pet._sos_engine_settings(t, rig, img)[2] == off[2]
    for bad in (("flow", None), (None, LK), ("match", LK), ("lk", dict(half=1))):
        with pytest.raises(ValueError):
            pet.set_f2f_tracker(t, *bad)
    rig.feature_matcher_for_motion.cross_check = True              # an option of the matcher the tracker would replace
    with pytest.raises(ValueError):
        pet.set_f2f_tracker(t, "lk")
    pet.set_f2f_tracker(t, "match")
    r = cfg_fakes.tracker(rgbd=True)
    r.camera_model = cfg_fakes.rgbd_cam()
    with pytest.raises(ValueError):
        pet.set_f2f_tracker(r, "lk")
    pet.set_f2f_tracker(r, "match")


def test_run_vo_and_the_drivers_take_the_option():
    import inspect
    for fn in (pet.run_VO, pet.run_VO_many, pet.run_VO_live, pet.driver_VO, pet.driver_VO_many, pet.driver_VO_live):
        p = inspect.signature(fn).parameters
        assert p["f2f_tracker"].default is None and p["lk"].default is None, fn.__name__


def test_the_demos_accept_the_flags():
    import demo_vo_rgbd
    import demo_vo_sos
    import demo_vo_sos_live
    from vo_single_camera_sos_amd.omnistereo.common_tools import f2f_tracker_arguments
    for demo in (demo_vo_sos, demo_vo_sos_live, demo_vo_rgbd):
        parser = demo.build_parser()
        args = parser.parse_args(["somewhere", "--f2f_tracker", "lk", "--lk_half", "4", "--lk_levels", "2", "--lk_max_iter", "10",
                                  "--lk_fb_max", "0.5"])
        assert f2f_tracker_arguments(args) == dict(f2f_tracker="lk", lk=dict(half=4, levels=2, max_iter=10, fb_max=0.5))
        assert f2f_tracker_arguments(parser.parse_args(["somewhere"])) == dict(f2f_tracker=None, lk=None)
        assert f2f_tracker_arguments(parser.parse_args(["somewhere", "--f2f_tracker", "match"])) == dict(f2f_tracker="match", lk=None)
        with pytest.raises(SystemExit):
            parser.parse_args(["somewhere", "--f2f_tracker", "flow"])
