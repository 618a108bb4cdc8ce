"""CPU (library and headers only, no GPU): the cyclic-column stages are declared, bound and reachable -- the header's define and
entry points against the ctypes table, the Context methods and the host mirror's option, and what stays as it was: the plain
entry points' bindings and Context.gray_pyramid's parameters; and FramePairPipeline(cyclic_columns=...): with the option off it
asks its context exactly what it asked before, with it on for the cyclic stages, and it refuses what cannot be cyclic before
anything is allocated (device calls replaced by a recorder, as in tests/test_lk_cfg.py).  Then the batched layers with the
fakes of tests/test_lk_layers_cfg.py: SOSVO_FLAG_CYCLIC_F2F in the header and free in the omni word, workspace sizes with the
bit set against clear, the cols % 8 rule, the constructors' validation before the device, the RGB-D refusals, what an engine
asks with the option off, set_cyclic_columns and the engine key, run_VO / the drivers / the demos, and the host gate."""
import inspect
import os
import re

import numpy as np
import pytest

from vo_single_camera_sos_amd import _lib
from vo_single_camera_sos_amd.device import Context, GrayPyramid
from vo_single_camera_sos_amd.omnistereo import common_cv

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sosvo.h")
TWINS = {"sosvo_gray_pyramid_cyclic": "sosvo_gray_pyramid", "sosvo_f2f_assemble_cyclic": "sosvo_f2f_assemble",
         "sosvo_f2f_assemble_tracked_cyclic": "sosvo_f2f_assemble_tracked"}


def _declaration(text, name):
    """The parameter list of a function declared in the header, comments removed."""
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_the_header_declares_the_flag_and_the_entry_points():
    text = open(HEADER).read()
    assert re.search(r"^#define SOSVO_LK_CYCLIC_COLUMNS 4\s*$", text, flags=re.M)
    assert re.search(r"^#define SOSVO_LK_INITIAL_FLOW 1\s*$", text, flags=re.M)
    assert _lib.LK_CYCLIC_COLUMNS == 4 and _lib.LK_INITIAL_FLOW == 1
    declared = _lib.declared_functions()
    for new, old in TWINS.items():
        assert new in declared and new in _lib.SIGNATURES
        assert _declaration(text, new) == _declaration(text, old)                 # the arguments of the plain call
        assert _lib.SIGNATURES[new] == _lib.SIGNATURES[old]
    # the gated matcher: the v side's bound leaves, the period arrives after max_du
    plain, cyc = _declaration(text, "sosvo_match_hamming_gated"), _declaration(text, "sosvo_match_hamming_gated_cyclic")
    assert [a for a in plain if a != "double min_dv"] == [a for a in cyc if a != "double period"]
    assert cyc.index("double period") == cyc.index("double max_du") + 1
    assert len(_lib.SIGNATURES["sosvo_match_hamming_gated_cyclic"][1]) == len(cyc)
    sig = _lib.SIGNATURES["sosvo_match_hamming_gated_cyclic"][1]
    assert sig[cyc.index("double max_du")] is sig[cyc.index("double period")] is _lib.c_f64
    assert sig[cyc.index("int32_t max_distance")] is _lib.c_i32
    for name, sg in _lib.SIGNATURES.items():                                      # (every binding has its declaration's length)
        if name.endswith("_cyclic"):
            assert len(sg[1]) == len(_declaration(text, name)), name
    # the rule is stated where the neighbouring rules are
    for phrase in ("mod (32 cols_l)", "min(d, W - d)", "W - d <= f2f_max_hdiff", "period - max_du", "2 half + 3 columns"):
        assert phrase in text, phrase


def test_the_library_exports_them():
    lib = _lib.load()
    for name in list(TWINS) + ["sosvo_match_hamming_gated_cyclic"]:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # sizes are those of the plain pyramid: the same buffer serves both
    assert _lib.gray_pyramid_bytes(4, 96, 128, 4) == 4 * (48 * 64 + 24 * 32 + 12 * 16)


def test_the_context_and_the_host_mirror_take_the_option():
    plain = inspect.signature(Context.gray_pyramid).parameters
    assert list(plain)[1:] == ["gray", "levels", "row_range", "out"]              # as it was
    assert list(inspect.signature(Context.gray_pyramid_cyclic).parameters) == list(plain)
    assert [p.default for p in inspect.signature(Context.gray_pyramid_cyclic).parameters.values()] == [p.default for p in plain.values()]
    sig = inspect.signature(Context.track_lk).parameters
    assert sig["cyclic"].default is None and list(sig)[-1] == "cyclic"
    for fn in (Context.f2f_assemble, Context.f2f_assemble_tracked):
        sig = inspect.signature(fn).parameters
        assert sig["cyclic"].default is False and list(sig)[-1] == "cyclic"
    sig = inspect.signature(Context.match_hamming_gated_cyclic).parameters
    assert list(sig)[1:9] == ["q_desc", "t_desc", "q_pos", "t_pos", "nq", "nt", "max_du", "period"]
    assert sig["max_distance"].default is None and sig["n_forward"].default is None
    assert GrayPyramid(None, None, 3, None).cyclic is False and GrayPyramid(None, None, 3, None, True).cyclic is True
    sig = inspect.signature(common_cv.calc_optical_flow_pyr_lk).parameters
    assert sig["cyclic"].default is False and list(sig)[-1] == "cyclic"


def test_the_host_mirror_checks_the_width_before_it_touches_the_device():
    """ctx is never used: the refusal comes first."""
    img = np.zeros((32, 126), np.uint8)
    pts = np.zeros((3, 2), np.float32)
    with pytest.raises(ValueError, match="126"):                                  # 126 is no multiple of 4
        common_cv.calc_optical_flow_pyr_lk(img, img, pts, win_half=4, max_level=2, ctx=object(), cyclic=True)
    with pytest.raises(ValueError, match="40"):                                   # 40 >> 2 = 10 columns, the template has 11
        common_cv.calc_optical_flow_pyr_lk(img[:, :40], img[:, :40], pts, win_half=4, max_level=2, ctx=object(), cyclic=True)
    empty = common_cv.calc_optical_flow_pyr_lk(img[:, :48], img[:, :48], pts[:0], win_half=4, max_level=2, ctx=object(), cyclic=True)
    assert empty[0].shape == (0, 1, 2)                                            # 48 >> 2 = 12: fine, and nothing to track


# ---- the pair pipeline (device calls replaced by a recorder on host tensors, as tests/test_lk_cfg.py) -----------------------------
def _recorded(pipe_kw, rig=None):
    import torch
    from test_lk_cfg import _ctx, _front_end, _rig
    from vo_single_camera_sos_amd import pipeline
    ctx, fe, calls = _ctx(), _front_end(), []

    def record(name, result=None):
        def call(*a, **k):
            calls.append((name, a, k))
            return result(*a, **k) if callable(result) else result
        return call
    pipe = pipeline.FramePairPipeline(ctx, rig or _rig(), 2, frame_cap=16, front_end=fe, **pipe_kw)
    pipe._M2[0].copy_(torch.tensor([5, 6, 7, 8], dtype=torch.int32))
    for name in ("match_1nn_slots", "sort_matches", "f2f_assemble", "ransac_abs_pose", "refine_abs_pose", "f2f_assemble_tracked"):
        setattr(ctx, name, record(name))
    ctx.gray_pyramid = record("gray_pyramid", "PYR")
    ctx.gray_pyramid_cyclic = record("gray_pyramid_cyclic", "CPYR")
    ctx.track_lk = record("track_lk", lambda *a, **k: k["out"])
    pipe.track()
    return pipe, calls


def _same(x, y):
    import torch
    if isinstance(x, torch.Tensor) or isinstance(y, torch.Tensor):
        return isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and x.shape == y.shape and bool((x == y).all())
    if isinstance(x, (tuple, list)) and isinstance(y, (tuple, list)):
        return len(x) == len(y) and all(_same(a, b) for a, b in zip(x, y))
    if isinstance(x, dict) and isinstance(y, dict):
        return list(x) == list(y) and all(_same(x[k], y[k]) for k in x)
    return type(x) is type(y) and (x == y or x is y or not isinstance(x, (int, float, str, bool, type(None))))


@pytest.mark.parametrize("kw", [{}, dict(gated_f2f=True, gated_max_distance=64), dict(f2f_tracker="lk", lk=dict(half=4, levels=2, fb_max=0.5))])
def test_with_the_option_off_the_pipeline_asks_its_context_what_it_asked_before(kw):
    """cyclic_columns=False spelt out against the constructor that has never heard of it: the same calls, the same positional
    and keyword arguments (no `cyclic` keyword, no period behind the gate)."""
    a, calls_a = _recorded(kw)
    b, calls_b = _recorded(dict(kw, cyclic_columns=False))
    assert a.cyclic is False and b.cyclic is False
    assert [c[0] for c in calls_a] == [c[0] for c in calls_b] and "gray_pyramid_cyclic" not in [c[0] for c in calls_a]
    for (_, aa, ka), (_, ab, kb) in zip(calls_a, calls_b):
        assert _same(aa, ab) and _same(ka, kb)
        assert "cyclic" not in ka and "period" not in ka


def test_with_the_option_on_the_pipeline_asks_for_the_cyclic_stages():
    from vo_single_camera_sos_amd import pipeline
    _, calls = _recorded(dict(cyclic_columns=True))
    by = {c[0]: c for c in calls}
    assert [c[0] for c in calls] == ["match_1nn_slots", "sort_matches", "f2f_assemble", "ransac_abs_pose", "refine_abs_pose"]
    assert by["f2f_assemble"][2]["cyclic"] is True and by["match_1nn_slots"][2]["gate"] is None
    _, calls = _recorded(dict(cyclic_columns=True, gated_f2f=True, gated_max_distance=64))
    kw = {c[0]: c for c in calls}["match_1nn_slots"][2]
    assert kw["gate"] == (-1.0, 75.0, 64) and kw["period"] == 1200.0                           # the gate as it was, the period beside it
    pipe, calls = _recorded(dict(cyclic_columns=True, f2f_tracker="lk", lk=dict(half=4, levels=2)))
    assert [c[0] for c in calls] == ["gray_pyramid_cyclic", "track_lk", "f2f_assemble_tracked", "ransac_abs_pose", "refine_abs_pose"]
    assert calls[1][1][0] == "CPYR" and calls[2][2]["cyclic"] is True and "cyclic" not in calls[1][2]    # (track_lk follows the pyramid)
    # refusals, before anything is allocated or asked of the device
    from test_lk_cfg import GEO, _ctx, _front_end
    odd = pipeline.RigConfig((1204.0,) + GEO[1:], (1204.0,) + GEO[1:], (0, 0, 100.0), (0, 0, -100.0), 500.0, 7000.0)
    with pytest.raises(ValueError, match="1204"):
        pipeline.FramePairPipeline(_ctx(), odd, 2, frame_cap=16, front_end=_front_end(), f2f_tracker="lk", lk=dict(half=4, levels=4),
                                   cyclic_columns=True)
    with pytest.raises(ValueError, match="ratio"):
        pipeline.FramePairPipeline(_ctx(), odd, 2, frame_cap=16, gated_f2f=True, ratio_f2f=True, ratio=0.75, cyclic_columns=True)
    assert pipeline.FramePairPipeline(_ctx(), odd, 2, frame_cap=16, cyclic_columns=True).cyclic is True


# ---- the batched layers (the fakes of tests/test_lk_layers_cfg.py: a Context without a device that records its calls) -------------
import ctypes  # noqa: E402

import cfg_fakes  # noqa: E402
from cfg_fakes import cfg, rgbd_cfg  # noqa: E402
from test_lk_layers_cfg import OMNI, SIZES_BEFORE, SMALL, _drive, _model, _Recorder, _rig, _sizes, _tensors, host_only  # noqa: E402,F401
from vo_single_camera_sos_amd import pipeline  # noqa: E402
from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet  # noqa: E402

CYC = _lib.FLAG_CYCLIC_F2F
LK2 = dict(half=4, levels=2, max_iter=10, fb_max=0.5)      # (the fakes' panoramas have 40 columns: 20 on top, the template has 11)


def test_the_header_declares_the_batch_flag():
    text = open(HEADER).read()
    assert re.search(r"^#define SOSVO_FLAG_CYCLIC_F2F 0x200\s*$", text, flags=re.M) and CYC == 0x200
    assert CYC & (_lib.RGBD_DETECTOR_MASK) == 0x200                  # (the RGB-D word has its detector there: omni only)
    for other in ("FLAG_CAM_ROT_IDENTITY", "FLAG_EPNP", "FLAG_GP3P", "FLAG_TWOPT", "FLAG_RATIO_STEREO", "FLAG_RATIO_F2F", "FLAG_SUBPIX",
                  "FLAG_LK_F2F", "FLAG_LK_STEREO", "FLAG_CROSS_CHECK_STEREO", "FLAG_CROSS_CHECK_F2F", "FLAG_GATED_STEREO",
                  "FLAG_GATED_F2F", "SUBPIX_HALF_MASK", "GATED_MAX_DIST_MASK", "RATIO_64THS_MASK"):
        assert CYC & getattr(_lib, other) == 0, other                # the bit is free in the omni word


@pytest.mark.parametrize("kw,pair_bytes,seq_bytes", SIZES_BEFORE)
def test_workspace_sizes_with_the_bit_set_equal_those_without(kw, pair_bytes, seq_bytes):
    lib = cfg_fakes.lib_or_skip()
    for more in (0, _lib.FLAG_LK_F2F if not kw["flags"] & _lib.FLAG_CROSS_CHECK_F2F else 0, _lib.FLAG_GATED_F2F):
        clear = _sizes(lib, cfg(**dict(kw, flags=kw["flags"] | more)), kw["n_pairs"])
        assert _sizes(lib, cfg(**dict(kw, flags=kw["flags"] | more | CYC)), kw["n_pairs"]) == clear and min(clear) > 0
        for ns in (2, 3):
            c0, c1 = cfg(**dict(kw, flags=kw["flags"] | more)), cfg(**dict(kw, flags=kw["flags"] | more | CYC))
            assert lib.sosvo_frame_pair_batch_streams_workspace(ctypes.byref(c1), ns) == \
                lib.sosvo_frame_pair_batch_streams_workspace(ctypes.byref(c0), ns)


def test_the_tracked_path_needs_a_width_that_is_a_multiple_of_eight():
    lib = cfg_fakes.lib_or_skip()
    for flags, cols, ok in ((_lib.FLAG_LK_F2F | CYC, 1444, False), (_lib.FLAG_LK_F2F | CYC, 1440, True), (_lib.FLAG_LK_F2F, 1444, True),
                            (CYC, 1444, True), (CYC | _lib.FLAG_GATED_F2F, 1444, True),
                            (CYC | _lib.FLAG_GATED_F2F | _lib.FLAG_RATIO_F2F | (48 << _lib.RATIO_64THS_SHIFT), 1440, False),
                            (_lib.FLAG_GATED_F2F | _lib.FLAG_RATIO_F2F | (48 << _lib.RATIO_64THS_SHIFT), 1440, True)):
        c = cfg(flags=flags)
        c.cols = cols
        sizes = _sizes(lib, c, 4) + (lib.sosvo_frame_pair_batch_streams_workspace(ctypes.byref(c), 2),)
        assert all(v > 0 for v in sizes) if ok else sizes == (0, 0, 0), (hex(flags), cols, sizes)


@pytest.mark.parametrize("cls,kw", OMNI, ids=[c.__name__ for c, _ in OMNI])
def test_omni_constructors_validate_the_option_before_the_device(cls, kw, host_only):  # noqa: F811
    new = lambda rig=None, **more: cls(_Recorder(), _model(), rig or _rig(), **kw, **SMALL, **more)  # noqa: E731
    assert new().cfg.ransac_flags & CYC == 0 and new(cyclic_columns=False).cfg.ransac_flags & CYC == 0
    assert new(cyclic_columns=True).cfg.ransac_flags & CYC and new(cyclic_columns=True, gated_f2f=True).cfg.ransac_flags & CYC
    on = new(cyclic_columns=True, f2f_tracker="lk", lk=LK2)
    assert on.cfg.ransac_flags & CYC and on.cfg.ransac_flags & _lib.FLAG_LK_F2F
    geo = lambda w: (w, 10.0, 0.005, 1.2)  # noqa: E731
    odd = pipeline.RigConfig(geo(44.0), geo(44.0), (0, 0, 100.0), (0, 0, -100.0), 500.0, 7000.0)      # 44 % 8 != 0
    for rig, bad, word in ((odd, dict(f2f_tracker="lk", lk=LK2), "44"), (None, dict(f2f_tracker="lk", lk=dict(half=4, levels=3)), "40"),
                           (None, dict(gated_f2f=True, ratio_f2f=True, ratio=0.75), "ratio"),
                           (pipeline.RigConfig(geo(40.5), geo(40.5), (0, 0, 100.0), (0, 0, -100.0), 500.0, 7000.0), {}, "40.5")):
        ctx = _Recorder()
        with pytest.raises(ValueError, match=word):
            cls(ctx, _model(), rig or _rig(), **kw, **SMALL, cyclic_columns=True, **bad)
        assert ctx.calls == []                                       # nothing was asked of the device
    assert new(odd, cyclic_columns=True).cfg.ransac_flags & CYC      # (the matcher takes any integer width)


def test_overlapped_pairs_validate_the_option_before_they_touch_the_device():
    for bad in (dict(f2f_tracker="lk", lk=dict(half=10, levels=3)), dict(gated_f2f=True, ratio_f2f=True, ratio=0.75)):
        with pytest.raises(ValueError, match="cyclic_columns"):
            pipeline.OverlappedFramePairs(0, None, (12, 16), _rig(), 2, cyclic_columns=True, **bad)


def test_rgbd_constructors_refuse_the_option():
    cam = pipeline.RGBDCamConfig(fx=500.0, fy=500.0, center_x=8.0, center_y=6.0)
    for cls, kw in ((pipeline.RGBDPairBatch, dict(n_pairs=2)), (pipeline.RGBDSequenceEngine, dict(window=2)),
                    (pipeline.RGBDMultiSequenceEngine, dict(lanes=2, window=2))):
        with pytest.raises(ValueError, match="cyclic"):
            cls(_Recorder(), cam, image_shape=(12, 16), cyclic_columns=True, **kw)
    r = cfg_fakes.tracker(rgbd=True)
    r.camera_model = cfg_fakes.rgbd_cam()
    with pytest.raises(ValueError, match="cyclic"):
        pet.set_cyclic_columns(r, True)
    pet.set_cyclic_columns(r, False)
    pet.set_cyclic_columns(r, None)


def test_with_the_option_off_an_engine_asks_what_it_asked_before(host_only):  # noqa: F811
    runs = []
    for more in ({}, dict(cyclic_columns=False)):
        eng = pipeline.SequenceEngine(_Recorder(), _model(), _rig(), window=2, **SMALL, **more)
        calls = _drive(eng)
        assert {c[1] for c in calls} == {_lib.FLAG_GP3P}
        runs.append((calls, _tensors(eng), _tensors(eng.fam), eng.workspace.numel()))
    assert runs[0] == runs[1]
    on = pipeline.SequenceEngine(_Recorder(), _model(), _rig(), window=2, cyclic_columns=True, **SMALL)
    calls = _drive(on)
    assert [c[0] for c in calls] == [c[0] for c in runs[0][0]] and {c[1] for c in calls} == {_lib.FLAG_GP3P | CYC}
    assert (_tensors(on), _tensors(on.fam), on.workspace.numel()) == runs[0][1:]      # no new buffers
    for more in ({}, dict(cyclic_columns=False)):
        b = pipeline.FramePairBatch(_Recorder(), _model(), _rig(), 2, **SMALL, **more)
        b.step()
        assert b.ctx.calls == [("frame_pair_batch_workspace", 0), ("frame_pair_batch", 0)] and b.cyclic is False


def test_set_cyclic_columns_and_the_engine_key():
    t, rig, img = cfg_fakes.tracker(rgbd=False), cfg_fakes.Rig(), np.zeros((480, 640, 3), np.uint8)
    t.camera_model = rig
    off = pet._sos_engine_settings(t, rig, img)
    assert "cyclic_columns" not in off[1]
    pet.set_cyclic_columns(t, None)
    assert not getattr(rig, "cyclic_columns", False) and pet._sos_engine_settings(t, rig, img)[2] == off[2]
    pet.set_cyclic_columns(t, True)
    on = pet._sos_engine_settings(t, rig, img)
    assert rig.cyclic_columns is True and t.cyclic_columns is True and on[1]["cyclic_columns"] is True and on[2] != off[2]
    pet.set_cyclic_columns(t, False)
    assert rig.cyclic_columns is False and pet._sos_engine_settings(t, rig, img)[2] == off[2]
    assert "cyclic_columns" not in pet._sos_engine_settings(t, rig, img)[1]


def test_run_vo_the_drivers_and_the_demos_take_the_option():
    import demo_vo_sos
    import demo_vo_sos_live
    for fn in (pet.run_VO, pet.run_VO_many, pet.run_VO_live, pet.driver_VO, pet.driver_VO_many, pet.driver_VO_live):
        assert inspect.signature(fn).parameters["cyclic_columns"].default is None, fn.__name__
    for cls in (pipeline.FramePairPipeline, pipeline.OverlappedFramePairs, pipeline.FramePairBatch, pipeline.SequenceEngine,
                pipeline.MultiSequenceEngine):
        assert inspect.signature(cls.__init__).parameters["cyclic_columns"].default is False, cls.__name__
    assert list(inspect.signature(pet.set_cyclic_columns).parameters) == ["tracker", "on"]
    for demo in (demo_vo_sos, demo_vo_sos_live):
        parser = demo.build_parser()
        assert parser.parse_args(["somewhere", "--cyclic_columns"]).cyclic_columns is True
        assert parser.parse_args(["somewhere"]).cyclic_columns is False


def test_the_host_gate_follows_the_camera_model():
    """match_features_frame_to_frame's |du| gate on a matcher that pairs row i with row i: pairs across the seam pass only with
    the camera model's cyclic_columns."""
    from types import SimpleNamespace
    n = 6
    u_t = np.array([2.0, 1195.0, 500.0, 500.0, 30.0, 30.0])
    u_q = np.array([1197.0, 60.0, 575.0, 575.5, 1155.0, 1154.5])     # W - d = 5, 65, d = 75, 75.5, W - d = 75, 75.5
    pts_t, pts_q = np.stack([u_t, np.full(n, 50.0)], 1), np.stack([u_q, np.full(n, 50.0)], 1)
    fm = SimpleNamespace(gated=False, percentage_good_matches=1.0, match_arrays=lambda q, t: (np.arange(n), np.arange(n), np.zeros(n)))
    desc, kp = np.zeros((n, 32), np.uint8), list(range(n))
    for cyclic, want in ((False, [2]), (True, [0, 1, 2, 4])):
        cm = SimpleNamespace(feature_matcher_for_motion=fm, cyclic_columns=cyclic, top_model=SimpleNamespace(panorama=SimpleNamespace(cols=1200)))
        (t, _, _), (q, _, _), _ = pet.match_features_frame_to_frame(cm, kp, desc, kp, desc, np.zeros((n, 3)), max_horizontal_diff=75.0,
                                                                    keypts_as_points_train=pts_t, keypts_as_points_query=pts_q)
        assert list(t) == want and list(q) == want
    cm = SimpleNamespace(feature_matcher_for_motion=fm, top_model=None)      # (a model that has never heard of the option)
    assert list(pet.match_features_frame_to_frame(cm, kp, desc, kp, desc, np.zeros((n, 3)), max_horizontal_diff=75.0,
                                                  keypts_as_points_train=pts_t, keypts_as_points_query=pts_q)[0][0]) == [2]
