"""CPU: the configuration layer of the Lucas-Kanade tracker -- the header's prototypes and the bindings, LKOptions' validation,
FramePairPipeline(f2f_tracker=..., lk=...): its refusals, that the default builds the MatchOptions and the buffers it built
before, and what track() asks of the context with the tracker on (device calls replaced by a recorder on host tensors)."""
import inspect
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cfg_fakes import lib_or_skip
from vo_single_camera_sos_amd import _lib, pipeline
from vo_single_camera_sos_amd.device import Context
from vo_single_camera_sos_amd.omnistereo import common_cv

GEO = (1200.0, 300.0, 0.005, 1.2)
# the tensors a FramePairPipeline without the tracker owns (name -> shape for n_pairs 2, nmask 3, bucket_cap 8, frame_cap 16)
BUFFERS = dict(kp_top=(12, 8, 2), kp_bot=(12, 8, 2), desc_top=(12, 8, 32), desc_bot=(12, 8, 32), n_top=(12,), n_bot=(12,),
               s_keys=(12, 8, 1), s_order=(12, 8), _d2=(2, 4, 16, 32), _M2=(2, 4), _m2=(2, 4, 16, 2), ref_frame=(2,),
               cur_frame=(2,), _o2=(4, 16), _q=(4,), _t=(4,), _k=(4, 16, 1), _q2=(4,), _t2=(4,), _k2=(4, 16, 1), k_top=(2, 16, 1),
               k_bot=(2, 16, 1), o_top=(2, 16), o_bot=(2, 16), T=(2, 3, 4), lm_cost=(2,), lm_iters=(2,), cam_off=(2, 3),
               cam_rot=(2, 3, 3))


def _rig():
    return pipeline.RigConfig(GEO, GEO, (0, 0, 100.0), (0, 0, -100.0), 500.0, 7000.0)


def _ctx():
    c = Context.__new__(Context)
    c.device = torch.device("cpu")
    return c


def _front_end(keep_panoramas=False):
    F, NM, cap = 4, 3, 8
    z = lambda shape, dt: torch.zeros(shape, dtype=dt)  # noqa: E731
    views = dict(kp_top=z((F * NM, cap, 2), torch.float32), kp_bot=z((F * NM, cap, 2), torch.float32),
                 desc_top=z((F * NM, cap, 32), torch.uint8), desc_bot=z((F * NM, cap, 32), torch.uint8),
                 n_top=z((F * NM,), torch.int32), n_bot=z((F * NM,), torch.int32))
    return SimpleNamespace(F=F, kp_cap=cap, model=SimpleNamespace(nmask=NM), view_arrays=lambda: views, subpix=None,
                           gray=z((2 * F, 30, 40), torch.uint8), gray_rows=torch.tensor([[3, 20], [5, 28]], dtype=torch.int32),
                           keep_panoramas=keep_panoramas)


def _tensors(obj):
    return {k: tuple(v.shape) for k, v in vars(obj).items() if isinstance(v, torch.Tensor)}


def test_header_declares_the_prototypes_and_the_bindings_match():
    text = open(_lib.HEADER_PATH).read()
    assert "#define SOSVO_LK_INITIAL_FLOW 1" in text and _lib.LK_INITIAL_FLOW == 1
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for proto in ("int32_t sosvo_gray_pyramid_bytes(sosvo_ctx* ctx, int32_t nimg, int32_t rows, int32_t cols, int32_t levels, "
                  "int64_t* bytes);",
                  "int32_t sosvo_gray_pyramid(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols, "
                  "int32_t levels, const int32_t* row_range, uint8_t* pyr);",
                  "int32_t sosvo_track_lk(sosvo_ctx* ctx, const uint8_t* gray, const uint8_t* pyr, int32_t nimg, int32_t rows, "
                  "int32_t cols, int32_t levels, const int32_t* row_range, const int32_t* prev_img, const int32_t* next_img, "
                  "int32_t nprob, int32_t cap, const float* prev_pts, const int32_t* n, int32_t half, int32_t max_iter, double eps, "
                  "double min_eig, int32_t flags, float* next_pts, uint8_t* status, float* err, float* back, double fb_max);"):
        assert proto in flat, proto
    assert "int32_t sosvo_f2f_assemble_tracked(sosvo_ctx* ctx, const sosvo_rig* rig_host," in flat
    i32, f64 = _lib.c_i32, _lib.c_f64
    restype, args = _lib.SIGNATURES["sosvo_track_lk"]
    assert restype is i32 and len(args) == 24
    assert [a is i32 for a in args] == [False] * 3 + [True] * 4 + [False] * 3 + [True] * 2 + [False] * 2 + [True] * 2 + \
        [False] * 2 + [True] + [False] * 5
    assert [a is f64 for a in args] == [False] * 16 + [True] * 2 + [False] * 5 + [True]
    assert len(_lib.SIGNATURES["sosvo_gray_pyramid"][1]) == 8 and len(_lib.SIGNATURES["sosvo_gray_pyramid_bytes"][1]) == 6
    assert len(_lib.SIGNATURES["sosvo_f2f_assemble_tracked"][1]) == 21
    for name in ("sosvo_gray_pyramid_bytes", "sosvo_gray_pyramid", "sosvo_track_lk", "sosvo_f2f_assemble_tracked"):
        assert name in _lib.declared_functions()
    assert (_lib.LK_MAX_HALF, _lib.LK_MAX_LEVELS, _lib.LK_MAX_ITER, _lib.LK_MAX_CAP) == (10, 4, 30, 4096)


def test_the_entries_refuse_a_null_context_and_the_size_helper_needs_none():
    lib = lib_or_skip()
    assert lib.sosvo_gray_pyramid(None, None, 2, 8, 8, 2, None, None) == -1
    assert lib.sosvo_track_lk(None, None, None, 2, 8, 8, 2, None, None, None, 1, 4, None, None, 4, 10, 0.01, 1e-4, 0, None, None,
                              None, None, 0.0) == -1
    assert lib.sosvo_f2f_assemble_tracked(None, *([None] * 5), 4, *([None] * 5), 1, 4, *([None] * 7)) == -1
    assert _lib.gray_pyramid_bytes(4, 96, 128, 3) == 4 * (48 * 64 + 24 * 32)
    assert _lib.gray_pyramid_bytes(2, 95, 127, 4) == 2 * (48 * 64 + 24 * 32 + 12 * 16)
    assert _lib.gray_pyramid_bytes(7, 300, 1200, 1) == 0
    for bad in ((2, 8, 8, 0), (2, 8, 8, 5), (2, 0, 8, 2), (2, 8, 16385, 2), (-1, 8, 8, 2)):
        with pytest.raises(_lib.SosvoError):
            _lib.gray_pyramid_bytes(*bad)


def test_lk_options_defaults_and_validation():
    o = _lib.LKOptions()
    assert o == (10, 3, 30, 0.01, 1e-4, None)                 # cv2.calcOpticalFlowPyrLK's: 21 x 21, maxLevel 2, (30, 0.01), 1e-4
    o = _lib.LKOptions(half=4, levels=1, max_iter=10, eps=0, min_eig=0, fb_max=0.5)
    assert o == (4, 1, 10, 0.0, 0.0, 0.5) and isinstance(o.eps, float) and hash(o) == hash(_lib.LKOptions(4, 1, 10, 0.0, 0.0, 0.5))
    assert _lib.LKOptions.of(None) == _lib.LKOptions() and _lib.LKOptions.of(o) is o
    assert _lib.LKOptions.of(dict(half=2, fb_max=1)) == _lib.LKOptions(half=2, fb_max=1.0)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(half=1), dict(half=11), dict(half=4.5), dict(half="4"), dict(half=True), dict(half=None), dict(levels=0),
                dict(levels=5), dict(levels=2.5), dict(max_iter=0), dict(max_iter=31), dict(eps=-1e-9), dict(eps=nan),
                dict(eps=inf), dict(eps="0.01"), dict(min_eig=-1.0), dict(min_eig=nan), dict(fb_max=0), dict(fb_max=-0.5),
                dict(fb_max=nan), dict(fb_max=inf), dict(fb_max=True)):
        with pytest.raises(ValueError, match="lk "):
            _lib.LKOptions(**bad)
    for bad in (dict(window=4), 4, "lk", (4, 3)):
        with pytest.raises(ValueError, match="lk"):
            _lib.LKOptions.of(bad)
    assert _lib.LKOptions(half=4.0).half == 4 and isinstance(_lib.LKOptions(half=4.0).half, int)      # (4.0 is 4: nothing rounded)


def test_the_public_interfaces_take_the_arguments():
    p = inspect.signature(pipeline.FramePairPipeline.__init__).parameters
    assert p["f2f_tracker"].default == "match" and p["lk"].default is None
    assert list(inspect.signature(Context.gray_pyramid).parameters)[1:] == ["gray", "levels", "row_range", "out"]
    sig = inspect.signature(Context.track_lk).parameters
    assert list(sig)[1:6] == ["pyr", "prev_img", "next_img", "prev_pts", "n"] and sig["next_pts"].default is None \
        and sig["fb_max"].default is None
    assert "f2f_assemble_tracked" in dir(Context)
    sig = inspect.signature(common_cv.calc_optical_flow_pyr_lk).parameters
    assert list(sig)[:9] == ["prev_gray", "next_gray", "prev_pts", "next_pts", "win_half", "max_level", "max_iter", "eps",
                             "min_eig_threshold"]
    assert [sig[k].default for k in list(sig)[3:9]] == [None, 10, 2, 30, 0.01, 1e-4]


def test_the_pipeline_refuses_the_tracker_without_a_front_end_and_bad_settings():
    ctx, fe = _ctx(), _front_end()
    with pytest.raises(ValueError, match="front end"):
        pipeline.FramePairPipeline(ctx, _rig(), 2, f2f_tracker="lk")
    with pytest.raises(ValueError, match="f2f_tracker"):
        pipeline.FramePairPipeline(ctx, _rig(), 2, front_end=fe, f2f_tracker="klt")
    with pytest.raises(ValueError, match="lk half"):
        pipeline.FramePairPipeline(ctx, _rig(), 2, front_end=fe, f2f_tracker="lk", lk=dict(half=11))
    with pytest.raises(ValueError, match="lk"):
        pipeline.FramePairPipeline(ctx, _rig(), 2, front_end=fe, lk=dict(half=4))          # settings without the tracker


def test_the_default_builds_what_it_built_before():
    """No tracker: the MatchOptions value, the tensors (names and shapes, listed above from the code before the option) and the
    search settings are those of a pipeline that has never heard of the option; "match" spelt out is the default."""
    ctx = _ctx()
    a = pipeline.FramePairPipeline(ctx, _rig(), 2, nmask=3, bucket_cap=8, frame_cap=16)
    b = pipeline.FramePairPipeline(ctx, _rig(), 2, nmask=3, bucket_cap=8, frame_cap=16, f2f_tracker="match")
    for p in (a, b):
        assert p.opts == _lib.MatchOptions() and p.opts.flags() == 0 and p.lk is None and p.f2f_tracker == "match"
        assert _tensors(p) == BUFFERS
        assert not [k for k in vars(p) if k.startswith("_lk")]
        assert p._f2f_search == dict(ratio_64ths=0, rivals=None, gate=None)
        assert {k: tuple(v.shape) for k, v in p.corr.items()} == dict(f=(2, 32, 3), p=(2, 32, 3), cam=(2, 32), q=(2, 32), t=(2, 32),
                                                                      n=(2,), n_top=(2,))
    o = pipeline.FramePairPipeline(ctx, _rig(), 2, nmask=3, bucket_cap=8, frame_cap=16, ratio_f2f=True, ratio=0.75, cross_check_f2f=True)
    assert o.opts == _lib.MatchOptions(cross_check_f2f=True, ratio_f2f=True, ratio=0.75) and o.lk is None


@pytest.mark.parametrize("keep_panoramas,fb_max", [(False, None), (True, 0.5)])
def test_track_with_the_tracker_asks_the_context_for_the_new_stages(keep_panoramas, fb_max):
    ctx, fe = _ctx(), _front_end(keep_panoramas)
    calls = []
    pipe = pipeline.FramePairPipeline(ctx, _rig(), 2, frame_cap=16, front_end=fe, f2f_tracker="lk",
                                      lk=dict(half=4, levels=2, max_iter=7, fb_max=fb_max))
    assert pipe.lk == _lib.LKOptions(4, 2, 7, 0.01, 1e-4, fb_max)
    extra = {k: v for k, v in _tensors(pipe).items() if k not in BUFFERS}
    assert extra == dict(_lk_prev=(4, 16, 2), _lk_n=(4,), _lk_ref=(4,))
    assert [tuple(t.shape) for t in pipe._lk_out] == [(4, 16, 2), (4, 16), (4, 16)] + ([(4, 16, 2)] if fb_max else [])
    pipe._m2.copy_(torch.arange(2 * 4 * 16 * 2, dtype=torch.float32).view(2, 4, 16, 2))
    pipe._M2[0].copy_(torch.tensor([5, 6, 7, 8], dtype=torch.int32))

    def record(name, result=None):
        def call(*a, **k):
            calls.append((name, a, k))
            return result(*a, **k) if callable(result) else result
        return call
    for name in ("match_1nn_slots", "sort_matches", "f2f_assemble", "ransac_abs_pose", "refine_abs_pose", "f2f_assemble_tracked"):
        setattr(ctx, name, record(name))
    ctx.gray_pyramid = record("gray_pyramid", "PYR")
    ctx.track_lk = record("track_lk", lambda *a, **k: k["out"])
    pipe.track()
    assert [c[0] for c in calls] == ["gray_pyramid", "track_lk", "f2f_assemble_tracked", "ransac_abs_pose", "refine_abs_pose"]
    (_, a, k) = calls[0]
    assert a[0] is fe.gray and a[1] == 2 and (k["row_range"] is None if keep_panoramas else k["row_range"] is fe.gray_rows)
    (_, a, k) = calls[1]
    assert a[0] == "PYR"
    # 2B problems: the top views' (reference -> current) images, then the bottom views' (offset F = 4)
    assert a[1].tolist() == [0, 2, 4, 6] and a[2].tolist() == [1, 3, 5, 7]
    assert np.array_equal(a[3].numpy(), pipe._m2.view(8, 16, 2)[[0, 2, 4, 6]].numpy())       # the reference frames' points
    assert a[4].tolist() == [5, 7, 5, 7]                                                       # ... and their counts
    assert (k["half"], k["max_iter"], k["eps"], k["min_eig"], k["fb_max"]) == (4, 7, 0.01, 1e-4, fb_max) and "next_pts" not in k
    (_, a, k) = calls[2]
    assert a[1] is pipe.frames and a[2] is pipe.ref_frame and k["out"] is pipe.corr and a[7] == pipe.corr_cap
    nxt, st = pipe._lk_out[0], pipe._lk_out[1]
    assert a[3].data_ptr() == nxt[:2].data_ptr() and a[4].data_ptr() == nxt[2:].data_ptr()
    assert a[5].data_ptr() == st[:2].data_ptr() and a[6].data_ptr() == st[2:].data_ptr()
    # the matcher's path is untouched by the option
    calls[:] = []
    plain = pipeline.FramePairPipeline(ctx, _rig(), 2, frame_cap=16, front_end=fe)
    plain.track()
    assert [c[0] for c in calls] == ["match_1nn_slots", "sort_matches", "f2f_assemble", "ransac_abs_pose", "refine_abs_pose"]
