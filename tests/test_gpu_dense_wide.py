"""GPU: dense omnistereo with D = 16 .. 256 disparities (sosvo_dense_stereo_wide).  The device reproduces
tests/refdense_wide.py -- the aggregated volume S and the disparity map d16 -- bit for bit for every lane width (one, two and
four disparities per lane), with and without idle lanes, at the smallest shapes where an index can go wrong, on planted shifts
whose winner is k* = 255, where S uses its sixteenth bit, and at long and limit shapes; D = 64 is sosvo_dense_stereo_paths; the
refusals launch nothing; the engine and the host mirror equal the staged calls.  array_equal throughout.
tests/test_dense_wide_reference.py pins the numpy statement from outside on the same scenes."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_long_cases as long_cases  # noqa: E402
import refdense  # noqa: E402
import refdense_wide  # noqa: E402
import refspeckle  # noqa: E402
import test_dense_wide_reference as scenes  # noqa: E402
from test_gpu_dense import _dev, _frames, _mask, _rig_cfg, rig  # noqa: E402, F401
from test_gpu_dense8 import _shifted  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 70), (70, 1), (12, 9), (70, 5), (5, 70), (64, 64), (130, 33)]
# one disparity per lane with 48 and 16 idle lanes; two with 24 idle lanes and with none; four with 28 and 4 idle lanes and with none
DISPARITIES = [16, 48, 80, 128, 144, 240, 256]
# (P1, P2, uniqueness, lr_max, d0) of section 39; the last one at the eight-path limit of P2
OPTION_SETS = [(8, 48, 15, 1, 0), (0, 0, 0, -1, 1), (50, 1000, 15, 0, 7), (8127, 8127, 99, 63, 0)]
PATH_NAMES = ["dense_wide_down_kernel", "dense_wide_path_kernel_up", "dense_wide_path_kernel_lr", "dense_wide_path_kernel_rl"]
DIAG_NAMES = ["dense_wide_diag_kernel_dr", "dense_wide_diag_kernel_dl", "dense_wide_diag_kernel_ur", "dense_wide_diag_kernel_ul"]


def _ref_S(top, bot, d0, P1, P2, cyclic, paths, D):
    cen = refdense.census(np.concatenate([top, bot]), cyclic)
    n = len(top)
    return np.stack([refdense_wide.aggregate(refdense_wide.cost_volume(cen[k], cen[n + k], d0, D), P1, P2, paths, cyclic) for k in range(n)])


def _check(ctx, top, bot, opts, cyclic, paths, D, masks, scratch=True):
    """S and d16 of the device against refdense_wide, for every mask of `masks`; S in the caller's buffer and (scratch) in the
    library's."""
    from vo_single_camera_sos_amd import dense_wide
    from vo_single_camera_sos_amd._lib import DenseOptions
    P1, P2, uniq, lr_max, d0 = opts
    o = DenseOptions(min_disparity=d0, P1=P1, P2=P2, uniqueness=uniq, lr_max=lr_max, cyclic=cyclic)
    t_top, t_bot = _dev(ctx, top), _dev(ctx, bot)
    want_S = _ref_S(top, bot, d0, P1, P2, cyclic, paths, D)
    for m in masks:
        t_m = None if m is None else _dev(ctx, m)
        d16, S = dense_wide.dense_stereo(ctx, t_top, t_bot, t_m, options=o, disparities=D, paths=paths, want_volume=True)
        only = dense_wide.dense_stereo(ctx, t_top, t_bot, t_m, options=o, disparities=D, paths=paths) if scratch else d16
        ctx.synchronize()
        assert S.shape == top.shape + (D,)
        S, d16, only = S.cpu().numpy(), d16.cpu().numpy(), only.cpu().numpy()
        assert np.array_equal(S, want_S), ("S", D, paths, cyclic, np.argwhere(S != want_S)[:5])
        del S
        want = np.stack([refdense_wide.select(s, d0, uniq, lr_max, m) for s in want_S])
        assert np.array_equal(d16, want), ("d16", D, paths, cyclic, m is not None, np.argwhere(d16 != want)[:5])
        assert np.array_equal(only, want), ("d16, S in the scratch", D, paths, cyclic, m is not None)
    return want_S


@pytest.mark.parametrize("opts", OPTION_SETS, ids=lambda o: "P%d_%d_u%d_lr%d_d%d" % o)
@pytest.mark.parametrize("D", DISPARITIES, ids=lambda d: "D%d" % d)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_volume_and_disparities_equal_the_numpy_statement(ctx, shape, D, opts):
    top, bot = _frames(*shape)
    for paths in (4, 8):
        for cyclic in (False, True):
            _check(ctx, top, bot, opts, cyclic, paths, D, (None, _mask(*shape)))


@pytest.mark.parametrize("D", (48, 144, 256), ids=lambda d: "D%d" % d)
def test_result_does_not_depend_on_the_scratch(ctx, D):
    from vo_single_camera_sos_amd import dense_wide
    from vo_single_camera_sos_amd._lib import DenseOptions
    top, bot = _frames(130, 33)
    t_top, t_bot, mask = _dev(ctx, top), _dev(ctx, bot), _dev(ctx, _mask(130, 33))
    for cyclic in (False, True):
        got = []
        for byte in (None, 0xFF, 0x00):
            if byte is not None:
                ctx.debug_fill_scratch(byte)
            d16 = dense_wide.dense_stereo(ctx, t_top, t_bot, mask, options=DenseOptions(cyclic=cyclic), disparities=D, paths=8)
            ctx.synchronize()
            got.append(d16.cpu().numpy().tobytes())
        assert got[0] == got[1] == got[2]


@pytest.mark.parametrize("case", scenes.PLANTED, ids=lambda c: "D%d_shift%d_d%d" % c)
def test_planted_shifts_beyond_63_rows(ctx, case):
    """The planted shifts of test_dense_wide_reference at 300 x 24; where the winner is k* = 255 (a byte's "dropped" marker) with
    lr_max 0 and 1: the left-right check reads the kept k* of other pixels."""
    from vo_single_camera_sos_amd import dense_wide
    from vo_single_camera_sos_amd._lib import DenseOptions
    D, shift, d0 = case
    top, bot = scenes.planted(shift)
    t, b = _dev(ctx, top[None]), _dev(ctx, bot[None])
    want_S = refdense_wide.aggregate(refdense_wide.cost_volume(refdense.census(top), refdense.census(bot), d0, D), 8, 48)
    for lr_max in ((1, 0) if shift - d0 == 255 else (1,)):
        d16, S = dense_wide.dense_stereo(ctx, t, b, None, options=DenseOptions(min_disparity=d0, lr_max=lr_max), disparities=D, want_volume=True)
        ctx.synchronize()
        d16 = d16.cpu().numpy()[0]
        assert np.array_equal(S.cpu().numpy()[0], want_S)
        assert np.array_equal(d16, refdense_wide.select(want_S, d0, 15, lr_max)), lr_max
        assert scenes.planted_share(d16, shift) >= 0.97
        if shift - d0 == 255:
            assert ((d16 >= 0) & (want_S.argmin(axis=-1) == 255)).sum() >= 500


@pytest.mark.parametrize("cyclic", (False, True), ids=("clamped", "cyclic"))
def test_S_above_32767_is_read_as_unsigned(ctx, cyclic):
    """The sign-bit case of test_dense_wide_reference at D = 128: more than 0.4 (clamped) / 0.9 (cyclic) of S lies above 32767."""
    from vo_single_camera_sos_amd import dense_wide
    from vo_single_camera_sos_amd._lib import DenseOptions
    img, (want, want_S) = scenes.sign_bit_volume(cyclic)
    assert (want_S > 32767).mean() >= (0.9 if cyclic else 0.4)
    t = _dev(ctx, img[None])
    o = DenseOptions(min_disparity=0, P1=8127, P2=8127, cyclic=cyclic)
    d16, S = dense_wide.dense_stereo(ctx, t, t, None, options=o, disparities=128, paths=8, want_volume=True)
    ctx.synchronize()
    S, d16 = S.cpu().numpy()[0], d16.cpu().numpy()[0]
    assert np.array_equal(S, want_S), np.argwhere(S != want_S)[:5]
    assert np.array_equal(d16, want), np.argwhere(d16 != want)[:5]


# name -> (frames, opts, cyclic, paths, D): lines that wrap a hundred times and a row path of 700; the row and the column limit
# with four disparities per lane; blockIdx.y up to 129; the working size
LONG = {
    "300x3_D240": (lambda: _shifted(300, 3, 2, 5), (50, 1000, 15, 0, 1), False, 8, 240),
    "3x700_cyclic_D80": (lambda: _shifted(3, 700, 2), (8, 48, 15, 1, 0), True, 8, 80),
    "16384x2_D256": (lambda: _shifted(16384, 2, 2, 5), (8, 48, 15, 1, 1), True, 8, 256),
    "3x16384_D256": (lambda: _shifted(3, 16384, 2), (8, 48, 15, 1, 0), False, 8, 256),
    "130_frames_5x3_D128": (lambda: long_cases.frames("many_small"), (8, 48, 15, 1, 0), True, 8, 128),
    "146x1440_cyclic_D128": (lambda: long_cases.frames("working"), (8, 48, 15, 1, 1), True, 4, 128),
}


@pytest.mark.parametrize("name", list(LONG))
def test_long_and_limit_shapes_equal_the_numpy_statement(ctx, name):
    make, opts, cyclic, paths, D = LONG[name]
    top, bot = make()
    _check(ctx, top, bot, opts, cyclic, paths, D, (None,), scratch=False)


def _raw_wide(ctx, t_top, t_bot, D, paths=4, P1=8, P2=48, flags=0, want_S=True, **kw):
    """sosvo_dense_stereo_wide as the library exports it -> (status, d16, S)."""
    import torch
    from vo_single_camera_sos_amd import dense_wide
    n, rows, cols = t_top.shape
    d16 = torch.zeros((n, rows, cols), dtype=torch.int16, device=ctx.device)
    S = torch.zeros((n, rows, cols, D), dtype=torch.uint16, device=ctx.device) if want_S else None
    a = dict(top=ctypes.c_void_p(t_top.data_ptr()), bot=ctypes.c_void_p(t_bot.data_ptr()), n=n, rows=rows, cols=cols, d0=1, P1=P1, P2=P2,
             uniq=15, lr=1, flags=flags, paths=paths, out=ctypes.c_void_p(d16.data_ptr()))
    a.update(kw)
    rc = dense_wide.load().sosvo_dense_stereo_wide(ctx._h, a["top"], a["bot"], a["n"], a["rows"], a["cols"], None, a["d0"], D, a["P1"],
                                                   a["P2"], a["uniq"], a["lr"], a["flags"], a["paths"], a["out"],
                                                   None if S is None else ctypes.c_void_p(S.data_ptr()))
    return rc, d16, S


def test_sixty_four_disparities_are_the_existing_entry_point(ctx):
    """disparities = 64: the bytes and exactly the kernel profile of sosvo_dense_stereo_paths, four and eight paths; any other D:
    the new kernels by name, eight paths giving four diagonal launches more after the right-to-left pass."""
    from vo_single_camera_sos_amd import dense_wide
    from vo_single_camera_sos_amd._lib import DenseOptions
    top, bot = _frames(70, 5)
    t, b = _dev(ctx, top), _dev(ctx, bot)
    for flags in (0, 1):
        o = DenseOptions(cyclic=bool(flags))
        for paths in (4, 8):
            ctx.profile_enable(True)
            want_d16, want_S = ctx.dense_stereo(t, b, None, options=o, want_volume=True, paths=paths)
            ctx.synchronize()
            old = [name for name, _ in ctx.profile_read()]
            ctx.profile_enable(True)
            rc, d16, S = _raw_wide(ctx, t, b, 64, paths, flags=flags)
            ctx.synchronize()
            raw = [name for name, _ in ctx.profile_read()]
            ctx.profile_enable(True)
            d16_py, S_py = dense_wide.dense_stereo(ctx, t, b, None, options=o, disparities=64, paths=paths, want_volume=True)
            ctx.synchronize()
            py = [name for name, _ in ctx.profile_read()]
            assert rc == 0 and raw == old == py and len(old) >= 7 and not any("wide" in name for name in old)
            for got in (d16, d16_py):
                assert got.cpu().numpy().tobytes() == want_d16.cpu().numpy().tobytes()
            for got in (S, S_py):
                assert got.cpu().numpy().tobytes() == want_S.cpu().numpy().tobytes()
        for D in (48, 128, 256):
            names = {}
            for paths in (4, 8):
                ctx.profile_enable(True)
                assert _raw_wide(ctx, t, b, D, paths, flags=flags)[0] == 0
                ctx.synchronize()
                names[paths] = [name for name, _ in ctx.profile_read()]
            assert len(names[4]) == 8 and all(name.startswith("dense_census_kernel") for name in names[4][:2]), names[4]
            assert names[4][2:] == PATH_NAMES + ["dense_wide_select_kernel", "dense_wide_left_right_kernel"], names[4]
            assert names[8] == names[4][:6] + DIAG_NAMES + names[4][6:]
        ctx.profile_enable(False)


@pytest.mark.parametrize("shape", ((70, 5), (130, 33)), ids=lambda s: "%dx%d" % s)
def test_the_new_kernels_at_sixty_four_disparities_equal_the_existing_ones(ctx, shape):
    """One disparity per lane and no idle lane: the entry point never runs the new kernels at D = 64, the hook
    sosvo_debug_dense_stereo_wide_kernels (in no header; scripts/bench_dense_wide.py times through it) does.  S and d16 equal
    refdense_wide and the bytes of Context.dense_stereo, four and eight paths, clamped and cyclic, under the new kernels' names."""
    from vo_single_camera_sos_amd import dense_wide
    from vo_single_camera_sos_amd._lib import DenseOptions
    top, bot = _frames(*shape)
    t, b, m = _dev(ctx, top), _dev(ctx, bot), _dev(ctx, _mask(*shape))
    for paths in (4, 8):
        for cyclic in (False, True):
            o = DenseOptions(min_disparity=0, cyclic=cyclic)
            want_d16, want_S = ctx.dense_stereo(t, b, m, options=o, want_volume=True, paths=paths)
            ctx.profile_enable(True)
            d16, S = dense_wide.debug_dense_stereo_wide_kernels(ctx, t, b, m, options=o, disparities=64, paths=paths, want_volume=True)
            ctx.synchronize()
            names = [name for name, _ in ctx.profile_read()]
            ctx.profile_enable(False)
            assert names[2:6] == PATH_NAMES and names[-2:] == ["dense_wide_select_kernel", "dense_wide_left_right_kernel"]
            assert [name for name in names if "diag" in name] == (DIAG_NAMES if paths == 8 else [])
            assert np.array_equal(S.cpu().numpy(), _ref_S(top, bot, 0, 8, 48, cyclic, paths, 64))
            assert S.cpu().numpy().tobytes() == want_S.cpu().numpy().tobytes()
            assert d16.cpu().numpy().tobytes() == want_d16.cpu().numpy().tobytes()


def test_argument_refusals_launch_nothing(ctx):
    """Every refusal of sosvo_dense_stereo_wide returns SOSVO_ERR_ARG before any launch, under its own name: what
    sosvo_dense_stereo_paths refuses, then the disparities; the Python layer raises ValueError before the call."""
    from vo_single_camera_sos_amd import dense_wide
    from vo_single_camera_sos_amd._lib import DenseOptions
    top, bot = _frames(12, 9)
    t, b = _dev(ctx, top), _dev(ctx, bot)
    ctx.profile_enable(True)
    disparities = "disparities out of range (16..256, a multiple of 16)"
    bad = [(dict(rows=0), "rows / cols out of range (1..16384)"), (dict(cols=0), None), (dict(rows=16385), None), (dict(cols=16385), None),
           (dict(n=0), "n out of range (1..32767)"), (dict(n=32768), None),
           (dict(P1=49), "penalties out of range (0 <= P1 <= P2 <= 8191)"), (dict(P2=8192, P1=0, paths=4), None), (dict(P1=-1), None),
           (dict(uniq=-1), "uniqueness out of range (0..99)"), (dict(uniq=100), None),
           (dict(d0=-1), "min_disparity out of range (0..1024)"), (dict(d0=1025), None),
           (dict(flags=2), "unknown flag bits"), (dict(flags=-1), None),
           (dict(top=None), "null pointer"), (dict(bot=None), None), (dict(out=None), None),
           (dict(paths=0), "paths must be 4 or 8"), (dict(paths=5), None), (dict(paths=-8), None), (dict(paths=16), None),
           (dict(P2=8128, P1=0), "eight paths need P2 <= 8127 (S stays 16 bits)"), (dict(P2=8191, P1=8191), None),
           (dict(D=0), disparities), (dict(D=8), disparities), (dict(D=15), disparities), (dict(D=17), disparities), (dict(D=72), disparities),
           (dict(D=100), disparities), (dict(D=255), disparities), (dict(D=257), disparities), (dict(D=272), disparities),
           (dict(D=512), disparities), (dict(D=-16), disparities), (dict(D=-64), disparities),
           (dict(D=300, rows=0), "rows / cols out of range (1..16384)"), (dict(D=300, paths=5), "paths must be 4 or 8")]
    for kw, message in bad:
        for D in ((kw.pop("D"),) if "D" in kw else (64, 128)):      # the 64-disparity route refuses under the new name as well
            rc, _, _ = _raw_wide(ctx, t, b, D, kw.get("paths", 8), want_S=False, **{k: v for k, v in kw.items() if k != "paths"})
            assert rc == -1, (kw, D)
            if message is not None:
                assert ctx._lib.sosvo_last_error(ctx._h).decode() == "sosvo_dense_stereo_wide: " + message, (kw, D)
    assert ctx.profile_read() == []
    assert _raw_wide(ctx, t, b, 16, 4, P1=8191, P2=8191)[0] == 0 and _raw_wide(ctx, t, b, 256, 8, P1=8127, P2=8127)[0] == 0
    assert _raw_wide(ctx, t, b, 240, 8, P1=0, P2=0, lr=-5)[0] == 0
    ctx.synchronize()
    names = [name for name, _ in ctx.profile_read()]
    assert [name for name in names if "diag" in name] == DIAG_NAMES * 2 and names.count("dense_wide_left_right_kernel") == 2
    ctx.profile_enable(True)
    for kw in (dict(disparities=0), dict(disparities=72), dict(disparities=272), dict(disparities="128"), dict(disparities=128.0),
               dict(disparities=True), dict(disparities=None), dict(disparities=-16), dict(disparities=128, paths=6),
               dict(disparities=128, paths=8, options=DenseOptions(P1=0, P2=8128)), dict(disparities=64, paths=8, options=dict(P2=8191))):
        with pytest.raises(ValueError):
            dense_wide.dense_stereo(ctx, t, b, **kw)
    assert ctx.profile_read() == []
    ctx.profile_enable(False)


@pytest.fixture(scope="module")
def staged(ctx, rig):
    """The device's gray panoramas of the rig's two frames, the engine's mask, and refdense_wide's maps of them at D = 128,
    min_disparity 0, cyclic, with four and eight paths."""
    from vo_single_camera_sos_amd.frontend import DeviceImageModel
    from vo_single_camera_sos_amd.pipeline import dense_mask
    model = DeviceImageModel(ctx, rig["gs"], (480, 640))
    mask = dense_mask(ctx, model)
    gray = ctx.unwrap_median_gray(_dev(ctx, rig["omni"]), model.unwrap_table, 0)
    ctx.synchronize()
    g, mask_h = gray.cpu().numpy(), mask.cpu().numpy()
    want = {paths: np.stack([refdense_wide.dense_stereo(g[k], g[2 + k], mask_h, min_disparity=0, cyclic=True, paths=paths, disparities=128)
                             for k in range(2)]) for paths in (4, 8)}
    return dict(model=model, mask=mask, gray=gray, want=want)


def test_engine_equals_the_staged_calls_and_the_numpy_statement(ctx, rig, staged):
    from vo_single_camera_sos_amd import dense_wide
    from vo_single_camera_sos_amd._lib import DenseOptions, SpeckleOptions, WlsOptions
    from vo_single_camera_sos_amd import dense_filter
    from vo_single_camera_sos_amd.pipeline import DenseOmniStereo
    model, mask, gray = staged["model"], staged["mask"], staged["gray"]
    cfg, o = _rig_cfg(rig), DenseOptions(min_disparity=0, cyclic=True)
    sp, wls = SpeckleOptions(max_size=12, max_diff=16, cyclic=True), WlsOptions(cyclic=True)
    top, bot = gray[:2].contiguous(), gray[2:].contiguous()
    raw = {paths: dense_wide.dense_stereo(ctx, top, bot, mask, options=o, disparities=128, paths=paths) for paths in (4, 8)}
    raw64 = ctx.dense_stereo(top, bot, mask, options=o)
    ctx.synchronize()
    for paths in (4, 8):
        assert np.array_equal(raw[paths].cpu().numpy(), staged["want"][paths])
    assert not np.array_equal(staged["want"][4], staged["want"][8])      # (33 rows: no disparity beyond 32 can win, the kernels differ)
    filtered = dense_filter.dense_wls(ctx, raw[4].clone(), top, options=wls, conf=dense_filter.dense_confidence(ctx, raw[4], options=wls), mask=mask)
    ctx.synchronize()
    cases = [(dict(), staged["want"][4]), (dict(paths=8), staged["want"][8]),
             (dict(speckle=sp), refspeckle.speckle(staged["want"][4], 12, 16, cyclic=True)), (dict(wls=wls), filtered.cpu().numpy())]
    for kw, want in cases:
        eng = DenseOmniStereo(ctx, model, cfg, 2, options=o, disparities=128, **kw)
        assert eng.disparities == 128
        eng.load_frames(rig["omni"])
        ctx.profile_enable(True)
        d16, X = eng.step()
        ctx.synchronize()
        names = [name for name, _ in ctx.profile_read()]
        ctx.profile_enable(False)
        assert "dense_wide_select_kernel" in names and "dense_select_kernel" not in names
        assert [name for name in names if "diag" in name] == (DIAG_NAMES if kw.get("paths") == 8 else [])
        want_X = ctx.dense_triangulate(cfg.as_struct(), _dev(ctx, want), 1.0, 0.0)
        ctx.synchronize()
        assert np.array_equal(d16.cpu().numpy(), want), (kw, np.argwhere(d16.cpu().numpy() != want)[:5])
        assert np.array_equal(X.cpu().numpy(), want_X.cpu().numpy(), equal_nan=True)
    profiles = []
    for kw in (dict(), dict(disparities=64)):         # 64: the engine as it was, bytes and launches
        eng = DenseOmniStereo(ctx, model, cfg, 2, options=o, **kw)
        assert eng.disparities == 64
        eng.load_frames(rig["omni"])
        ctx.profile_enable(True)
        d16, _ = eng.step()
        ctx.synchronize()
        profiles.append([name for name, _ in ctx.profile_read()])
        ctx.profile_enable(False)
        assert d16.cpu().numpy().tobytes() == raw64.cpu().numpy().tobytes()
    assert profiles[0] == profiles[1] and profiles[0] and not any("wide" in name for name in profiles[0])
    for kw in (dict(disparities=72), dict(disparities=0), dict(disparities=128, paths=8, options=DenseOptions(P1=0, P2=8128))):
        with pytest.raises(ValueError):
            DenseOmniStereo(ctx, model, cfg, 2, **kw)


def test_host_mirror_gives_the_engines_numbers(ctx, rig):
    from vo_single_camera_sos_amd._lib import DenseOptions
    from vo_single_camera_sos_amd.frontend import DeviceImageModel
    from vo_single_camera_sos_amd.pipeline import DenseOmniStereo
    gs, o = rig["gs"], DenseOptions()
    maps = {}
    for D in (64, 128):
        eng = DenseOmniStereo(ctx, DeviceImageModel(ctx, gs, (480, 640)), _rig_cfg(rig, 0.0, 0.0), 1, options=o, min_disparity=0.0,
                              disparities=D)
        eng.load_frames(rig["omni"][:1])
        d16, _ = eng.step()
        ctx.synchronize()
        maps[D] = d16.cpu().numpy()[0]
    gs.__dict__.pop("_dense_engines", None)
    gs.set_current_omni_image(rig["omni"][0], generate_panoramas=True)
    dmap0, dimg0 = gs.get_depth_map_from_panoramas(method="sgbm", options=o)                    # as before the keyword existed
    assert np.array_equal(gs.disparity_d16, maps[64])
    dmap64, dimg64 = gs.get_depth_map_from_panoramas(method="sgbm", options=o, disparities=64)
    assert np.array_equal(dmap64, dmap0) and np.array_equal(dimg64, dimg0) and len(gs._dense_engines) == 1
    assert np.array_equal(dimg0, np.where(maps[64] >= 0, np.clip((maps[64] / 16.0 - 1) * 255.0 / 63, 0, 255), 0).astype(np.uint8))
    num_of_disparities = 128                                                                     # the tuner's slider
    dmap, dimg = gs.get_depth_map_from_panoramas(method="sgbm", options=o, disparities=num_of_disparities)
    d16 = maps[128]
    assert np.array_equal(gs.disparity_d16, d16) and len(gs._dense_engines) == 2
    assert np.array_equal(dmap, np.where(d16 >= 0, d16 / 16.0, 0.0)) and np.array_equal(dmap == 0, d16 == -1)
    assert np.array_equal(dimg, np.where(d16 >= 0, np.clip((d16 / 16.0 - 1) * 255.0 / 127, 0, 255), 0).astype(np.uint8))
    assert not np.array_equal(dimg, dimg0)            # (the image scales by the number of disparities where it had 64)
    with pytest.raises(ValueError):
        gs.get_depth_map_from_panoramas(method="sgbm", options=o, disparities=100)
