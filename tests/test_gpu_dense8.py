"""GPU: dense omnistereo with eight aggregation paths (sosvo_dense_stereo_paths).  The device reproduces
tests/refdense8.py -- the aggregated volume S and the disparity map d16 -- bit for bit at the smallest shapes where an index
can go wrong, where S uses its sixteenth bit, and at long and limit shapes; paths = 4 is sosvo_dense_stereo; the refusals
launch nothing; the engine and the host mirror equal the staged calls.  array_equal throughout.
tests/test_dense8_reference.py shows that these inputs can tell the forms apart."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_long_cases as long_cases  # noqa: E402
import refdense  # noqa: E402
import refdense8  # noqa: E402
import refspeckle  # noqa: E402
from test_dense8_reference import sign_bit_volume  # noqa: E402
from test_gpu_dense import _dev, _frames, _mask, _rig_cfg, _texture, rig  # noqa: E402, F401

pytestmark = pytest.mark.gpu

# test_gpu_dense.SHAPES and 5 x 70: fewer rows than columns, a line that wraps fourteen times
SHAPES = [(1, 70), (70, 1), (12, 9), (70, 5), (5, 70), (64, 64), (130, 33)]
# (P1, P2, uniqueness, lr_max, d0); the last one at the eight-path limit of P2
OPTION_SETS = [(8, 48, 15, 1, 0), (0, 0, 0, -1, 1), (50, 1000, 15, 0, 7), (8127, 8127, 99, 63, 0)]
DIAG_NAMES = ["dense_diag_kernel_dr", "dense_diag_kernel_dl", "dense_diag_kernel_ur", "dense_diag_kernel_ul"]


def _ref_S(top, bot, d0, P1, P2, cyclic):
    cen = refdense.census(np.concatenate([top, bot]), cyclic)
    n = len(top)
    return np.stack([refdense8.aggregate(refdense.cost_volume(cen[k], cen[n + k], d0), P1, P2, 8, cyclic) for k in range(n)])


def _check(ctx, top, bot, opts, cyclic, masks, scratch=True):
    """S and d16 of the device with eight paths against refdense8, for every mask of `masks`; S in the caller's buffer and
    (scratch) in the library's."""
    from vo_single_camera_sos_amd._lib import DenseOptions
    P1, P2, uniq, lr_max, d0 = opts
    o = DenseOptions(min_disparity=d0, P1=P1, P2=P2, uniqueness=uniq, lr_max=lr_max, cyclic=cyclic)
    t_top, t_bot = _dev(ctx, top), _dev(ctx, bot)
    want_S = _ref_S(top, bot, d0, P1, P2, cyclic)
    for m in masks:
        t_m = None if m is None else _dev(ctx, m)
        d16, S = ctx.dense_stereo(t_top, t_bot, t_m, options=o, want_volume=True, paths=8)
        only = ctx.dense_stereo(t_top, t_bot, t_m, options=o, paths=8) if scratch else d16
        ctx.synchronize()
        S, d16, only = S.cpu().numpy(), d16.cpu().numpy(), only.cpu().numpy()
        assert np.array_equal(S, want_S), ("S", cyclic, np.argwhere(S != want_S)[:5])
        del S
        want = np.stack([refdense.select(s, d0, uniq, lr_max, m) for s in want_S])
        assert np.array_equal(d16, want), ("d16", cyclic, m is not None, np.argwhere(d16 != want)[:5])
        assert np.array_equal(only, want), ("d16, S in the scratch", cyclic, m is not None)
    return want_S


@pytest.mark.parametrize("opts", OPTION_SETS, ids=lambda o: "P%d_%d_u%d_lr%d_d%d" % o)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_volume_and_disparities_equal_the_numpy_statement(ctx, shape, opts):
    top, bot = _frames(*shape)
    for cyclic in (False, True):
        _check(ctx, top, bot, opts, cyclic, (None, _mask(*shape)))


def test_result_does_not_depend_on_the_scratch(ctx):
    from vo_single_camera_sos_amd._lib import DenseOptions
    top, bot = _frames(130, 33)
    t_top, t_bot, mask = _dev(ctx, top), _dev(ctx, bot), _dev(ctx, _mask(130, 33))
    for cyclic in (False, True):
        got = []
        for byte in (None, 0xFF, 0x00):
            if byte is not None:
                ctx.debug_fill_scratch(byte)
            d16 = ctx.dense_stereo(t_top, t_bot, mask, options=DenseOptions(cyclic=cyclic), paths=8)
            ctx.synchronize()
            got.append(d16.cpu().numpy().tobytes())
        assert got[0] == got[1] == got[2]


@pytest.mark.parametrize("cyclic", (False, True), ids=("clamped", "cyclic"))
def test_S_above_32767_is_read_as_unsigned(ctx, cyclic):
    """The sign-bit case of test_dense8_reference: more than 0.4 (clamped) / 0.9 (cyclic) of S lies above 32767."""
    from vo_single_camera_sos_amd._lib import DenseOptions
    img, (want, want_S) = sign_bit_volume(cyclic)
    assert (want_S > 32767).mean() > 0.4
    t = _dev(ctx, img[None])
    o = DenseOptions(min_disparity=0, P1=8127, P2=8127, cyclic=cyclic)
    d16, S = ctx.dense_stereo(t, t, None, options=o, want_volume=True, paths=8)
    ctx.synchronize()
    S, d16 = S.cpu().numpy()[0], d16.cpu().numpy()[0]
    assert np.array_equal(S, want_S), np.argwhere(S != want_S)[:5]
    assert np.array_equal(d16, want), np.argwhere(d16 != want)[:5]


def _shifted(rows, cols, n, shift=1):
    """n frames [rows, cols] with textures of their own, the bottom view the top shifted by `shift` rows plus noise in +-3."""
    rng = np.random.default_rng(rows * 1000 + cols + 8)
    top, bot = [], []
    for _ in range(n):
        t = _texture(rng, rows + shift, cols)
        top.append(t[:rows])
        bot.append(np.clip(t[shift:].astype(np.int32) + rng.integers(-3, 4, (rows, cols)), 0, 255).astype(np.uint8))
    return np.ascontiguousarray(np.stack(top)), np.ascontiguousarray(np.stack(bot))


# name -> (frames, opts, cyclic): lines that wrap a hundred times and a row path of 700; the row and the column limit; blockIdx.y
# up to 129; the working size
LONG = {
    "300x3_cyclic": (lambda: _shifted(300, 3, 2, 5), (8, 48, 15, 1, 0), True),
    "3x700_cyclic": (lambda: _shifted(3, 700, 2), (8, 48, 15, 1, 0), True),
    "300x3_clamped": (lambda: _shifted(300, 3, 2, 5), (50, 1000, 15, 0, 1), False),
    "16384x2": (lambda: _shifted(16384, 2, 2, 5), (8, 48, 15, 1, 1), True),
    "3x16384": (lambda: _shifted(3, 16384, 2), (8, 48, 15, 1, 0), False),
    "130_frames_5x3": (lambda: long_cases.frames("many_small"), (8, 48, 15, 1, 0), True),
    "146x1440_cyclic": (lambda: long_cases.frames("working"), (8, 48, 15, 1, 1), True),
}


@pytest.mark.parametrize("name", list(LONG))
def test_long_and_limit_shapes_equal_the_numpy_statement(ctx, name):
    make, opts, cyclic = LONG[name]
    top, bot = make()
    _check(ctx, top, bot, opts, cyclic, (None,), scratch=False)


def _raw_paths(ctx, t_top, t_bot, paths, P1=8, P2=48, flags=0, want_S=True, **kw):
    """sosvo_dense_stereo_paths as the library exports it -> (status, d16, S)."""
    import torch
    n, rows, cols = t_top.shape
    d16 = torch.zeros((n, rows, cols), dtype=torch.int16, device=ctx.device)
    S = torch.zeros((n, rows, cols, 64), dtype=torch.uint16, device=ctx.device) if want_S else None
    a = dict(top=ctypes.c_void_p(t_top.data_ptr()), bot=ctypes.c_void_p(t_bot.data_ptr()), n=n, rows=rows, cols=cols, d0=1, P1=P1, P2=P2,
             uniq=15, lr=1, flags=flags, paths=paths, out=ctypes.c_void_p(d16.data_ptr()))
    a.update(kw)
    rc = ctx._lib.sosvo_dense_stereo_paths(ctx._h, a["top"], a["bot"], a["n"], a["rows"], a["cols"], None, a["d0"], a["P1"], a["P2"],
                                           a["uniq"], a["lr"], a["flags"], a["paths"], a["out"],
                                           None if S is None else ctypes.c_void_p(S.data_ptr()))
    return rc, d16, S


def test_four_paths_through_the_new_entry_point_are_the_old_one(ctx):
    """paths = 4: the bytes and the launches of sosvo_dense_stereo; paths = 8: exactly the four diagonal launches more, after
    the right-to-left pass and before the select."""
    top, bot = _frames(70, 5)
    t, b = _dev(ctx, top), _dev(ctx, bot)
    names = {}
    for flags in (0, 1):
        from vo_single_camera_sos_amd._lib import DenseOptions
        ctx.profile_enable(True)
        want_d16, want_S = ctx.dense_stereo(t, b, None, options=DenseOptions(cyclic=bool(flags)), want_volume=True)
        ctx.synchronize()
        names["old"] = [name for name, _ in ctx.profile_read()]
        for paths in (4, 8):
            ctx.profile_enable(True)
            rc, d16, S = _raw_paths(ctx, t, b, paths, flags=flags)
            ctx.synchronize()
            names[paths] = [name for name, _ in ctx.profile_read()]
            assert rc == 0
            same = d16.cpu().numpy().tobytes() == want_d16.cpu().numpy().tobytes(), S.cpu().numpy().tobytes() == want_S.cpu().numpy().tobytes()
            assert same == ((True, True) if paths == 4 else (False, False))
        ctx.profile_enable(False)
        assert names[4] == names["old"] and len(names["old"]) >= 7 and not any("diag" in name for name in names[4])
        k = names[4].index("dense_path_kernel_rl") + 1
        assert names[8] == names[4][:k] + DIAG_NAMES + names[4][k:] and names[8][k + 4] == "dense_select_kernel"


def test_default_arguments_give_the_four_path_bytes(ctx):
    from vo_single_camera_sos_amd._lib import DenseOptions
    top, bot = _frames(12, 9)
    t, b, m = _dev(ctx, top), _dev(ctx, bot), _dev(ctx, _mask(12, 9))
    o = DenseOptions(min_disparity=0)
    plain, S = ctx.dense_stereo(t, b, m, options=o, want_volume=True)
    four, S4 = ctx.dense_stereo(t, b, m, options=o, want_volume=True, paths=4)
    ctx.synchronize()
    want_S = np.stack([refdense.aggregate(refdense.cost_volume(refdense.census(x), refdense.census(y), 0), 8, 48) for x, y in zip(top, bot)])
    assert np.array_equal(S.cpu().numpy(), want_S) and np.array_equal(S4.cpu().numpy(), want_S)
    assert plain.cpu().numpy().tobytes() == four.cpu().numpy().tobytes()
    assert np.array_equal(plain.cpu().numpy(), np.stack([refdense.select(s, 0, 15, 1, _mask(12, 9)) for s in want_S]))


def test_argument_refusals_launch_nothing(ctx):
    """Every refusal of sosvo_dense_stereo_paths returns SOSVO_ERR_ARG before any launch, under its own name; the Python layer
    raises ValueError before the call."""
    from vo_single_camera_sos_amd import _lib
    from vo_single_camera_sos_amd._lib import DenseOptions
    top, bot = _frames(12, 9)
    t, b = _dev(ctx, top), _dev(ctx, bot)
    ctx.profile_enable(True)
    bad = [(dict(rows=0), "rows / cols out of range (1..16384)"), (dict(cols=0), None), (dict(rows=16385), None), (dict(cols=16385), None),
           (dict(n=0), "n out of range (1..32767)"), (dict(n=32768), None),
           (dict(P1=49), "penalties out of range (0 <= P1 <= P2 <= 8191)"), (dict(P2=8192, P1=0, paths=4), None), (dict(P1=-1), None),
           (dict(uniq=-1), "uniqueness out of range (0..99)"), (dict(uniq=100), None),
           (dict(d0=-1), "min_disparity out of range (0..1024)"), (dict(d0=1025), None),
           (dict(flags=2), "unknown flag bits"), (dict(flags=-1), None),
           (dict(top=None), "null pointer"), (dict(bot=None), None), (dict(out=None), None),
           (dict(paths=0), "paths must be 4 or 8"), (dict(paths=5), None), (dict(paths=-8), None), (dict(paths=16), None), (dict(paths=12), None),
           (dict(P2=8128, P1=0), "eight paths need P2 <= 8127 (S stays 16 bits)"), (dict(P2=8191, P1=8191), None)]
    for kw, message in bad:
        rc, _, _ = _raw_paths(ctx, t, b, kw.pop("paths", 8), want_S=False, **kw)
        assert rc == -1, kw
        if message is not None:
            assert ctx._lib.sosvo_last_error(ctx._h).decode() == "sosvo_dense_stereo_paths: " + message, kw
    assert ctx.profile_read() == []
    assert _raw_paths(ctx, t, b, 4, P1=8191, P2=8191)[0] == 0 and _raw_paths(ctx, t, b, 8, P1=8127, P2=8127)[0] == 0
    assert _raw_paths(ctx, t, b, 8, P1=0, P2=0, lr=-5)[0] == 0
    ctx.synchronize()
    names = [name for name, _ in ctx.profile_read()]
    assert [name for name in names if "diag" in name] == DIAG_NAMES * 2 and len(names) > 8
    ctx.profile_enable(True)
    for kw in (dict(paths=0), dict(paths=6), dict(paths="8"), dict(paths=8.0), dict(paths=True), dict(paths=None),
               dict(paths=8, options=DenseOptions(P1=0, P2=8128)), dict(paths=8, options=dict(P2=8191))):
        with pytest.raises(ValueError):
            ctx.dense_stereo(t, b, **kw)
    assert ctx.profile_read() == []
    ctx.profile_enable(False)
    assert _lib.DENSE_MAX_P2_EIGHT_PATHS == 8127 and _lib.dense_paths(8, DenseOptions(P2=8127)) == 8 and _lib.dense_paths(4, DenseOptions(P2=8191)) == 4


def test_engine_equals_the_staged_calls_and_the_numpy_statement(ctx, rig):
    from vo_single_camera_sos_amd._lib import DenseOptions, SpeckleOptions
    from vo_single_camera_sos_amd.frontend import DeviceImageModel
    from vo_single_camera_sos_amd.pipeline import DenseOmniStereo, dense_mask
    model = DeviceImageModel(ctx, rig["gs"], (480, 640))
    cfg, o, sp = _rig_cfg(rig), DenseOptions(min_disparity=0, cyclic=True), SpeckleOptions(max_size=12, max_diff=16, cyclic=True)
    mask = dense_mask(ctx, model)
    gray = ctx.unwrap_median_gray(_dev(ctx, rig["omni"]), model.unwrap_table, 0)
    raw8 = ctx.dense_stereo(gray[:2].contiguous(), gray[2:].contiguous(), mask, options=o, paths=8)
    raw4 = ctx.dense_stereo(gray[:2].contiguous(), gray[2:].contiguous(), mask, options=o)
    ctx.synchronize()
    g, mask_h, raw8_h, raw4_h = gray.cpu().numpy(), mask.cpu().numpy(), raw8.cpu().numpy(), raw4.cpu().numpy()
    want8 = np.stack([refdense8.dense_stereo(g[k], g[2 + k], mask_h, min_disparity=0, cyclic=True, paths=8) for k in range(2)])
    assert np.array_equal(raw8_h, want8) and not np.array_equal(raw8_h, raw4_h)
    for speckle, want in ((None, want8), (sp, refspeckle.speckle(want8, 12, 16, cyclic=True))):
        eng = DenseOmniStereo(ctx, model, cfg, 2, options=o, speckle=speckle, paths=8)
        assert eng.paths == 8
        eng.load_frames(rig["omni"])
        ctx.profile_enable(True)
        d16, X = eng.step()
        ctx.synchronize()
        names = [name for name, _ in ctx.profile_read()]
        ctx.profile_enable(False)
        assert [name for name in names if "diag" in name] == DIAG_NAMES
        want_X = ctx.dense_triangulate(cfg.as_struct(), _dev(ctx, want), 1.0, 0.0)
        ctx.synchronize()
        assert np.array_equal(d16.cpu().numpy(), want), np.argwhere(d16.cpu().numpy() != want)[:5]
        assert np.array_equal(X.cpu().numpy(), want_X.cpu().numpy(), equal_nan=True)
    assert not np.array_equal(want, want8)
    for kw in (dict(), dict(paths=4)):               # four paths: the engine as it was, and no diagonal kernel runs
        eng = DenseOmniStereo(ctx, model, cfg, 2, options=o, **kw)
        assert eng.paths == 4
        eng.load_frames(rig["omni"])
        ctx.profile_enable(True)
        d16, _ = eng.step()
        ctx.synchronize()
        names = [name for name, _ in ctx.profile_read()]
        ctx.profile_enable(False)
        assert names and not any("diag" in name for name in names)
        assert d16.cpu().numpy().tobytes() == raw4_h.tobytes()
    for kw in (dict(paths=6), dict(paths=8, options=DenseOptions(P1=0, P2=8128))):
        with pytest.raises(ValueError):
            DenseOmniStereo(ctx, model, cfg, 2, **kw)


def test_host_mirror_gives_the_engines_numbers(ctx, rig):
    from vo_single_camera_sos_amd._lib import DenseOptions
    from vo_single_camera_sos_amd.frontend import DeviceImageModel
    from vo_single_camera_sos_amd.pipeline import DenseOmniStereo
    gs, o = rig["gs"], DenseOptions()
    maps = {}
    for paths in (4, 8):
        eng = DenseOmniStereo(ctx, DeviceImageModel(ctx, gs, (480, 640)), _rig_cfg(rig, 0.0, 0.0), 1, options=o, min_disparity=0.0,
                              paths=paths)
        eng.load_frames(rig["omni"][:1])
        d16, _ = eng.step()
        ctx.synchronize()
        maps[paths] = d16.cpu().numpy()[0]
    assert not np.array_equal(maps[4], maps[8])
    gs.__dict__.pop("_dense_engines", None)
    gs.set_current_omni_image(rig["omni"][0], generate_panoramas=True)
    dmap0, dimg0 = gs.get_depth_map_from_panoramas(method="sgbm", options=o)                    # as before the keyword existed
    assert np.array_equal(gs.disparity_d16, maps[4])
    dmap4, dimg4 = gs.get_depth_map_from_panoramas(method="sgbm", options=o, paths=4)
    assert np.array_equal(dmap4, dmap0) and np.array_equal(dimg4, dimg0) and len(gs._dense_engines) == 1
    full_dyn_prog = True                                                                         # the tuner's "Full DP" trackbar
    dmap, dimg = gs.get_depth_map_from_panoramas(method="sgbm", options=o, paths=8 if full_dyn_prog else 4)
    d16 = maps[8]
    assert np.array_equal(gs.disparity_d16, d16) and len(gs._dense_engines) == 2
    assert np.array_equal(dmap, np.where(d16 >= 0, d16 / 16.0, 0.0)) and np.array_equal(dmap == 0, d16 == -1)
    assert np.array_equal(dimg, np.where(d16 >= 0, np.clip((d16 / 16.0 - 1) * 255.0 / 63, 0, 255), 0).astype(np.uint8))
    with pytest.raises(ValueError):
        gs.get_depth_map_from_panoramas(method="sgbm", options=o, paths=2)
