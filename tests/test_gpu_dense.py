"""GPU: dense omnistereo.  The device reproduces tests/refdense.py -- census words, the aggregated
volume S and the disparity map d16 -- bit for bit at the smallest shapes where an index can go wrong; the dense triangulation
equals the sparse path's staged calls; the engine and the host mirror equal the staged calls.  array_equal throughout."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refdense  # noqa: E402

pytestmark = pytest.mark.gpu

# rows x cols: one row, one column, fewer rows than the window and than D, fewer columns than the window, D x D, and a shape
# of several blocks that is no multiple of anything
SHAPES = [(1, 70), (70, 1), (12, 9), (70, 5), (64, 64), (130, 33)]
# (P1, P2, uniqueness, lr_max, d0)
OPTION_SETS = [(8, 48, 15, 1, 0), (0, 0, 0, -1, 1), (50, 1000, 15, 0, 7), (8191, 8191, 99, 63, 0)]


def _texture(rng, rows, cols):
    """A lightly smoothed random texture, u8."""
    a = rng.integers(0, 256, (rows + 2, cols + 2)).astype(np.float64)
    a = (a[:-2, 1:-1] + a[2:, 1:-1] + a[1:-1, :-2] + a[1:-1, 2:] + 2 * a[1:-1, 1:-1]) / 6.0
    return a.astype(np.uint8)


def _frames(rows, cols):
    """n = 3 frames of different content -> top, bot [3, rows, cols]: two textures related by a shift of 5 rows plus noise, a
    constant image (all ties), a planted shift of 63 rows."""
    rng = np.random.default_rng(rows * 1000 + cols)
    tall = _texture(rng, rows + 63, cols)
    noisy = np.clip(tall[5:5 + rows].astype(np.int32) + rng.integers(-3, 4, (rows, cols)), 0, 255).astype(np.uint8)
    top = np.stack([tall[:rows], np.full((rows, cols), 77, np.uint8), tall[:rows]])
    bot = np.stack([noisy, np.full((rows, cols), 77, np.uint8), tall[63:63 + rows]])
    return np.ascontiguousarray(top), np.ascontiguousarray(bot)


def _mask(rows, cols):
    rng = np.random.default_rng(rows + 7 * cols)
    return (rng.random((rows, cols)) < 0.8).astype(np.uint8) * 255


_REF_S = {}


def _ref_S(shape, d0, P1, P2, cyclic):
    """refdense's S of the three frames, computed once per (shape, d0, P1, P2, cyclic)."""
    key = (shape, d0, P1, P2, cyclic)
    if key not in _REF_S:
        top, bot = _frames(*shape)
        _REF_S[key] = np.stack([refdense.aggregate(refdense.cost_volume(refdense.census(t, cyclic), refdense.census(b, cyclic), d0),
                                                   P1, P2) for t, b in zip(top, bot)])
    return _REF_S[key]


def _dev(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_census_equals_the_numpy_statement(ctx, shape):
    top, bot = _frames(*shape)
    gray = np.concatenate([top, bot])
    for cyclic in (False, True):
        got = ctx.census(_dev(ctx, gray), cyclic=cyclic)
        ctx.synchronize()
        got = got.cpu().numpy().view(np.uint64)
        want = refdense.census(gray, cyclic)
        assert np.array_equal(got, want), (cyclic, np.argwhere(got != want)[:5])
        assert (got >> np.uint64(62)).max() == 0


@pytest.mark.parametrize("opts", OPTION_SETS, ids=lambda o: "P%d_%d_u%d_lr%d_d%d" % o)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_volume_and_disparities_equal_the_numpy_statement(ctx, shape, opts):
    from vo_single_camera_sos_amd._lib import DenseOptions
    P1, P2, uniq, lr_max, d0 = opts
    top, bot = _frames(*shape)
    t_top, t_bot, mask = _dev(ctx, top), _dev(ctx, bot), _mask(*shape)
    for cyclic in (False, True):
        o = DenseOptions(min_disparity=d0, P1=P1, P2=P2, uniqueness=uniq, lr_max=lr_max, cyclic=cyclic)
        want_S = _ref_S(shape, d0, P1, P2, cyclic)
        for m in (None, mask):
            d16, S = ctx.dense_stereo(t_top, t_bot, None if m is None else _dev(ctx, m), options=o, want_volume=True)
            only = ctx.dense_stereo(t_top, t_bot, None if m is None else _dev(ctx, m), options=o)   # S in the scratch
            ctx.synchronize()
            S, d16 = S.cpu().numpy(), d16.cpu().numpy()
            assert np.array_equal(S, want_S), ("S", cyclic, np.argwhere(S != want_S)[:5])
            want = np.stack([refdense.select(s, d0, uniq, lr_max, m) for s in want_S])
            assert np.array_equal(d16, want), ("d16", cyclic, m is not None, np.argwhere(d16 != want)[:5])
            assert np.array_equal(only.cpu().numpy(), want)


def test_result_does_not_depend_on_the_scratch(ctx):
    top, bot = _frames(130, 33)
    t_top, t_bot, mask = _dev(ctx, top), _dev(ctx, bot), _dev(ctx, _mask(130, 33))
    got = []
    for byte in (None, 0xFF, 0x00):
        if byte is not None:
            ctx.debug_fill_scratch(byte)
        d16 = ctx.dense_stereo(t_top, t_bot, mask)
        ctx.synchronize()
        got.append(d16.cpu().numpy().tobytes())
    assert got[0] == got[1] == got[2]


@pytest.fixture(scope="module")
def rig():
    """The synthetic rig at Panorama(width=320) (33 rows), two rendered frames, the device model."""
    from vo_single_camera_sos_amd import synthetic
    from vo_single_camera_sos_amd.omnistereo.gum import synthetic_gums
    from vo_single_camera_sos_amd.omnistereo.panorama import Panorama
    gs = synthetic_gums()
    for m in (gs.top_model, gs.bot_model):
        m.panorama = Panorama(m, width=320)
    gs.make_annulus_masks((480, 640))
    pano = gs.top_model.panorama
    geo = (pano.cols, pano.rows, pano.pixel_size, pano.cyl_height_max)
    omni, _ = synthetic.make_frame_pairs(gs, 1, seed=7)
    return dict(gs=gs, geo=geo, omni=omni, F_top=gs.top_model.F[:3, 0], F_bot=gs.bot_model.F[:3, 0])


def _rig_cfg(rig, min_range=500.0, max_range=7000.0):
    from vo_single_camera_sos_amd.pipeline import RigConfig
    return RigConfig(rig["geo"], rig["geo"], rig["F_top"], rig["F_bot"], min_range, max_range)


def _staged_triangulation(ctx, cfg, d16, lo, hi):
    """The sparse path's stage calls on the valid pixels of d16 [n, rows, cols] (numpy) -> X [n, rows, cols, 3]."""
    X = np.full(d16.shape + (3,), np.nan)
    sel = (d16 >= 0) & (d16 >= lo) & ((d16 <= hi) if hi > 0 else True)
    idx = np.nonzero(sel)
    r, c, d = idx[1].astype(np.float64), idx[2].astype(np.float64), d16[idx].astype(np.float64)
    az1, el1, _ = ctx.pano_to_bearing(_dev(ctx, np.stack([c, r], axis=1)), *cfg.pano_top)
    az2, el2, _ = ctx.pano_to_bearing(_dev(ctx, np.stack([c, r - d / 16.0], axis=1)), *cfg.pano_bot)
    P = ctx.triangulate_midpoint(az1, el1, az2, el2, cfg.F_top, cfg.F_bot)
    ok = ctx.range_filter(P, cfg.min_range, cfg.max_range)
    ctx.synchronize()
    P, ok = P.cpu().numpy(), ok.cpu().numpy().astype(bool)
    P[~ok] = np.nan
    X[idx] = P
    return X


def test_dense_triangulation_equals_the_staged_calls_and_the_oracle(ctx, rig):
    cols, rows = rig["geo"][0], rig["geo"][1]
    rng = np.random.default_rng(5)
    d16 = rng.integers(-1, 64 * 16, (2, rows, cols)).astype(np.int16)    # bottom rows above the panorama included
    d16[0, :4] = rng.integers(-1, 40, (4, cols))
    for min_d, max_d, lo, hi in ((1.0, 0.0, 16, 0), (0.0, 0.0, 0, 0), (2.5, 30.25, 40, 484)):
        cfg = _rig_cfg(rig)
        got = ctx.dense_triangulate(cfg.as_struct(), _dev(ctx, d16), min_d, max_d)
        ctx.synchronize()
        got = got.cpu().numpy()
        want = _staged_triangulation(ctx, cfg, d16, lo, hi)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(got, want, equal_nan=True)
        assert np.array_equal(got, refdense.triangulate(cfg, d16, lo, hi), equal_nan=True)
        finite = ~np.isnan(got[..., 0])
        assert finite.any() and (~finite).any()
        assert np.isnan(got[d16 < lo]).all()
    open_cfg = _rig_cfg(rig, 0.0, 0.0)       # no range filter: more points, the same bits where both have one
    more = ctx.dense_triangulate(open_cfg.as_struct(), _dev(ctx, d16), 1.0, 0.0)
    ctx.synchronize()
    assert np.array_equal(more.cpu().numpy(), _staged_triangulation(ctx, open_cfg, d16, 16, 0), equal_nan=True)


def test_engine_equals_the_staged_calls(ctx, rig):
    from vo_single_camera_sos_amd._lib import DenseOptions
    from vo_single_camera_sos_amd.frontend import DeviceImageModel
    from vo_single_camera_sos_amd.pipeline import DenseOmniStereo, dense_mask
    model = DeviceImageModel(ctx, rig["gs"], (480, 640))
    cfg, o = _rig_cfg(rig), DenseOptions(min_disparity=0)
    for ksize in (0, 5):
        eng = DenseOmniStereo(ctx, model, cfg, 2, median_win_size=ksize, options=o)
        eng.load_frames(rig["omni"])
        d16, X = eng.step()
        depth = eng.depth()
        gray = ctx.unwrap_median_gray(_dev(ctx, rig["omni"]), model.unwrap_table, ksize)
        mask = dense_mask(ctx, model)
        want_d16 = ctx.dense_stereo(gray[:2].contiguous(), gray[2:].contiguous(), mask, options=o)
        want_X = ctx.dense_triangulate(cfg.as_struct(), want_d16, 1.0, 0.0)
        ctx.synchronize()
        d16, X, mask_h = d16.cpu().numpy(), X.cpu().numpy(), mask.cpu().numpy()
        assert np.array_equal(d16, want_d16.cpu().numpy()) and np.array_equal(X, want_X.cpu().numpy(), equal_nan=True)
        assert d16.shape == (2, 33, 320) and 0 < mask_h.mean() < 1 and (d16[:, mask_h == 0] == -1).all()
        assert (d16 >= 0).mean() > 0.5 and not np.array_equal(d16[0], d16[1])
        g = gray.cpu().numpy()        # ... and the whole engine equals the numpy statement on the device's gray panoramas
        assert np.array_equal(d16[0], refdense.dense_stereo(g[0], g[2], mask_h, min_disparity=0))
        with np.errstate(invalid="ignore"):
            want_depth = np.linalg.norm(X - np.asarray(cfg.F_top), axis=-1).astype(np.float32)
        assert np.array_equal(depth.cpu().numpy(), want_depth, equal_nan=True)


def test_host_mirror_gives_the_engines_numbers(ctx, rig, tmp_path):
    from vo_single_camera_sos_amd._lib import DenseOptions
    from vo_single_camera_sos_amd.frontend import DeviceImageModel
    from vo_single_camera_sos_amd.pipeline import DenseOmniStereo
    gs, o = rig["gs"], DenseOptions()
    eng = DenseOmniStereo(ctx, DeviceImageModel(ctx, gs, (480, 640)), _rig_cfg(rig, 0.0, 0.0), 1, options=o, min_disparity=0.0)
    eng.load_frames(rig["omni"][:1])
    d16, X = eng.step()
    ctx.synchronize()
    d16, X = d16.cpu().numpy()[0], X.cpu().numpy()[0]
    gs.set_current_omni_image(rig["omni"][0], generate_panoramas=True)
    dmap, dimg = gs.get_depth_map_from_panoramas(method="sgbm", show=True, tune_live=True, options=o)
    assert dmap.dtype == np.float64 and dimg.dtype == np.uint8 and dmap.shape == dimg.shape == d16.shape
    assert np.array_equal(dmap, np.where(d16 >= 0, d16 / 16.0, 0.0)) and np.array_equal(dmap == 0, d16 == -1)
    assert np.array_equal(dimg, np.where(d16 >= 0, np.clip((d16 / 16.0 - 1) * 255.0 / 63, 0, 255), 0).astype(np.uint8))
    ref = np.transpose(np.indices(dmap.shape[::-1]), (1, 2, 0))
    top, bot, disp = gs.resolve_pano_correspondences_from_disparity_map(ref, min_disparity=2, max_disparity=40)
    assert top.shape == bot.shape == (1, len(disp), 2) and len(disp) > 100
    assert np.array_equal(disp, dmap[top[0, :, 1], top[0, :, 0]]) and disp.min() >= 2 and disp.max() <= 40
    assert np.array_equal(bot[0, :, 0], top[0, :, 0]) and np.array_equal(bot[0, :, 1], top[0, :, 1] - disp)
    (xyz, rgb), clouds = gs.triangulate_from_depth_map(min_disparity=2, max_disparity=40, export_to_pcd=True,
                                                       cloud_path=str(tmp_path), cloud_index=3)
    keep = ~np.isnan(X[top[0, :, 1], top[0, :, 0], 0])
    u, v = top[0, keep, 0], top[0, keep, 1]
    assert xyz.shape == (1, len(u), 4) and rgb.shape == (len(u), 3) and clouds == (None, None)
    assert np.array_equal(xyz[0, :, :3], X[v, u]) and (xyz[0, :, 3] == 1).all() and not np.isnan(xyz).any()
    assert np.array_equal(rgb, gs.top_model.panorama.panoramic_img[v, u, ::-1].astype(np.float32))
    lines = open(os.path.join(str(tmp_path), "XYZ-3.pcd")).read().splitlines()
    assert "POINTS %d" % len(u) in lines and len(lines) == 11 + len(u)


def test_argument_refusals_launch_nothing(ctx, rig):
    """Every refusal returns SOSVO_ERR_ARG before any launch: the profile records no kernel."""
    import torch
    from vo_single_camera_sos_amd import _lib
    lib, h = ctx._lib, ctx._h
    top, bot = _frames(12, 9)
    t, b = _dev(ctx, top), _dev(ctx, bot)
    d16 = torch.zeros((3, 12, 9), dtype=torch.int16, device=ctx.device)
    cen = torch.zeros((3, 12, 9), dtype=torch.int64, device=ctx.device)
    X = torch.zeros((3, 12, 9, 3), dtype=torch.float64, device=ctx.device)
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    ctx.profile_enable(True)

    def stereo(top=p(t), bot=p(b), n=3, rows=12, cols=9, d0=1, P1=8, P2=48, uniq=15, lr=1, flags=0, out=p(d16)):
        return lib.sosvo_dense_stereo(h, top, bot, n, rows, cols, None, d0, P1, P2, uniq, lr, flags, out, None)
    bad = [dict(rows=0), dict(cols=0), dict(rows=16385), dict(cols=16385), dict(n=0), dict(P1=49), dict(P2=8192, P1=0), dict(P1=-1),
           dict(uniq=-1), dict(uniq=100), dict(d0=-1), dict(d0=1025), dict(flags=2), dict(flags=-1), dict(top=None), dict(bot=None),
           dict(out=None)]
    for kw in bad:
        assert stereo(**kw) == -1, kw
    for args in ((None, 3, 12, 9, 0, p(cen)), (p(t), 3, 12, 9, 0, None), (p(t), 0, 12, 9, 0, p(cen)), (p(t), 3, 0, 9, 0, p(cen)),
                 (p(t), 3, 12, 16385, 0, p(cen)), (p(t), 3, 12, 9, 2, p(cen))):
        assert lib.sosvo_census_9x7(h, *args) == -1, args
    good = _rig_cfg(rig).as_struct()
    skew = _rig_cfg(rig).as_struct()
    skew.pano_bot[1] += 1
    rp = lambda r: ctypes.cast(ctypes.pointer(r), ctypes.c_void_p)   # noqa: E731
    for args in ((None, p(d16), 3, 12, 9, 16, 0, p(X)), (rp(good), None, 3, 12, 9, 16, 0, p(X)), (rp(good), p(d16), 3, 12, 9, 16, 0, None),
                 (rp(good), p(d16), 0, 12, 9, 16, 0, p(X)), (rp(good), p(d16), 3, 0, 9, 16, 0, p(X)),
                 (rp(good), p(d16), 3, 12, 16385, 16, 0, p(X)), (rp(skew), p(d16), 3, 12, 9, 16, 0, p(X))):
        assert lib.sosvo_dense_triangulate(h, *args) == -1, args
    assert ctx.profile_read() == []
    assert stereo() == 0 and stereo(P1=0, P2=0, lr=-5) == 0     # (the reference's tuner: no smoothness)
    ctx.synchronize()
    assert len(ctx.profile_read()) > 0
    ctx.profile_enable(False)
    with pytest.raises(_lib.SosvoError):
        ctx.dense_stereo(t, b[:2].contiguous())
