"""GPU: the WLS disparity filter.  The device reproduces tests/refwls.py -- the confidence, the final
numerator and denominator planes and the filtered map -- bit for bit, three frames of different content per call; the engine
and the host mirror equal the staged calls.  array_equal throughout, doubles through .view(int64)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refdense  # noqa: E402
import refwls  # noqa: E402
from test_dense_reference import OPTS, _texture  # noqa: E402
from test_gpu_speckle import _rig_cfg, rig  # noqa: E402,F401

pytestmark = pytest.mark.gpu

# 65 x 200: one row past a 64-row tile, several column tiles; 130 x 33: three row tiles, the last of two rows
SHAPES = [(1, 1), (1, 70), (70, 1), (2, 2), (3, 3), (12, 9), (70, 5), (64, 64), (65, 200), (130, 33)]
IDS = ["%dx%d" % s for s in SHAPES]
_FRAMES = {}


def _stereo_frame(rng, rows, cols):
    """A refdense map of two textures (the left half shifted by 3 rows, the right half by 9) and its own top view."""
    img = _texture(rng, rows + 9, cols)
    top, bot = img[:rows], img[3:3 + rows].copy()
    bot[:, cols // 2:] = img[9:9 + rows, cols // 2:]
    return refdense.dense_stereo(top, bot, None, min_disparity=1, **OPTS), top


def _striped_frame(rng, rows, cols):
    """A constant map with 30 % holes under the striped guide (affinity exp(-255 / sigma) between any two columns)."""
    d = np.where(rng.random((rows, cols)) < 0.3, -1, 333).astype(np.int16)
    return d, np.broadcast_to(((np.arange(cols) & 1) * 255).astype(np.uint8), (rows, cols)).copy()


def _random_frame(rng, rows, cols):
    d = rng.integers(0, 1024, (rows, cols)).astype(np.int16)
    d[rng.random((rows, cols)) < 0.1] = -1
    return d, rng.integers(0, 256, (rows, cols)).astype(np.uint8)


def _frames(shape, kinds=(_stereo_frame, _striped_frame, _random_frame)):
    """-> (d16, guide, conf, mask) of the shape, made once: conf is the confidence stage's, but random for a _random_frame
    (the confidence of a random map is 0 nearly everywhere)."""
    key = (shape, kinds)
    if key not in _FRAMES:
        rows, cols = shape
        rng = np.random.default_rng(1000 * rows + cols)
        d, g = (np.stack(x) for x in zip(*[kind(rng, rows, cols) for kind in kinds]))
        conf = np.stack([rng.integers(0, 256, (rows, cols)).astype(np.uint8) if kind is _random_frame else refwls.confidence(f)
                         for kind, f in zip(kinds, d)])
        mask = (rng.random((rows, cols)) < 0.8).astype(np.uint8)
        _FRAMES[key] = (d, g, conf, mask)
    return _FRAMES[key]


def _dev(ctx, a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _reference(d, g, conf, mask, o):
    res = [refwls.wls(d[k], g[k], None if conf is None else conf[k], mask, o.lam, o.weight_table(), o.iters, o.min_weight, o.cyclic)
           for k in range(d.shape[0])]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def _filter(ctx, d, g, conf, mask, o, in_place=False):
    from vo_single_camera_sos_amd import dense_filter
    t = _dev(ctx, d)
    out, planes = dense_filter.dense_wls(ctx, t, _dev(ctx, g), options=o, conf=_dev(ctx, conf), mask=_dev(ctx, mask),
                                         out=t if in_place else None, want_planes=True)
    ctx.synchronize()
    assert (out is t) == in_place
    if not in_place:
        assert np.array_equal(t.cpu().numpy(), d), "the input was written"
    return out.cpu().numpy(), planes.cpu().numpy()


def _same(got, want, where):
    (out, planes), (want_out, want_planes) = got, want
    for name, k in (("numerator", 0), ("denominator", 1)):
        a, b = planes[:, k].view(np.int64), np.ascontiguousarray(want_planes[:, k]).view(np.int64)
        assert np.array_equal(a, b), (name,) + where + (np.argwhere(a != b)[:5].tolist(),)
    assert np.array_equal(out, want_out), ("map",) + where + (np.argwhere(out != want_out)[:5].tolist(),)


def _configs():
    """(options, with conf, with mask): clamped and cyclic, iters 1, 3, 8, lambda 0, 50, 8000, sigma 1 and 8."""
    from vo_single_camera_sos_amd._lib import WlsOptions
    return [(WlsOptions(), True, False), (WlsOptions(cyclic=True), True, True),
            (WlsOptions(lam=50.0, sigma=8.0, iters=1), False, True), (WlsOptions(lam=50.0, sigma=8.0, iters=8, cyclic=True), False, False),
            (WlsOptions(lam=0.0, cyclic=True), True, False), (WlsOptions(sigma=8.0, iters=8, min_weight=0.01), True, True),
            (WlsOptions(lam=0.0, iters=1), False, False)]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_confidence_equals_the_numpy_statement(ctx, shape):
    from vo_single_camera_sos_amd import dense_filter
    d = _frames(shape)[0]
    t = _dev(ctx, d)
    for cyclic in (False, True):
        for radius, roll_ppm in ((3, 1000), (0, 1000), (1, 1000000), (7, 40), (7, 0)):
            got = dense_filter.dense_confidence(ctx, t, options=dict(radius=radius, roll_ppm=roll_ppm, cyclic=cyclic))
            ctx.synchronize()
            want = np.stack([refwls.confidence(f, radius, roll_ppm, cyclic) for f in d])
            assert np.array_equal(got.cpu().numpy(), want), (cyclic, radius, roll_ppm)
    assert np.array_equal(t.cpu().numpy(), d)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_planes_and_map_equal_the_numpy_statement(ctx, shape):
    d, g, conf, mask = _frames(shape)
    for i, (o, with_conf, with_mask) in enumerate(_configs()):
        c, m = conf if with_conf else None, mask if with_mask else None
        want = _reference(d, g, c, m, o)
        for in_place in (False, True):
            _same(_filter(ctx, d, g, c, m, o, in_place), want, (o, with_conf, with_mask, in_place))
        if o.lam == 0:       # the filter returns d16 wherever w > 0
            w = (d >= 0) & ((conf > 0) if with_conf else True) & ((mask != 0) if with_mask else True)
            assert np.array_equal(want[0][w], d[w]) and (want[0][~w] == -1).all()


@pytest.mark.parametrize("shape", [(12, 9), (65, 200)], ids=lambda s: "%dx%d" % s)
def test_the_scratch_changes_nothing(ctx, shape):
    from vo_single_camera_sos_amd._lib import WlsOptions
    d, g, conf, mask = _frames(shape)
    for o in (WlsOptions(cyclic=True), WlsOptions(lam=50.0, sigma=8.0, iters=1)):
        want = _reference(d, g, conf, mask, o)
        filled = []
        for byte in (0xFF, 0x00):
            ctx.debug_fill_scratch(byte)
            got = _filter(ctx, d, g, conf, mask, o)
            _same(got, want, (o, byte))
            filled.append(got[0].tobytes() + got[1].tobytes())
        assert filled[0] == filled[1]


@pytest.mark.parametrize("cyclic", (False, True), ids=("clamped", "cyclic"))
@pytest.mark.parametrize("shape", [(3, 16384), (4096, 2)], ids=lambda s: "%dx%d" % s)
def test_one_long_axis_each_way(ctx, shape, cyclic):
    """The limits' rows and columns as one long line each: 1024 column tiles, 64 row tiles.  Two frames, two iterations."""
    from vo_single_camera_sos_amd import dense_filter
    from vo_single_camera_sos_amd._lib import WlsOptions
    d, g, conf, mask = _frames(shape, (_striped_frame, _random_frame))
    o = WlsOptions(lam=8000.0, sigma=8.0, iters=2, cyclic=cyclic)
    _same(_filter(ctx, d, g, conf, mask, o), _reference(d, g, conf, mask, o), (o,))
    got = dense_filter.dense_confidence(ctx, _dev(ctx, d), options=o)
    ctx.synchronize()
    assert np.array_equal(got.cpu().numpy(), np.stack([refwls.confidence(f, o.radius, o.roll_ppm, cyclic) for f in d]))


def test_130_frames_of_5x3(ctx):
    from vo_single_camera_sos_amd import dense_filter
    from vo_single_camera_sos_amd._lib import WlsOptions
    d, g, conf, mask = _frames((5, 3), (_random_frame,) * 130)
    for o in (WlsOptions(lam=50.0, sigma=8.0, cyclic=True), WlsOptions(lam=50.0, sigma=8.0)):
        _same(_filter(ctx, d, g, conf, mask, o, in_place=True), _reference(d, g, conf, mask, o), (o,))
        got = dense_filter.dense_confidence(ctx, _dev(ctx, d), options=o)
        ctx.synchronize()
        assert np.array_equal(got.cpu().numpy(), np.stack([refwls.confidence(f, o.radius, o.roll_ppm, o.cyclic) for f in d]))


def test_argument_refusals_launch_nothing(ctx):
    """Every refusal of the two entry points returns SOSVO_ERR_ARG before any launch, with the function's own name in front of
    the message: the profile records no kernel.  The Python refusals happen before any call."""
    import torch
    from vo_single_camera_sos_amd import _lib, dense_filter
    lib, h = dense_filter.load(), ctx._h
    assert lib is ctx._lib
    d, g, conf, mask = (_dev(ctx, a) for a in _frames((12, 9)))
    out = torch.zeros((3, 12, 9), dtype=torch.int16, device=ctx.device)
    conf_out = torch.zeros((3, 12, 9), dtype=torch.uint8, device=ctx.device)
    planes = torch.zeros((3, 2, 12, 9), dtype=torch.float64, device=ctx.device)
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    table = (ctypes.c_double * 256)(*_lib.WlsOptions().weight_table())

    def table_with(k, v):
        t = (ctypes.c_double * 256)(*table)
        t[k] = v
        return t
    nan, inf = float("nan"), float("inf")
    ctx.profile_enable(True)

    def confidence(src=p(d), n=3, rows=12, cols=9, radius=3, roll_ppm=1000, flags=0, dst=p(conf_out)):
        return lib.sosvo_dense_confidence(h, src, n, rows, cols, radius, roll_ppm, flags, dst)

    def wls(src=p(d), guide=p(g), c=p(conf), m=p(mask), n=3, rows=12, cols=9, lam=8000.0, weights=table, iters=3, min_weight=2.0 ** -20,
            flags=0, dst=p(out), pl=p(planes)):
        return lib.sosvo_dense_wls(h, src, guide, c, m, n, rows, cols, lam, weights, iters, min_weight, flags, dst, pl)
    sizes = [dict(rows=0), dict(cols=0), dict(rows=16385), dict(cols=16385), dict(rows=-1), dict(n=0), dict(n=-3), dict(n=32768),
             dict(flags=2), dict(flags=3), dict(flags=-1), dict(src=None), dict(dst=None)]
    for kw in sizes + [dict(radius=-1), dict(radius=8), dict(roll_ppm=-1), dict(roll_ppm=1000001)]:
        assert confidence(**kw) == -1, kw
        assert lib.sosvo_last_error(h).startswith(b"sosvo_dense_confidence: "), kw
    for kw in sizes + [dict(guide=None), dict(weights=None), dict(lam=-1.0), dict(lam=1000000.5), dict(lam=nan), dict(lam=inf),
                       dict(iters=0), dict(iters=9), dict(iters=-1), dict(min_weight=0.0), dict(min_weight=-1.0), dict(min_weight=nan),
                       dict(min_weight=inf), dict(weights=table_with(0, nan)), dict(weights=table_with(255, inf)),
                       dict(weights=table_with(17, -0.5)), dict(weights=table_with(100, 1.5))]:
        assert wls(**kw) == -1, kw
        assert lib.sosvo_last_error(h).startswith(b"sosvo_dense_wls: "), kw
    assert ctx.profile_read() == []
    for bad in (lambda: dense_filter.dense_wls(ctx, d, g, options=None), lambda: dense_filter.dense_confidence(ctx, d, options=None),
                lambda: dense_filter.dense_wls(ctx, d, g, options=dict(sigma=0.0))):
        with pytest.raises(ValueError):
            bad()
    o = _lib.WlsOptions()
    for bad in (lambda: dense_filter.dense_wls(ctx, d, g, options=o, out=out[:2]), lambda: dense_filter.dense_wls(ctx, d.to(torch.int32), g, options=o),
                lambda: dense_filter.dense_wls(ctx, d, g[:, :, :8], options=o), lambda: dense_filter.dense_wls(ctx, d, g.to(torch.int16), options=o),
                lambda: dense_filter.dense_wls(ctx, d, g, options=o, conf=conf[:1]), lambda: dense_filter.dense_wls(ctx, d, g, options=o, mask=mask[:5]),
                lambda: dense_filter.dense_wls(ctx, d.cpu(), g, options=o), lambda: dense_filter.dense_wls(ctx, d, g.cpu().numpy(), options=o),
                lambda: dense_filter.dense_confidence(ctx, d.to(torch.int32), options=o), lambda: dense_filter.dense_confidence(ctx, d[0], options=o)):
        with pytest.raises(_lib.SosvoError):
            bad()
    assert ctx.profile_read() == []
    assert confidence() == 0 and confidence(radius=0, roll_ppm=0, flags=1) == 0 and confidence(radius=7, roll_ppm=1000000) == 0
    assert wls() == 0 and wls(c=None, m=None, pl=None, lam=0.0, iters=1) == 0 and wls(lam=1e6, iters=8, flags=1, min_weight=1e300) == 0
    ctx.synchronize()
    names = [name for name, _ in ctx.profile_read()]
    ctx.profile_enable(False)
    # (init, final and four solve kernels per iteration; five in the cyclic form)
    assert len(names) == 3 + (2 + 4 * 3) + (2 + 4 * 1) + (2 + 5 * 8) and all(name.startswith("wls_") for name in names)


def test_engine_equals_the_staged_calls_and_none_changes_nothing(ctx, rig):   # noqa: F811
    from vo_single_camera_sos_amd import dense_filter
    from vo_single_camera_sos_amd._lib import DenseOptions, SpeckleOptions, WlsOptions
    from vo_single_camera_sos_amd.frontend import DeviceImageModel
    from vo_single_camera_sos_amd.pipeline import DenseOmniStereo, dense_mask
    model = DeviceImageModel(ctx, rig["gs"], (480, 640))
    cfg, o, sp = _rig_cfg(rig), DenseOptions(min_disparity=0), SpeckleOptions(max_size=12, max_diff=16, cyclic=True)
    w = WlsOptions(cyclic=True)
    mask = dense_mask(ctx, model)
    gray = ctx.unwrap_median_gray(_dev(ctx, rig["omni"]), model.unwrap_table, 0)
    top = gray[:2].contiguous()
    raw = ctx.dense_speckle(ctx.dense_stereo(top, gray[2:].contiguous(), mask, options=o), options=sp)
    conf = dense_filter.dense_confidence(ctx, raw, options=w)
    want_d16 = dense_filter.dense_wls(ctx, raw, top, options=w, conf=conf, mask=mask)
    want_X = ctx.dense_triangulate(cfg.as_struct(), want_d16, 1.0, 0.0)
    raw_X = ctx.dense_triangulate(cfg.as_struct(), raw, 1.0, 0.0)
    ctx.synchronize()
    raw_h, want_h, top_h, mask_h = raw.cpu().numpy(), want_d16.cpu().numpy(), top.cpu().numpy(), mask.cpu().numpy()
    conf_h = np.stack([refwls.confidence(f, w.radius, w.roll_ppm, True) for f in raw_h])
    assert np.array_equal(conf.cpu().numpy(), conf_h)
    assert np.array_equal(want_h, _reference(raw_h, top_h, conf_h, mask_h, w)[0])
    inside = np.broadcast_to(mask_h != 0, raw_h.shape)
    filled = int(((raw_h < 0) & (want_h >= 0)).sum())
    assert 0 < filled and (want_h[inside] >= 0).mean() > (raw_h[inside] >= 0).mean() and (want_h[~inside] == -1).all()

    for wls in (w, dict(cyclic=True)):
        eng = DenseOmniStereo(ctx, model, cfg, 2, options=o, speckle=sp, wls=wls)
        assert eng.wls == w
        eng.load_frames(rig["omni"])
        ctx.profile_enable(True)
        d16, X = eng.step()
        depth = eng.depth()
        ctx.synchronize()
        names = [name for name, _ in ctx.profile_read()]
        ctx.profile_enable(False)
        assert sum(name.startswith("wls_") for name in names) == 1 + 2 + 5 * 3
        assert d16 is eng.d16 and np.array_equal(d16.cpu().numpy(), want_h)
        assert np.array_equal(X.cpu().numpy(), want_X.cpu().numpy(), equal_nan=True)
        assert np.isnan(X.cpu().numpy()[want_h < 0]).all()
        with np.errstate(invalid="ignore"):
            want_depth = np.linalg.norm(X.cpu().numpy() - np.asarray(cfg.F_top), axis=-1).astype(np.float32)
        assert np.array_equal(depth.cpu().numpy(), want_depth, equal_nan=True)

    runs = []
    for kw in (dict(), dict(wls=None)):          # off: the engine as it was, and no kernel of the filter runs
        eng = DenseOmniStereo(ctx, model, cfg, 2, options=o, speckle=sp, **kw)
        assert eng.wls is None
        eng.load_frames(rig["omni"])
        ctx.profile_enable(True)
        d16, X = eng.step()
        ctx.synchronize()
        names = [name for name, _ in ctx.profile_read()]
        ctx.profile_enable(False)
        assert names and not any("wls" in name for name in names)
        assert d16.cpu().numpy().tobytes() == raw_h.tobytes()
        assert np.array_equal(X.cpu().numpy(), raw_X.cpu().numpy(), equal_nan=True)
        runs.append((names, d16.cpu().numpy().tobytes(), X.cpu().numpy().tobytes()))
    assert runs[0] == runs[1]
    with pytest.raises(ValueError):
        DenseOmniStereo(ctx, model, cfg, 2, options=o, wls=dict(lamda=3))
    with pytest.raises(ValueError):
        DenseOmniStereo(ctx, model, cfg, 2, options=o, wls=dict(sigma=-1.0))


def test_host_mirror_with_and_without_the_filter(ctx, rig):   # noqa: F811
    from vo_single_camera_sos_amd._lib import DenseOptions, WlsOptions
    from vo_single_camera_sos_amd.frontend import DeviceImageModel
    from vo_single_camera_sos_amd.pipeline import DenseOmniStereo
    gs, o, w = rig["gs"], DenseOptions(), WlsOptions.from_tuner(True, 8000, 100)
    assert w == WlsOptions()
    maps = {}
    for key, wls in (("off", None), ("on", w)):
        eng = DenseOmniStereo(ctx, DeviceImageModel(ctx, gs, (480, 640)), _rig_cfg(rig, 0.0, 0.0), 1, options=o, min_disparity=0.0, wls=wls)
        eng.load_frames(rig["omni"][:1])
        d16, _ = eng.step()
        ctx.synchronize()
        maps[key] = d16.cpu().numpy()[0]
    assert not np.array_equal(maps["off"], maps["on"])
    gs.__dict__.pop("_dense_engines", None)
    gs.set_current_omni_image(rig["omni"][0], generate_panoramas=True)
    dmap0, dimg0 = gs.get_depth_map_from_panoramas(method="sgbm", options=o)                    # as before the keyword existed
    assert np.array_equal(gs.disparity_d16, maps["off"])
    dmap_none, dimg_none = gs.get_depth_map_from_panoramas(method="sgbm", options=o, wls=None)
    assert np.array_equal(dmap_none, dmap0) and np.array_equal(dimg_none, dimg0) and len(gs._dense_engines) == 1
    assert np.array_equal(dimg0, np.where(maps["off"] >= 0, np.clip((maps["off"] / 16.0 - 1) * 255.0 / 63, 0, 255), 0).astype(np.uint8))
    for wls in (w, dict()):
        dmap, dimg = gs.get_depth_map_from_panoramas(method="sgbm", options=o, wls=wls)
        d16 = maps["on"]
        assert np.array_equal(gs.disparity_d16, d16) and len(gs._dense_engines) == 2
        assert np.array_equal(dmap, np.where(d16 >= 0, d16 / 16.0, 0.0))
        assert np.array_equal(dimg, np.where(d16 >= 0, np.clip((d16 / 16.0 + 1) * 255.0 / 65, 0, 255), 0).astype(np.uint8))   # from -1
        assert np.array_equal(dmap, gs.disparity_map) and np.array_equal(dimg, gs.disparity_img)
    (xyz, _), _ = gs.triangulate_from_depth_map(min_disparity=1)
    gs.get_depth_map_from_panoramas(method="sgbm", options=o)
    (xyz0, _), _ = gs.triangulate_from_depth_map(min_disparity=1)
    assert xyz.shape[1] > xyz0.shape[1] > 0          # the filled holes are points of the cloud now
