"""GPU: the speckle filter of the dense disparity map.  The device reproduces tests/refspeckle.py -- the
filtered map and the labels -- bit for bit on the maps of tests/speckle_cases.py, n = 3 frames of different content per call;
the engine and the host mirror equal the staged calls.  array_equal throughout."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refspeckle  # noqa: E402
import speckle_cases  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = ["%dx%d" % s for s in speckle_cases.SHAPES]
_LABELS = {}


def _ref_labels(shape, batch, max_diff, cyclic):
    """refspeckle's labels [3, rows, cols] of one batch of the shape, computed once per (max_diff, cyclic)."""
    key = (shape, batch, max_diff, cyclic)
    if key not in _LABELS:
        _LABELS[key] = np.stack([refspeckle.labels_of(f, max_diff, cyclic) for f in speckle_cases.batches(*shape)[batch][1]])
    return _LABELS[key]


def _ref_map(d, lab, max_size):
    """The threshold of refspeckle.speckle on labels already known."""
    out = d.copy()
    for k in range(d.shape[0]):
        valid = lab[k] != refspeckle.NONE
        size = np.bincount(lab[k][valid].astype(np.int64), minlength=lab[k].size)
        drop = np.zeros(lab[k].shape, bool)
        drop[valid] = size[lab[k][valid].astype(np.int64)] <= max_size
        out[k][drop] = -1
    return out


def _dev(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _run(ctx, t, max_size, max_diff, cyclic, **kw):
    from vo_single_camera_sos_amd._lib import SpeckleOptions
    res = ctx.dense_speckle(t, options=SpeckleOptions(max_size, max_diff, cyclic), **kw)
    ctx.synchronize()
    return [r.cpu().numpy() for r in res] if isinstance(res, tuple) else res.cpu().numpy()


@pytest.mark.parametrize("shape", speckle_cases.SHAPES, ids=IDS)
def test_map_and_labels_equal_the_numpy_statement(ctx, shape):
    rows, cols = shape
    for b, (names, d) in enumerate(speckle_cases.batches(*shape)):
        t = _dev(ctx, d)
        for cyclic in (False, True):
            for max_diff in (0, 15, 16, 32767):
                want_lab = _ref_labels(shape, b, max_diff, cyclic)
                # a component's exact size (dropped) and one less (kept): the largest component of the batch's first frame
                counts = np.unique(want_lab[0][want_lab[0] != refspeckle.NONE], return_counts=True)[1]
                exact = int(counts.max()) if len(counts) else 2
                sizes = (0, 1, exact, exact - 1, rows * cols, (1 << 31) - 1) if max_diff == 16 else (1, 5)
                for max_size in sizes:
                    got, lab = _run(ctx, t, max_size, max_diff, cyclic, want_labels=True)
                    where = (names, cyclic, max_diff, max_size)
                    assert np.array_equal(lab, want_lab), ("labels",) + where + (np.argwhere(lab != want_lab)[:5].tolist(),)
                    want = _ref_map(d, want_lab, max_size)
                    assert np.array_equal(got, want), ("map",) + where + (np.argwhere(got != want)[:5].tolist(),)
                    if max_size == 0:
                        assert np.array_equal(got, d)
                    if max_size >= rows * cols:
                        assert (got < 0).all() and np.array_equal(got[d < 0], d[d < 0])
                    if max_size in (exact, exact - 1) and len(counts):
                        big = want_lab[0] == np.unique(want_lab[0][want_lab[0] != refspeckle.NONE])[counts.argmax()]
                        assert (got[0][big] == -1).all() if max_size == exact else np.array_equal(got[0][big], d[0][big])


def test_the_threshold_helper_is_refspeckles(ctx):
    """_ref_map on refspeckle's labels is refspeckle.speckle (the parity test shares the labels among its max_size values)."""
    names, d = speckle_cases.batches(12, 9)[0]
    for max_size in (0, 1, 7, 108):
        want, lab = refspeckle.speckle(d, max_size, 16, True, want_labels=True)
        assert np.array_equal(_ref_map(d, lab, max_size), want)


@pytest.mark.parametrize("shape", [(12, 9), (65, 257)], ids=lambda s: "%dx%d" % s)
def test_in_place_labels_or_not_and_the_scratch_change_nothing(ctx, shape):
    for names, d in speckle_cases.batches(*shape)[:2]:
        for cyclic in (False, True):
            want, want_lab = refspeckle.speckle(d, 6, 16, cyclic, want_labels=True)
            t = _dev(ctx, d)
            plain = _run(ctx, t, 6, 16, cyclic)                              # out of place, labels_out NULL
            assert np.array_equal(t.cpu().numpy(), d), "the input was written"
            with_labels, lab = _run(ctx, t, 6, 16, cyclic, want_labels=True)
            t2 = _dev(ctx, d)
            same = ctx.dense_speckle(t2, options=dict(max_size=6, max_diff=16, cyclic=cyclic), out=t2)     # in place
            ctx.synchronize()
            assert same is t2
            t3 = _dev(ctx, d)
            in_place_lab = _run(ctx, t3, 6, 16, cyclic, want_labels=True, out=t3)[1]
            for got in (plain, with_labels, t2.cpu().numpy(), t3.cpu().numpy()):
                assert np.array_equal(got, want), (names, cyclic)
            assert np.array_equal(lab, want_lab) and np.array_equal(in_place_lab, want_lab)
            filled = []
            for byte in (0xFF, 0x00):
                ctx.debug_fill_scratch(byte)
                got, lab = _run(ctx, t, 6, 16, cyclic, want_labels=True)
                filled.append(got.tobytes() + lab.tobytes())
            assert filled[0] == filled[1] == want.tobytes() + want_lab.tobytes()


def test_argument_refusals_launch_nothing(ctx):
    """Every refusal returns SOSVO_ERR_ARG before any launch: the profile records no kernel."""
    import torch
    from vo_single_camera_sos_amd import _lib
    lib, h = ctx._lib, ctx._h
    d = _dev(ctx, speckle_cases.batches(12, 9)[0][1])
    out = torch.zeros((3, 12, 9), dtype=torch.int16, device=ctx.device)
    lab = torch.zeros((3, 12, 9), dtype=torch.int32, device=ctx.device)
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    ctx.profile_enable(True)

    def speckle(src=p(d), n=3, rows=12, cols=9, max_size=100, max_diff=16, flags=0, dst=p(out), labels=p(lab)):
        return lib.sosvo_dense_speckle(h, src, n, rows, cols, max_size, max_diff, flags, dst, labels)
    bad = [dict(rows=0), dict(cols=0), dict(rows=16385), dict(cols=16385), dict(rows=-1), dict(n=0), dict(n=-3), dict(n=32768),
           dict(max_size=-1), dict(max_size=-(1 << 31)), dict(max_diff=-1), dict(max_diff=32768), dict(flags=2), dict(flags=3),
           dict(flags=-1), dict(src=None), dict(dst=None)]
    for kw in bad:
        assert speckle(**kw) == -1, kw
    assert ctx.profile_read() == []
    assert speckle() == 0 and speckle(max_size=0, max_diff=0, labels=None) == 0 and speckle(max_size=(1 << 31) - 1, max_diff=32767, flags=1) == 0
    ctx.synchronize()
    names = [name for name, _ in ctx.profile_read()]
    assert len(names) == 3 * 4 and all(name.startswith("speckle_") for name in names)
    ctx.profile_enable(False)
    with pytest.raises(ValueError):
        ctx.dense_speckle(d, options=None)
    with pytest.raises(_lib.SosvoError):
        ctx.dense_speckle(d, options=_lib.SpeckleOptions(), out=out[:2])
    with pytest.raises(_lib.SosvoError):
        ctx.dense_speckle(d.to(torch.int32), options=_lib.SpeckleOptions())


@pytest.fixture(scope="module")
def rig():
    """The synthetic rig at Panorama(width=320) (33 rows), two rendered frames."""
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


def test_engine_equals_the_staged_calls_and_none_changes_nothing(ctx, rig):
    from vo_single_camera_sos_amd._lib import DenseOptions, SpeckleOptions
    from vo_single_camera_sos_amd.frontend import DeviceImageModel
    from vo_single_camera_sos_amd.pipeline import DenseOmniStereo, dense_mask
    model = DeviceImageModel(ctx, rig["gs"], (480, 640))
    cfg, o, sp = _rig_cfg(rig), DenseOptions(min_disparity=0), SpeckleOptions(max_size=12, max_diff=16, cyclic=True)
    mask = dense_mask(ctx, model)                 # (makes the model's unwrap table too)
    gray = ctx.unwrap_median_gray(_dev(ctx, rig["omni"]), model.unwrap_table, 0)
    raw = ctx.dense_stereo(gray[:2].contiguous(), gray[2:].contiguous(), mask, options=o)
    want_d16 = ctx.dense_speckle(raw, options=sp)
    want_X = ctx.dense_triangulate(cfg.as_struct(), want_d16, 1.0, 0.0)
    raw_X = ctx.dense_triangulate(cfg.as_struct(), raw, 1.0, 0.0)
    ctx.synchronize()
    raw_h, want_h = raw.cpu().numpy(), want_d16.cpu().numpy()
    assert np.array_equal(want_h, refspeckle.speckle(raw_h, 12, 16, cyclic=True))
    removed = int(((raw_h >= 0) & (want_h < 0)).sum())
    assert 0 < removed < (raw_h >= 0).sum() // 2, removed

    for speckle in (sp, dict(max_size=12, max_diff=16, cyclic=True)):
        eng = DenseOmniStereo(ctx, model, cfg, 2, options=o, speckle=speckle)
        assert eng.speckle == sp
        eng.load_frames(rig["omni"])
        ctx.profile_enable(True)
        d16, X = eng.step()
        depth = eng.depth()
        ctx.synchronize()
        names = [name for name, _ in ctx.profile_read()]
        ctx.profile_enable(False)
        assert sum(name.startswith("speckle_") for name in names) == 4
        assert d16 is eng.d16 and np.array_equal(d16.cpu().numpy(), want_h)
        assert np.array_equal(X.cpu().numpy(), want_X.cpu().numpy(), equal_nan=True)
        assert np.isnan(X.cpu().numpy()[want_h < 0]).all()
        with np.errstate(invalid="ignore"):
            want_depth = np.linalg.norm(X.cpu().numpy() - np.asarray(cfg.F_top), axis=-1).astype(np.float32)
        assert np.array_equal(depth.cpu().numpy(), want_depth, equal_nan=True)

    for kw in (dict(), dict(speckle=None)):          # off: the engine as it was, and no speckle kernel runs
        eng = DenseOmniStereo(ctx, model, cfg, 2, options=o, **kw)
        assert eng.speckle is None
        eng.load_frames(rig["omni"])
        ctx.profile_enable(True)
        d16, X = eng.step()
        ctx.synchronize()
        names = [name for name, _ in ctx.profile_read()]
        ctx.profile_enable(False)
        assert names and not any("speckle" in name for name in names)
        assert d16.cpu().numpy().tobytes() == raw_h.tobytes()
        assert np.array_equal(X.cpu().numpy(), raw_X.cpu().numpy(), equal_nan=True)
    with pytest.raises(ValueError):
        DenseOmniStereo(ctx, model, cfg, 2, options=o, speckle=dict(window=3))


def test_host_mirror_with_and_without_the_filter(ctx, rig):
    from vo_single_camera_sos_amd._lib import DenseOptions, SpeckleOptions
    from vo_single_camera_sos_amd.frontend import DeviceImageModel
    from vo_single_camera_sos_amd.pipeline import DenseOmniStereo
    gs, o, sp = rig["gs"], DenseOptions(), SpeckleOptions.from_tuner(12, 1, cyclic=True)
    assert sp == (12, 16, True)
    maps = {}
    for key, speckle in (("off", None), ("on", sp)):
        eng = DenseOmniStereo(ctx, DeviceImageModel(ctx, gs, (480, 640)), _rig_cfg(rig, 0.0, 0.0), 1, options=o, min_disparity=0.0,
                              speckle=speckle)
        eng.load_frames(rig["omni"][:1])
        d16, _ = eng.step()
        ctx.synchronize()
        maps[key] = d16.cpu().numpy()[0]
    assert not np.array_equal(maps["off"], maps["on"])
    gs.set_current_omni_image(rig["omni"][0], generate_panoramas=True)
    dmap0, dimg0 = gs.get_depth_map_from_panoramas(method="sgbm", options=o)                    # as before the keyword existed
    assert np.array_equal(gs.disparity_d16, maps["off"])
    dmap_none, dimg_none = gs.get_depth_map_from_panoramas(method="sgbm", options=o, speckle=None)
    assert np.array_equal(dmap_none, dmap0) and np.array_equal(dimg_none, dimg0) and len(gs._dense_engines) == 1
    for speckle in (sp, dict(max_size=12, max_diff=16, cyclic=True)):
        dmap, dimg = gs.get_depth_map_from_panoramas(method="sgbm", options=o, speckle=speckle)
        d16 = maps["on"]
        assert np.array_equal(gs.disparity_d16, d16) and len(gs._dense_engines) == 2
        assert np.array_equal(dmap, np.where(d16 >= 0, d16 / 16.0, 0.0)) and np.array_equal(dmap == 0, d16 == -1)
        assert np.array_equal(dimg, np.where(d16 >= 0, np.clip((d16 / 16.0 - 1) * 255.0 / 63, 0, 255), 0).astype(np.uint8))
        assert np.array_equal(dmap, gs.disparity_map) and np.array_equal(dimg, gs.disparity_img)
    (xyz, _), _ = gs.triangulate_from_depth_map(min_disparity=1)
    gs.get_depth_map_from_panoramas(method="sgbm", options=o)
    (xyz0, _), _ = gs.triangulate_from_depth_map(min_disparity=1)
    assert 0 < xyz.shape[1] < xyz0.shape[1]          # the removed islands are no longer points of the cloud
