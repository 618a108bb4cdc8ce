"""GPU: the stages of the seam-free front end and the front end itself.  The reference of every check is
the project's plain entry point on host-padded inputs (tests/refseam.py: pad, pad0, unpad), bit for bit; the fixture's counts
are the CPU oracle's (tests/test_seam_free_reference.py)."""
import numpy as np
import pytest
import torch

import matching_scenes as scenes
import refseam
from refseam import HALO
from vo_single_camera_sos_amd import _lib, orb_pattern, synthetic
from vo_single_camera_sos_amd._lib import SosvoError
from vo_single_camera_sos_amd.frontend import DeviceImageModel, ImageFrontEnd

pytestmark = pytest.mark.gpu


def _dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _same_words(a, b):
    """Two uint32 tensors, word for word."""
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- the table ---------------------------------------------------------------------------------------------------------------
def _maps(rng, H, W, rows, cols, nan_share=0.05):
    """Map values all over the frame and a little beyond it, with NaN entries."""
    mx = rng.uniform(-6.0, W + 6.0, (2, rows, cols)).astype(np.float32)
    my = rng.uniform(-6.0, H + 6.0, (2, rows, cols)).astype(np.float32)
    mx[rng.random((2, rows, cols)) < nan_share] = np.nan
    my[rng.random((2, rows, cols)) < nan_share] = np.nan
    return mx, my


def _annulus(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.hypot(yy - H / 2.0, xx - W / 2.0)
    return np.stack([(r > 0.15 * H) & (r < 0.48 * H), (r > 0.05 * H) & (r < 0.3 * H)]).astype(np.uint8)


@pytest.mark.parametrize("rows,cols", [(12, 40), (12, 48), (33, 200)])
def test_table_equals_unwrap_prepare_on_padded_maps(ctx, rows, cols):
    H, W = 64, 48
    mx, my = _maps(np.random.default_rng(rows * cols), H, W, rows, cols)
    masks = _dev(ctx, _annulus(H, W))
    for m in (masks, None):
        got = ctx.unwrap_prepare_seam_free(m, _dev(ctx, mx), _dev(ctx, my), (H, W))
        want = ctx.unwrap_prepare(m, _dev(ctx, refseam.pad(mx, axis=2)), _dev(ctx, refseam.pad(my, axis=2)), (H, W))
        ctx.synchronize()
        assert got.shape == (2, rows, cols + 2 * HALO, 2) and _same_words(got, want)
        assert int((want.view(torch.int32) != 0).sum()) > rows * cols // 4         # (the table is not empty)


def test_table_of_a_frame_above_4_mb(ctx):
    """1200 x 1200: the pixels whose first tap lies beyond byte 4 194 303 take the other entry format; both are covered."""
    H = W = 1200
    mx, my = _maps(np.random.default_rng(7), H, W, 8, 64, nan_share=0.02)
    my[:, :, ::2] = np.random.default_rng(8).uniform(1166.0, H - 2.0, my[:, :, ::2].shape).astype(np.float32)     # beyond 4 MB
    got = ctx.unwrap_prepare_seam_free(None, _dev(ctx, mx), _dev(ctx, my), (H, W))
    want = ctx.unwrap_prepare(None, _dev(ctx, refseam.pad(mx, axis=2)), _dev(ctx, refseam.pad(my, axis=2)), (H, W))
    ctx.synchronize()
    assert _same_words(got, want)
    y = want.cpu().numpy().view(np.uint32)[..., 1]
    assert (y >> 31).any() and ((y >> 31) == 0).any()                                # both entry formats occur


def test_stage_refusals(ctx):
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=ctx.device)  # noqa: E731
    with pytest.raises(SosvoError):
        ctx.unwrap_prepare_seam_free(None, z(2, 4, 39), z(2, 4, 39), (64, 48))       # cols < 40
    with pytest.raises(SosvoError):
        ctx.unwrap_prepare_seam_free(None, z(2, 4, 48), z(2, 4, 48), (1, 48))        # the frame-size rule of the table
    kp, n = z(2, 4, 2), torch.zeros(2, dtype=torch.int32, device=ctx.device)
    for period in (0, 16385):
        with pytest.raises(SosvoError):
            ctx.keypoints_unpad(kp, n, period)
    with pytest.raises(SosvoError):                                                   # row_range needs both views' images
        ctx.gray_unpad(torch.zeros((3, 4, 128), dtype=torch.uint8, device=ctx.device), 48,
                       row_range=torch.zeros((2, 2), dtype=torch.int32, device=ctx.device))


# ---- mask pad, keypoint unpad, gray unpad ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsets,rows,cols", [(2, 9, 40), (1, 3, 257), (3, 17, 300)])
def test_mask_pad_against_numpy(ctx, nsets, rows, cols):
    bits = np.random.default_rng(cols).integers(0, 2 ** 32, (nsets, rows, cols), dtype=np.uint32)
    out = _dev(ctx, np.full((nsets, rows, cols + 2 * HALO), 0xDEADBEEF, np.uint32))
    got = ctx.mask_bits_seam_free(_dev(ctx, bits), out=out)
    ctx.synchronize()
    assert np.array_equal(got.cpu().numpy(), refseam.pad0(bits))


def test_keypoint_unpad_against_numpy(ctx):
    W, cap = 256, 300            # (more than one block of 256 keypoints)
    rng = np.random.default_rng(3)
    hand = np.array([39.5, 40.0, W + 39.96875, W + 40.0, 40.0 - 2.0 ** -10, np.nextafter(np.float32(40.0), np.float32(0.0)), 41.25, 79.0],
                    np.float32)
    kp = np.stack([rng.uniform(34.0, W + 46.0, (5, cap)), rng.uniform(0.0, 96.0, (5, cap))], -1).astype(np.float32)
    kp[1, :32, 0] = (rng.integers(0, (W + 80) * 32, 32) / 32.0).astype(np.float32)       # the detector's grid
    kp[2, :len(hand), 0] = hand
    n = np.array([0, 1, len(hand), cap, cap + 7], np.int32)                              # (a count beyond the capacity is cut to it)
    d = _dev(ctx, kp)
    ctx.keypoints_unpad(d, _dev(ctx, n), W)
    ctx.synchronize()
    got, want = d.cpu().numpy(), kp.copy()
    for p, cnt in enumerate(np.minimum(n, cap)):
        want[p, :cnt, 0] = refseam.unpad(kp[p, :cnt, 0], W)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))                     # rows beyond the counts and y: untouched
    assert np.array_equal(got[2, :len(hand), 0], np.array([W - 0.5, 0.0, W - 0.03125, 0.0, W - 2.0 ** -10, 0.0, 1.25, 39.0], np.float32))
    assert got[3, :, 0].min() >= 0 and got[3, :, 0].max() < W


@pytest.mark.parametrize("cols", [48, 61])       # (rows of whole words, and a width that is copied byte by byte)
def test_gray_unpad_under_a_row_range(ctx, cols):
    rows, nimg = 21, 6
    gray = np.random.default_rng(cols).integers(0, 256, (nimg, rows, cols + 2 * HALO), dtype=np.uint8)
    rr = np.array([[3, 17], [0, 9]], np.int32)
    out = torch.full((nimg, rows, cols), 0xA5, dtype=torch.uint8, device=ctx.device)
    got = ctx.gray_unpad(_dev(ctx, gray), cols, row_range=_dev(ctx, rr), out=out).cpu().numpy()
    want = np.full((nimg, rows, cols), 0xA5, np.uint8)
    for i in range(nimg):
        r0, r1 = rr[i // 3]
        want[i, r0:r1] = gray[i, r0:r1, HALO:HALO + cols]
    assert np.array_equal(got, want)                                                     # rows outside the range: untouched
    full = ctx.gray_unpad(_dev(ctx, gray), cols).cpu().numpy()
    assert np.array_equal(full, gray[:, :, HALO:HALO + cols])
    odd = ctx.gray_unpad(_dev(ctx, gray[:3]), cols).cpu().numpy()                        # (no range: any image count)
    assert np.array_equal(odd, gray[:3, :, HALO:HALO + cols])


# ---- the front end -----------------------------------------------------------------------------------------------------------
def _model(ctx, map_x, map_y, omni_masks, bits, nmask):
    """A DeviceImageModel from arrays (the constructor's members, without a rig)."""
    m = DeviceImageModel.__new__(DeviceImageModel)
    m.H, m.W = omni_masks.shape[1:]
    m.rows, m.cols = map_x.shape[1:]
    m.map_x, m.map_y, m.omni_masks = _dev(ctx, map_x.astype(np.float32)), _dev(ctx, map_y.astype(np.float32)), _dev(ctx, omni_masks)
    m.nmask, m.mask_bits_host = nmask, np.ascontiguousarray(bits, np.uint32)
    m.mask_bits = _dev(ctx, m.mask_bits_host)
    m.pattern_host = orb_pattern.orb_pattern()
    m.pattern = _dev(ctx, m.pattern_host)
    m.seam_free, m.cols_run = False, m.cols
    return m


def _host_padded(ctx, m):
    """The plain model of the host-padded maps and masks: the GPU reference's input."""
    return _model(ctx, refseam.pad(m.map_x.cpu().numpy(), axis=2), refseam.pad(m.map_y.cpu().numpy(), axis=2), m.omni_masks.cpu().numpy(),
                  refseam.pad0(m.mask_bits_host), m.nmask)


def _fixture_model(ctx, roll=0):
    """The fixture seen through identity-like maps: the top view reads the frame's pixels themselves (rolled by `roll`
    columns), the bottom view a quarter pixel beside and below them."""
    P, bits = refseam.fixture()
    R, W = P.shape[:2]
    yy, xx = np.mgrid[0:R, 0:W].astype(np.float32)
    xx = (xx - roll) % W
    mx, my = np.stack([xx, xx + 0.25]), np.stack([yy, yy + 0.25])
    return P, _model(ctx, mx, my, np.ones((2, R, W), np.uint8), np.stack([bits, bits]), 4)


def _run(ctx, model, omni, **kw):
    fe = ImageFrontEnd(ctx, model, len(omni), **dict(dict(num_of_features=refseam.MAX_CORNERS), **kw))
    fe.load_frames(omni)
    fe.run()
    ctx.synchronize()
    return fe, fe.kp.cpu().numpy(), fe.n.cpu().numpy(), fe.desc.cpu().numpy()


def _assert_is_the_plain_front_end_on_padded_inputs(ctx, model, omni, **kw):
    """-> the seam-free front end's (kp, n, desc), after the comparison."""
    fe, kp, n, desc = _run(ctx, model.seam_free_form(ctx), omni, **kw)
    ref, kp_r, n_r, desc_r = _run(ctx, _host_padded(ctx, model), omni, **kw)
    assert fe.seam_free and not ref.seam_free and fe.gray.shape == ref.gray.shape == (2 * len(omni), model.rows, model.cols + 2 * HALO)
    assert torch.equal(fe.gray, ref.gray)
    if fe.pano is not None:
        assert torch.equal(fe.pano, ref.pano)
    want = kp_r.copy()
    for p, cnt in enumerate(np.minimum(n_r, kp_r.shape[1])):
        want[p, :cnt, 0] = refseam.unpad(kp_r[p, :cnt, 0], model.cols)
    assert np.array_equal(n, n_r) and n.sum() > 0
    assert np.array_equal(kp.view(np.uint32), want.view(np.uint32)) and np.array_equal(desc, desc_r)
    for p, cnt in enumerate(n):
        assert (kp[p, :cnt, 0] >= 0).all() and (kp[p, :cnt, 0] < model.cols).all()
    # the interior of the padded gray is what the cyclic tracker reads
    assert torch.equal(fe.gray_interior(), ref.gray[:, :, HALO:HALO + model.cols].contiguous())
    return kp, n, desc


@pytest.mark.parametrize("kw", [dict(), dict(keep_panoramas=False), dict(subpix=5), dict(median_win_size=0), dict(detection_method="FAST"),
                                dict(detection_method="AGAST", keep_panoramas=False), dict(keep_panoramas=False, subpix=5, median_win_size=5)],
                         ids=["gft", "gft_fused", "gft_subpix5", "gft_median0", "fast", "agast_fused", "gft_fused_subpix5_median5"])
def test_front_end_equals_the_plain_one_on_the_host_padded_model(ctx, kw):
    P, model = _fixture_model(ctx)
    kp, n, _ = _assert_is_the_plain_front_end_on_padded_inputs(ctx, model, P[None], **kw)
    if kw.get("subpix") is None:        # the detectors' positions are on the grid: keypoints in the 31-column bands exist
        x = np.concatenate([kp[p, :c, 0] for p, c in enumerate(n)])
        assert ((x < 31) | (x >= 256 - 31)).any()


def test_front_end_on_the_rig(ctx):
    """The rendered rig (480 x 640 frames, 1200-column panoramas, 12 azimuthal masks), two frames, the fused median under its
    row range: the plain front end keeps no keypoint within 31 columns of the seam, the seam-free one does."""
    gs, _ = scenes.rig()
    model = DeviceImageModel(ctx, gs, (480, 640))
    omni, _ = synthetic.make_frame_pairs(gs, 1, seed=99)
    kp, n, _ = _assert_is_the_plain_front_end_on_padded_inputs(ctx, model, omni, keep_panoramas=False, num_of_features=300)
    _, kp0, n0, _ = _run(ctx, model, omni, keep_panoramas=False, num_of_features=300)
    band = lambda k, c: int(sum((((k[p, :q, 0] < 31) | (k[p, :q, 0] >= model.cols - 31)).sum()) for p, q in enumerate(c)))  # noqa: E731
    print("rig: %d keypoints plain (%d in the bands), %d seam-free (%d in the bands)" % (n0.sum(), band(kp0, n0), n.sum(), band(kp, n)))
    assert band(kp0, n0) == 0 and band(kp, n) > 0 and n.sum() > n0.sum()


def _per_mask(kp, n, desc, view=0, nmask=4):
    return [(kp[view * nmask + m, :n[view * nmask + m]], desc[view * nmask + m, :n[view * nmask + m]]) for m in range(nmask)]


def test_the_fixtures_counts_and_rolls(ctx):
    """The oracle's table (tests/test_seam_free_reference.py) on the device, top view (identity maps: the panorama IS the
    fixture), and the three rolls by whole sectors, done by rolling the maps' columns."""
    P, model = _fixture_model(ctx)
    _, kp, n, desc = _run(ctx, model.seam_free_form(ctx), P[None])
    _, kp0, n0, _ = _run(ctx, model, P[None])
    assert list(n0[:4]) == [15, 37, 37, 20] and list(n[:4]) == [33, 37, 37, 35]
    base = _per_mask(kp, n, desc)
    x = np.concatenate([k[:, 0] for k, _ in base])
    assert (int((x < 31).sum()), int((x >= 256 - 31).sum()), int(((x < 5) | (x >= 251)).sum())) == (18, 15, 8)
    oracle_sf = refseam.front_end(P, refseam.fixture()[1], seam_free=True)
    for (k, d), (ko, do) in zip(base, oracle_sf):                                     # ... and the oracle's keypoints themselves
        assert np.array_equal(k, ko) and np.array_equal(d, do)
    for shift in (64, 128, 192):
        _, rolled = _fixture_model(ctx, roll=shift)
        _, kp_r, n_r, desc_r = _run(ctx, rolled.seam_free_form(ctx), P[None])
        for m, (k, d) in enumerate(_per_mask(kp_r, n_r, desc_r)):
            kb, db = base[(m - shift // 64) % 4]
            want = kb.copy()
            want[:, 0] = (want[:, 0] + shift) % 256
            assert np.array_equal(k, want) and np.array_equal(d, db), (shift, m)


def test_front_end_refusals(ctx):
    P, model = _fixture_model(ctx)
    sf = model.seam_free_form(ctx)
    assert sf is model.seam_free_form(ctx) and sf.cols == 256 and sf.cols_run == 336 and sf.mask_bits is model.mask_bits
    with pytest.raises(ValueError, match="ORB"):
        ImageFrontEnd(ctx, sf, 1, detection_method="ORB")
    with pytest.raises(ValueError, match="edge"):
        ImageFrontEnd(ctx, sf, 1, edge=32)
    narrow = _model(ctx, np.zeros((2, 8, 32)), np.zeros((2, 8, 32)), np.ones((2, 16, 16), np.uint8), np.ones((2, 8, 32), np.uint32), 1)
    with pytest.raises(ValueError, match="32"):
        narrow.seam_free_form(ctx)


def test_batch_refusals_at_call_time(ctx):
    """What only the call can see (the context's stereo-LK settings), and the C layer's own refusal of a flag word that the
    Python layers never build."""
    from vo_single_camera_sos_amd.pipeline import FramePairBatch, RigConfig
    gs, rig_kw = scenes.rig()
    model = DeviceImageModel(ctx, gs, (480, 640))
    b = FramePairBatch(ctx, model, RigConfig(**rig_kw), 1, num_of_features=100, frame_cap=256, max_iter=50, cyclic_columns="seam_free",
                       stereo_refine="lk", stereo_lk=dict(half=10, max_shift=23))
    b.options = b.options._replace(stereo_lk=_lib.StereoLKOptions(half=10, max_shift=24))      # 2 + 10 + 24 > 35
    with pytest.raises(SosvoError, match="35"):
        b.step()
    b = FramePairBatch(ctx, model, RigConfig(**rig_kw), 1, num_of_features=100, frame_cap=256, max_iter=50, cyclic_columns="seam_free")
    b.cfg.ransac_flags &= ~_lib.FLAG_CYCLIC_F2F
    assert ctx.frame_pair_batch_workspace(b.cfg) == 0
    with pytest.raises(SosvoError, match="CYCLIC"):
        b.step()
    ctx.set_stereo_lk_options(_lib.StereoLKOptions())
