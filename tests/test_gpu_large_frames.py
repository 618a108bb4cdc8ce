"""The table-driven unwrap (sosvo_unwrap_prepare -> sosvo_unwrap_table / sosvo_unwrap_median_gray[_rows]) at the two ends
of its frame-size range, bit for bit against the oracle's map form (oracle.unwrap works per byte and takes no table: it
shares none of the code under test).

Large end: a tap beyond byte 4 194 303 of a frame does not fit the 22-bit offset of a fast table entry and takes the edge
format (int16 ix, iy; csrc/image.hip), for interior pixels too.  No frame of at most 4 MB -- every other test, the soak
and the fuzzer's small draws -- reaches that branch.  The frames here are the smallest that do: (1100, 1280) just over
4 MB, and (90, 16384) / (16384, 90) with W / H at the accepted limit, i.e. ix / iy up to 16387 in the int16 fields.  The
maps are built by construction (tests/unwrap_cases.py: (a) uniform with NaN, (b) a band around the last fast pixel, (c)
~40 % of view 1 beyond 4 MB, (d) the frame's last pixels); a CPU test asserts that they reach the branch, and the GPU
test reads the table back and pins its format.

Small end: the per-frame kernels load 8 bytes at a tap offset and at that offset + 3 W unconditionally, so a frame must
hold 8 bytes after the start of its second row (3 W (H - 1) >= 8).  Smaller frames are refused by every entry point that
reads frames through the table; the smallest accepted ones are compared with the oracle (nearly every entry is an edge or
zero entry there); the map form sosvo_unwrap accepts every size."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle
import unwrap_cases as uc
from vo_single_camera_sos_amd import _lib

gpu = pytest.mark.gpu
NFRAMES = 3          # frame, view and last-frame indexing all differ
KSIZES = (0, 3, 5, 11)
SENTINEL = 0xA5
TINY_REFUSED = [(1, 1), (1, 5), (2, 2), (1, 16384)]
TINY_ACCEPTED = [(2, 3), (3, 2), (4, 1), (3, 3)]
OVER_LIMIT = [(16385, 2), (2, 16385)]
RULE = "3 * W * (H - 1) >= 8"


def _to(dev, *arrs):
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrs]     # (a copy: the shared inputs are read-only)


@functools.lru_cache(maxsize=None)
def _frames(shape):
    omni = np.random.default_rng(shape[0] * 7 + shape[1]).integers(0, 256, (NFRAMES,) + shape + (3,), dtype=np.uint8)
    omni.setflags(write=False)
    return omni


@functools.lru_cache(maxsize=None)
def _case(shape, pshape):
    """-> maps (a) - (d) and the masks (e) of one frame shape and panorama shape (shared, read-only)."""
    rng = np.random.default_rng([shape[0], shape[1], pshape[0], pshape[1]])
    if shape in uc.LARGE_FRAMES:
        mx, my = uc.large_frame_maps(rng, shape[0], shape[1], pshape)
    else:
        mx, my = uc.uniform_maps(rng, shape[0], shape[1], pshape)
    masks = uc.masks_for(rng, shape[0], shape[1])
    for a in (mx, my, masks):
        a.setflags(write=False)
    return mx, my, masks


def _row_range(rows):
    """A range that starts and ends inside the panorama, different for the two views."""
    return [[rows // 4, rows - rows // 5], [rows // 8, rows - 3]]


# ---- the inputs reach the branch (CPU) --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(uc.LARGE_FRAMES))
@pytest.mark.parametrize("pshape", uc.PANO_SHAPES)
def test_large_frame_maps_reach_the_far_entries(shape, pshape):
    """A condition on the inputs, not a measurement: at least a quarter of view 1 are FAR entries (fast-shaped pixels whose
    off0 does not fit 22 bits), the band (b) holds both formats, and the eight pixels around the boundary split 4 / 4."""
    H, W = shape
    mx, my, masks = _case(shape, pshape)
    for m in (masks, None):
        view = [uc.classify(mx[v], my[v], None if m is None else m[v], H, W) for v in range(2)]
        far_share = float((view[1]["kind"] == uc.FAR).mean())
        print("frame %s pano %s masked %s: far share of view 1 %.3f" % (shape, pshape, m is not None, far_share))
        assert far_share >= 0.25, far_share
        band = view[0]["kind"][list(uc.BAND_ROWS)]
        assert (band == uc.FAST).sum() >= 10 and (band == uc.FAR).sum() >= 10, np.bincount(band.ravel(), minlength=4)
        eight = view[0]["kind"][uc.BAND_ROWS[0], uc.BOUNDARY_COLS]
        assert list(eight) == [uc.FAST] * 4 + [uc.FAR] * 4, eight
        pix = (view[0]["iy"] * W + view[0]["ix"])[uc.BAND_ROWS[0], uc.BOUNDARY_COLS]
        assert np.array_equal(pix, uc.BOUNDARY_PIXELS)
        assert view[0]["off0"][uc.BAND_ROWS[0], uc.BOUNDARY_COLS][3] == uc.TAB_OFF_MASK
        for v in range(2):   # (a) and (d): every kind occurs, and ix / iy use the top of the accepted range
            assert set(np.unique(view[v]["kind"])) == {uc.ZERO, uc.FAST, uc.FAR, uc.BORDER}
            edge = view[v]["kind"] >= uc.FAR
            assert view[v]["ix"][edge].max() >= W - 1 and view[v]["iy"][edge].max() >= H - 1
    if W == 16384:
        assert view[1]["ix"][view[1]["kind"] == uc.FAR].max() > 16000
    if H == 16384:
        assert view[1]["iy"][view[1]["kind"] == uc.FAR].max() > 16000


def test_fuzzer_draws_large_frames_and_no_refused_frame():
    """scripts/fuzz_parity.py's `unwrap` stage: about one draw in eight is one of the large frames (all three occur, with
    maps that reach the far entries), and no draw is a frame size the table form refuses."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fuzz_parity_module", os.path.join(root, "scripts", "fuzz_parity.py"))
    fp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fp)
    rng = np.random.default_rng(11)
    large = []
    for _ in range(400):
        params, mx, my = fp.draw_unwrap(rng)
        H, W = params["H"], params["W"]
        assert 1 <= H <= 16384 and 1 <= W <= 16384 and 3 * W * (H - 1) >= 8, params
        assert mx.shape == my.shape == (2, params["rows"], params["cols"]) and mx.dtype == my.dtype == np.float32
        if params["large"]:
            large.append((H, W))
            assert (uc.classify(mx[1], my[1], None, H, W)["kind"] == uc.FAR).mean() >= 0.25, params
    assert set(large) == set(uc.LARGE_FRAMES) and 400 / 16 <= len(large) <= 400 / 4, len(large)


def test_frame_size_rule_cases():
    """The rule as the tests use it: what is refused has fewer than 8 bytes after the start of its second row."""
    assert all(3 * W * (H - 1) < 8 for H, W in TINY_REFUSED) and all(3 * W * (H - 1) >= 8 for H, W in TINY_ACCEPTED)


# ---- parity of every consumer ------------------------------------------------------------------------------------------
def _check_table(table, mx, my, masks, H, W):
    """The table sosvo_unwrap_prepare wrote, against the numpy restatement of its format."""
    tab = table.view(torch.int32).cpu().numpy().view(np.uint32)
    for v in range(2):
        c = uc.classify(mx[v], my[v], None if masks is None else masks[v], H, W)
        x, y, kind = tab[v, :, :, 0], tab[v, :, :, 1], c["kind"]
        assert np.array_equal((y >> 31) == 1, kind >= uc.FAR), v                       # bit 31: exactly far + border
        fast, edge = kind == uc.FAST, kind >= uc.FAR
        assert np.array_equal((x & uc.TAB_OFF_MASK)[fast], c["off0"][fast]), v
        assert np.array_equal((x & 0xFFFF).astype(np.uint16).view(np.int16)[edge], c["ix"][edge]), v
        assert np.array_equal((x >> 16).astype(np.uint16).view(np.int16)[edge], c["iy"][edge]), v
        assert np.array_equal(x, c["x"]) and np.array_equal(y, c["y"]), v               # and every other field


def _check_consumers(ctx, omni, masks, mx, my):
    """unwrap_prepare's table, unwrap_table, unwrap_median_gray for every window and its row-range form against the oracle
    chain oracle.unwrap -> oracle.median_gray."""
    F, H, W = omni.shape[:3]
    rows, cols = mx.shape[1:]
    t_omni, t_mx, t_my = _to(ctx.device, omni, mx, my)
    tm = None if masks is None else _to(ctx.device, masks)[0]
    table = ctx.unwrap_prepare(tm, t_mx, t_my, (H, W))
    pano = ctx.unwrap_table(t_omni, table)
    gray = {k: ctx.unwrap_median_gray(t_omni, table, k) for k in KSIZES}
    rng_rows = _row_range(rows)
    rr = torch.tensor(rng_rows, dtype=torch.int32, device=ctx.device)
    part = {k: ctx.unwrap_median_gray(t_omni, table, k, gray=torch.full_like(gray[k], 77), row_range=rr) for k in (3, 11)}
    ctx.synchronize()
    pano = pano.cpu().numpy()
    gray = {k: g.cpu().numpy().reshape(2, F, rows, cols) for k, g in gray.items()}
    part = {k: g.cpu().numpy().reshape(2, F, rows, cols) for k, g in part.items()}
    for v in range(2):
        lo, hi = rng_rows[v]
        for f in range(F):
            want = oracle.unwrap(omni[f], None if masks is None else masks[v], mx[v], my[v])
            assert np.array_equal(pano[v, f], want), (v, f)
            for k in KSIZES:
                want_gray = oracle.median_gray(want, k)
                assert np.array_equal(gray[k][v, f], want_gray), (v, f, k)
                if k in part:
                    assert np.array_equal(part[k][v, f, lo:hi], want_gray[lo:hi]), (v, f, k)
                    assert (part[k][v, f, :lo] == 77).all() and (part[k][v, f, hi:] == 77).all(), (v, f, k)
    _check_table(table, mx, my, masks, H, W)
    return pano


@gpu
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("pshape", uc.PANO_SHAPES)
@pytest.mark.parametrize("shape", list(uc.LARGE_FRAMES))
def test_large_frames_equal_oracle(ctx, shape, pshape, masked):
    """Frames above 4 MB and at the 16384 limits: far entries for interior pixels, W in the thousands, ix / iy near the top
    of the int16 fields, through unwrap_lut_kernel, unwrap_gray_kernel<2 | 4> ((24, 130) / (32, 70)) and the fused median."""
    mx, my, masks = _case(shape, pshape)
    pano = _check_consumers(ctx, _frames(shape), masks if masked else None, mx, my)
    assert pano[1].any() and pano[0, :, list(uc.BAND_ROWS)].any()      # the far pixels and the band produce image content


@gpu
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("shape", TINY_ACCEPTED)
def test_smallest_accepted_frames_equal_oracle(ctx, shape, masked):
    """The smallest frames the rule 3 W (H - 1) >= 8 accepts: nearly every entry is an edge or zero entry, the clamp of the
    loads works on a frame of 18 / 12 / 27 bytes, and the last frame of the batch ends the buffer."""
    for pshape in uc.PANO_SHAPES:
        mx, my, masks = _case(shape, pshape)
        _check_consumers(ctx, _frames(shape), masks if masked else None, mx, my)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _refused(ctx, lib, name, *args):
    rc = getattr(lib, name)(ctx._h, *args)
    msg = lib.sosvo_last_error(ctx._h).decode()
    assert rc == -1 and name in msg, (name, rc, msg)          # SOSVO_ERR_ARG
    return msg


def _image_calls(ctx, H, W, pshape=(4, 6)):
    """Buffers of the RIGHT size for an (H, W) frame (a call that was wrongly accepted would stay inside them), the outputs
    filled with a sentinel, and the image entry points' raw argument lists."""
    rows, cols = pshape
    dev = ctx.device
    b = SimpleNamespace(
        omni=torch.zeros((1, H, W, 3), dtype=torch.uint8, device=dev), mx=torch.zeros((2, rows, cols), device=dev),
        my=torch.zeros((2, rows, cols), device=dev), zero_table=torch.zeros((2, rows, cols, 2), dtype=torch.int32, device=dev),
        table=torch.full((2, rows, cols, 8), SENTINEL, dtype=torch.uint8, device=dev),
        pano=torch.full((2, 1, rows, cols, 3), SENTINEL, dtype=torch.uint8, device=dev),
        gray=torch.full((2, rows, cols), SENTINEL, dtype=torch.uint8, device=dev),
        rr=torch.tensor([[0, rows], [0, rows]], dtype=torch.int32, device=dev))
    p = lambda t: t.data_ptr()
    calls = [("sosvo_unwrap_prepare", (None, p(b.mx), p(b.my), H, W, rows, cols, p(b.table))),
             ("sosvo_unwrap_table", (p(b.omni), p(b.zero_table), 1, H, W, rows, cols, p(b.pano)))]
    for k in KSIZES:
        calls.append(("sosvo_unwrap_median_gray", (p(b.omni), p(b.zero_table), 1, H, W, rows, cols, k, p(b.gray))))
        calls.append(("sosvo_unwrap_median_gray_rows", (p(b.omni), p(b.zero_table), 1, H, W, rows, cols, k, p(b.rr), p(b.gray))))
    map_form = ("sosvo_unwrap", (p(b.omni), None, p(b.mx), p(b.my), 1, H, W, rows, cols, p(b.pano)))
    return b, calls, map_form


def _untouched(ctx, b):
    ctx.synchronize()
    for t in (b.table, b.pano, b.gray):
        assert bool((t == SENTINEL).all())


@gpu
@pytest.mark.parametrize("shape", OVER_LIMIT)
def test_frames_beyond_16384_are_refused(ctx, shape):
    """H = 16385 or W = 16385: SOSVO_ERR_ARG from the map form and from every table entry point, outputs untouched (16384
    itself is accepted: test_large_frames_equal_oracle)."""
    lib = _lib.load()
    b, calls, map_form = _image_calls(ctx, *shape)
    for name, args in [map_form] + calls:
        _refused(ctx, lib, name, *args)
    _untouched(ctx, b)


@gpu
@pytest.mark.parametrize("shape", TINY_REFUSED)
def test_frames_without_8_bytes_after_the_second_row_start_are_refused(ctx, shape):
    """3 W (H - 1) < 8: sosvo_unwrap_prepare and the table's consumers answer SOSVO_ERR_ARG with the rule in the message
    and leave the outputs alone; the map form has no 8-byte loads and keeps accepting the frame (checked on (1, 1) below)."""
    lib = _lib.load()
    b, calls, _ = _image_calls(ctx, *shape)
    for name, args in calls:
        assert RULE in _refused(ctx, lib, name, *args), name
    _untouched(ctx, b)


@gpu
@pytest.mark.parametrize("shape", TINY_REFUSED + OVER_LIMIT)
def test_batch_and_sequence_entry_points_refuse_the_frame_size(ctx, shape):
    """The one-call batch, its streams forms and the sequence front ends read frames through the table: the same refusal,
    before anything is launched (the dummy buffers are far too small for a call that went on; such a call would still end at
    its workspace-size check)."""
    from vo_single_camera_sos_amd.pipeline import batch_cfg
    lib = _lib.load()
    model = SimpleNamespace(H=shape[0], W=shape[1], rows=40, cols=72, nmask=2)
    cfg = batch_cfg(model, 2, 50, 64, 128, 11, 0.01, 5.0, 31, None, 50, False, 0, 5, "P3P", "GFT")
    rig = _lib.Rig()
    buf = torch.full((4096,), SENTINEL, dtype=torch.uint8, device=ctx.device)
    slots = (ctypes.c_int32 * 2)(0, 1)
    p, r, c = buf.data_ptr(), ctypes.cast(ctypes.pointer(rig), _lib.c_p), ctypes.cast(ctypes.pointer(cfg), _lib.c_p)
    msgs = [_refused(ctx, lib, "sosvo_frame_pair_batch", r, c, p, p, p, p, p, 256, p),
            _refused(ctx, lib, "sosvo_frame_pair_batch_streams", r, c, 2, p, p, p, p, p, 256, p),
            _refused(ctx, lib, "sosvo_frame_pair_batch_streams_enqueue", r, c, 2, p, p, p, p, p, 256, p),
            _refused(ctx, lib, "sosvo_sequence_front_end", r, c, 2, 4, p, 2, 0, p, p, p, p, 256),
            _refused(ctx, lib, "sosvo_sequence_front_end_slots", r, c, 2, 4, p, 2, ctypes.cast(slots, _lib.c_p), p, p, p, p, 256)]
    assert all(RULE in m for m in msgs), msgs
    assert lib.sosvo_frame_pair_batch_streams_join(ctx._h) == 0
    ctx.synchronize()
    assert bool((buf == SENTINEL).all())


@gpu
def test_map_form_accepts_a_one_pixel_frame(ctx):
    """sosvo_unwrap on a (1, 1) frame (and the other frames the table form refuses) against the oracle."""
    for shape in TINY_REFUSED[:3]:
        H, W = shape
        rng = np.random.default_rng(H * 100 + W)
        omni = rng.integers(1, 256, (NFRAMES, H, W, 3), dtype=np.uint8)
        mx, my = uc.uniform_maps(rng, H, W, (24, 130))
        mx[0, 0, :3], my[0, 0, :3] = [0.0, -0.5, 0.25], [0.0, 0.0, -0.75]
        masks = np.full((2, H, W), 255, np.uint8)
        masks[1, 0, 0] = 0
        t_omni, t_masks, t_mx, t_my = _to(ctx.device, omni, masks, mx, my)
        for tm, hm in ((t_masks, masks), (None, [None, None])):
            pano = ctx.unwrap(t_omni, tm, t_mx, t_my)
            ctx.synchronize()
            pano = pano.cpu().numpy()
            for v in range(2):
                for f in range(NFRAMES):
                    assert np.array_equal(pano[v, f], oracle.unwrap(omni[f], hm[v], mx[v], my[v])), (shape, v, f)
        assert pano[0].any()
