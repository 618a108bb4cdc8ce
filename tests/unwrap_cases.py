"""Inputs that drive the table-driven unwrap kernels into the entry formats small frames never reach, and a numpy
restatement of the table format (shared by tests/test_gpu_large_frames.py and scripts/fuzz_parity.py; no GPU needed).

A table entry (csrc/image.hip, "K1, table-driven form") is one of
    ZERO    no valid tap: the all-zero entry,
    FAST    off0 = 3 (iy W + ix) and the four weights, both 8-byte row loads inside the frame and off0 <= 0x3FFFFF,
    FAR     the same pixel geometry (both row loads inside the frame) but off0 > 0x3FFFFF: stored in the edge format,
    BORDER  a row load would start before the frame or end beyond it: the edge format, loads clamped and shifted back.
Frames of at most 4 MB (everything else in the suite) have no FAR entries; the maps built here consist mostly of them.
"""
import numpy as np

TAB_OFF_MASK = 0x3FFFFF
TAB_EDGE = 0x80000000
LAST_FAST_PIXEL = TAB_OFF_MASK // 3                # 1398101: off0 == 0x3FFFFF, the last pixel index a fast entry can hold
BOUNDARY_PIXELS = np.arange(LAST_FAST_PIXEL - 3, LAST_FAST_PIXEL + 5)      # 1398098 .. 1398105: four fast, four far
ZERO, FAST, FAR, BORDER = 0, 1, 2, 3

# frame (H, W) -> last frame row that construction (c) aims at.  (90, 16384) has only rows 85 .. 89 beyond 4 MB, and a tap
# whose first row is the frame's last is a BORDER entry, not a FAR one: there (c) stays on rows <= H - 3.
LARGE_FRAMES = {(1100, 1280): 1099, (90, 16384): 87, (16384, 90): 16383}
PANO_SHAPES = [(24, 130), (32, 70)]
BAND_ROWS = (2, 3)             # panorama rows of view 0 that hold construction (b)
BOUNDARY_COLS = slice(4, 12)   # columns of BAND_ROWS[0] that hold BOUNDARY_PIXELS


def pixel_targets(rng, pix, W):
    """Map coordinates whose first tap (ix, iy) is pixel index `pix`, with random 1/32 fractions (exact in float32)."""
    pix = np.asarray(pix, dtype=np.int64)
    fx, fy = rng.integers(0, 32, pix.shape), rng.integers(0, 32, pix.shape)
    return (pix % W + fx / 32.0).astype(np.float32), (pix // W + fy / 32.0).astype(np.float32)


def last_pixel_taps(H, W):
    """(d): the frame's last pixels as taps -- tap rows that end within the last 8 bytes of the frame, the last fast-shaped
    position, positions past the right / lower border, and one without any valid tap."""
    return np.array([(W - 1, H - 1), (W - 1.5, H - 1.5), (W - 4, H - 1.25), (W - 3, H - 2), (W - 2.6875, H - 2),
                     (W - 3, H - 2.96875), (W - 1, H - 2.5), (W - 2, H - 1), (0, H - 1), (-0.5, H - 1.5),
                     (W - 0.5, H - 0.5), (W - 1, H + 2.5), (W + 3.9, H - 1)], dtype=np.float32)


def uniform_maps(rng, H, W, pshape, nan_share=0.01):
    """(a): both views uniform over [-6, W + 6) x [-6, H + 6), some NaN."""
    rows, cols = pshape
    mx = rng.uniform(-6, W + 6, (2, rows, cols)).astype(np.float32)
    my = rng.uniform(-6, H + 6, (2, rows, cols)).astype(np.float32)
    mx[rng.random(mx.shape) < nan_share] = np.nan
    my[rng.random(my.shape) < nan_share] = np.nan
    return mx, my


def large_frame_maps(rng, H, W, pshape):
    """Maps (a) - (d) for a frame larger than 4 MB -> map_x, map_y [2, rows, cols] float32."""
    rows, cols = pshape
    assert H * W > LAST_FAST_PIXEL + 5 + 3 * W and rows > BAND_ROWS[1] + 1 and cols >= 16
    mx, my = uniform_maps(rng, H, W, pshape)
    # (c) view 1, ~40 % of the pixels: first taps uniform over the pixel indices beyond 4 MB
    sel = rng.random((rows, cols)) < 0.4
    c_hi = (LARGE_FRAMES.get((H, W), H - 1) + 1) * W
    mx[1][sel], my[1][sel] = pixel_targets(rng, rng.integers(LAST_FAST_PIXEL, c_hi, int(sel.sum())), W)
    # (b) view 0, two rows: a band of +- 3 frame rows around the last fast pixel, the eight pixels around it explicitly
    for r in BAND_ROWS:
        pix = np.clip(LAST_FAST_PIXEL + rng.integers(-3 * W, 3 * W, cols), 0, H * W - 1)
        mx[0, r], my[0, r] = pixel_targets(rng, pix, W)
    mx[0, BAND_ROWS[0], BOUNDARY_COLS], my[0, BAND_ROWS[0], BOUNDARY_COLS] = pixel_targets(rng, BOUNDARY_PIXELS, W)
    # (d) both views: the frame's last pixels, at the start of panorama row 1 and at the very end of the last row
    taps = last_pixel_taps(H, W)
    n = len(taps)
    for v in range(2):
        mx[v, 1, :n], my[v, 1, :n] = taps[:, 0], taps[:, 1]
        mx[v, rows - 1, cols - n:], my[v, rows - 1, cols - n:] = taps[::-1, 0], taps[::-1, 1]
    return mx, my


def masks_for(rng, H, W, density=0.8):
    """(e): [2, H, W] u8 masks at ~80 % density; the pixels the explicit cases name stay unmasked."""
    masks = (rng.random((2, H, W)) < density).astype(np.uint8) * 255
    masks[:, H - 1, W - 1] = 255
    if H * W > BOUNDARY_PIXELS[-1]:
        masks.reshape(2, -1)[:, BOUNDARY_PIXELS] = 255
    return masks


def classify(map_x, map_y, mask, H, W):
    """The table of one view restated in numpy: map_x, map_y [rows, cols] f32, mask [H, W] u8 or None ->
    dict(kind, ix, iy, fx, fy, valid, off0, x, y) with x, y the expected uint32 words of every entry."""
    mx, my = np.asarray(map_x, np.float32), np.asarray(map_y, np.float32)
    with np.errstate(invalid="ignore"):
        inside = (mx == mx) & (my == my) & (mx > np.float32(-4)) & (mx < np.float32(W) + np.float32(4)) & \
            (my > np.float32(-4)) & (my < np.float32(H) + np.float32(4))
    sx = np.rint(np.where(inside, mx, 0) * np.float32(32)).astype(np.int64)      # ties to even, like __float2int_rn
    sy = np.rint(np.where(inside, my, 0) * np.float32(32)).astype(np.int64)
    ix, iy, fx, fy = sx >> 5, sy >> 5, sx & 31, sy & 31
    valid = np.zeros(mx.shape, np.int64)
    for t in range(4):
        x, y = ix + (t & 1), iy + (t >> 1)
        ok = inside & (x >= 0) & (x < W) & (y >= 0) & (y < H)
        if mask is not None:
            ok &= mask[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)] != 0
        valid |= ok.astype(np.int64) << t
    off0 = 3 * (iy * W + ix)
    inner = (off0 >= 0) & (off0 + 3 * W + 8 <= 3 * H * W)          # both 8-byte row loads lie inside the frame
    kind = np.where(valid == 0, ZERO, np.where(inner, np.where(off0 <= TAB_OFF_MASK, FAST, FAR), BORDER))
    w = [np.where((valid >> t) & 1, (fx if t & 1 else 32 - fx) * (fy if t >> 1 else 32 - fy), 0) for t in range(4)]
    fast_x, fast_y = off0 | (w[3] << 22), w[0] | (w[1] << 11) | (w[2] << 21)
    edge_x, edge_y = ((iy & 0xFFFF) << 16) | (ix & 0xFFFF), fx | (fy << 5) | (valid << 10) | TAB_EDGE
    x = np.where(kind == ZERO, 0, np.where(kind == FAST, fast_x, edge_x)).astype(np.uint32)
    y = np.where(kind == ZERO, 0, np.where(kind == FAST, fast_y, edge_y)).astype(np.uint32)
    return dict(kind=kind, ix=ix, iy=iy, fx=fx, fy=fy, valid=valid, off0=off0, x=x, y=y)
