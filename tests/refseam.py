"""The seam-free front end's rule (include/sosvo.h) in numpy, and the fixture its tests share.

The seam-free front end of a panorama P of W columns and mask bits M is BY DEFINITION the plain front end run on pad(P) and
pad0(M), followed by unpad of every keypoint's x.  So the CPU reference is the oracle's plain stages on host-padded arrays
(front_end below), and the GPU reference is the project's plain entry points on host-padded maps and masks."""
import zlib

import numpy as np

HALO = 40
FIXTURE_CRC32 = 1721023341
# the fixture's settings: median 11, GFT quality 0.01, distance 5, 1000 corners, candidate cap 4096, edge 31
MEDIAN, QUALITY, MIN_DISTANCE, MAX_CORNERS, CAND_CAP, EDGE = 11, 0.01, 5.0, 1000, 4096, 31
ROW0, ROW1, MASK_W = 8, 88, 64      # mask k covers the columns [64 k, 64 k + 64) of the rows 8 to 87


def pad(a, axis=1, halo=HALO):
    """pad(P)[:, c'] = P[:, (c' - halo) mod W] for c' in [0, W + 2 halo) along `axis`."""
    w = a.shape[axis]
    return np.take(a, (np.arange(w + 2 * halo) - halo) % w, axis=axis)


def pad0(bits, axis=-1, halo=HALO):
    """The mask bits in the columns [halo, halo + W) and 0 in the halo."""
    width = [(0, 0)] * bits.ndim
    width[axis] = (halo, halo)
    return np.pad(bits, width)


def unpad(x, period, halo=HALO):
    """The unpad rule on float32 x values: x - halo, + period if negative, - period if >= period, `period` itself is 0."""
    w = np.float32(period)
    x = np.asarray(x, np.float32) - np.float32(halo)
    x = np.where(x < 0, x + w, x).astype(np.float32)
    x = np.where(x >= w, x - w, x).astype(np.float32)
    return np.where(x == w, np.float32(0), x).astype(np.float32)


def texture(seed, R=96, W=256):
    """A panorama that is textured across its seam (the boxes wrap around): uint8 [R, W, 3]."""
    r = np.random.default_rng(seed); img = np.zeros((R, W, 3)); yy, xx = np.mgrid[0:R, 0:W]
    for _ in range(220):
        cx = r.uniform(0, W); cy = r.uniform(0, R); s = r.uniform(3, 9); a = r.uniform(-90, 90, 3)
        dx = np.minimum(np.abs(xx - cx), W - np.abs(xx - cx)); dy = yy - cy
        img += ((dx < s) & (np.abs(dy) < s * r.uniform(.5, 1.5)))[..., None] * a
    img -= img.min(); return (img / img.max() * 255).astype(np.uint8)


def fixture():
    """-> (P uint8 [96, 256, 3] = texture(3), mask bits uint32 [96, 256] of the four masks)."""
    P = texture(3)
    assert zlib.crc32(P.tobytes()) == FIXTURE_CRC32, "the fixture's bytes changed (numpy's generator?)"
    return P, sector_masks(P.shape[0], P.shape[1])


def sector_masks(rows, cols, shift=0):
    """Mask k = the columns [64 k + shift, 64 k + 64 + shift) mod cols of the rows 8 to 87, as bit k."""
    bits = np.zeros((rows, cols), np.uint32)
    for k in range(cols // MASK_W):
        bits[ROW0:ROW1, (np.arange(MASK_W * k, MASK_W * (k + 1)) + shift) % cols] |= np.uint32(1 << k)
    return bits


def front_end(P, bits, nmask=4, seam_free=False):
    """The CPU oracle's front end on a panorama (median_gray, min_eigen, gft_select, gauss7, orb_describe, the GFT keypoint
    angle of -1 degree) -> per mask (kp [n, 2] float32, desc [n, 32] uint8); seam_free: on pad(P), pad0(bits), then unpad."""
    import oracle
    from vo_single_camera_sos_amd import orb_pattern
    cos_a, sin_a = orb_pattern.angle_cos_sin(orb_pattern.GFT_KEYPOINT_ANGLE)
    if seam_free:
        P, bits = pad(P), pad0(bits)
    gray = oracle.median_gray(P, MEDIAN)
    eig, blurred = oracle.min_eigen(gray), oracle.gauss7(gray)
    out = []
    for m in range(nmask):
        kp, _ = oracle.gft_select(eig, bits, m, QUALITY, MIN_DISTANCE, MAX_CORNERS, cand_cap=CAND_CAP)
        desc, kept = oracle.orb_describe(blurred, kp, cos_a, sin_a, orb_pattern.orb_pattern(), EDGE)
        kp = kp[kept].copy()
        if seam_free:
            kp[:, 0] = unpad(kp[:, 0], bits.shape[1] - 2 * HALO)
        out.append((kp, desc))
    return out
