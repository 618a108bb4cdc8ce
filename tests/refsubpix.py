"""The sub-pixel refinement rule of sosvo_refine_subpix (include/sosvo.h) in plain Python integers and floats, line by line:
the CPU reference the device stage is compared with bit for bit, and the rendered-corner scene both are measured on.  The
weight table comes from the library (sosvo_subpix_weights), so a libm difference in the last bit cannot split the two."""
import math

import numpy as np

from vo_single_camera_sos_amd import _lib

MAX_ITER, EPS = 10, 0.01        # what the one-call and sequence entry points run the stage with


def weights(half):
    return _lib.subpix_weights(half)


def cut_rows(rows, row_range):
    """The rows [first, last + 1) samples are clamped to: row_range cut to the image, at least one row; None = all rows."""
    if row_range is None:
        return 0, rows
    r0 = min(max(int(row_range[0]), 0), rows - 1)
    return r0, min(max(int(row_range[1]), r0 + 1), rows)


def refine(gray, x0, y0, half, max_iter=MAX_ITER, eps=EPS, row_range=None, w=None, stats=None):
    """gray: 2-D uint8 array (or nested lists); (x0, y0): the position as given (float32 values) -> (x, y) as float32 values.
    stats (a dict): receives iterations, reverted, max_sum (the largest |sum| seen)."""
    rows, cols = len(gray), len(gray[0])
    w = weights(half) if w is None else w
    r0, r1 = cut_rows(rows, row_range)
    if stats is not None:
        stats.update(iterations=0, reverted=False, max_sum=0)
    c0x, c0y = float(x0), float(y0)
    if not (math.isfinite(c0x) and math.isfinite(c0y)):
        return x0, y0
    cx, cy = c0x, c0y
    side3 = 2 * half + 3
    eps2 = eps * eps
    for _ in range(max_iter):
        xq, yq = math.floor(32.0 * cx + 0.5), math.floor(32.0 * cy + 0.5)
        ix, fx, iy, fy = xq >> 5, xq & 31, yq >> 5, yq & 31
        S = [[0] * side3 for _ in range(side3)]
        for i in range(side3):
            y = iy + i - half - 1
            ya, yb = min(max(y, r0), r1 - 1), min(max(y + 1, r0), r1 - 1)
            for j in range(side3):
                x = ix + j - half - 1
                xa, xb = min(max(x, 0), cols - 1), min(max(x + 1, 0), cols - 1)
                p00, p01, p10, p11 = int(gray[ya][xa]), int(gray[ya][xb]), int(gray[yb][xa]), int(gray[yb][xb])
                S[i][j] = (32 - fy) * ((32 - fx) * p00 + fx * p01) + fy * ((32 - fx) * p10 + fx * p11)
        a = b = c2 = b1 = b2 = 0
        for i in range(2 * half + 1):
            for j in range(2 * half + 1):
                gx = S[i + 1][j + 2] - S[i + 1][j]
                gy = S[i + 2][j + 1] - S[i][j + 1]
                m = (w[i] * w[j]) >> 8
                px, py = j - half, i - half
                a += gx * gx * m
                b += gx * gy * m
                c2 += gy * gy * m
                b1 += gx * gx * m * px + gx * gy * m * py
                b2 += gx * gy * m * px + gy * gy * m * py
        if stats is not None:
            stats["max_sum"] = max(stats["max_sum"], *(abs(v) for v in (a, b, c2, b1, b2)))
        A, B, C, B1, B2 = float(a), float(b), float(c2), float(b1), float(b2)
        det = A * C - B * B
        if det == 0.0:
            break
        if stats is not None:
            stats["iterations"] += 1
        nx = xq / 32 + (C * B1 - B * B2) / det
        ny = yq / 32 + (A * B2 - B * B1) / det
        dx, dy = nx - cx, ny - cy
        err = dx * dx + dy * dy
        if not (abs(nx - c0x) <= half and abs(ny - c0y) <= half):
            if stats is not None:
                stats["reverted"] = True
            cx, cy = c0x, c0y
            break
        cx, cy = nx, ny
        if err <= eps2:
            break
    return np.float32(cx), np.float32(cy)


def refine_problems(gray, nmask, kp, n, half, max_iter=MAX_ITER, eps=EPS, row_range=None):
    """The stage on host arrays: gray [nimg, rows, cols] u8, kp [nimg * nmask, cap, 2] f32, n [nimg * nmask]; row_range
    [2, 2] (view-major: image i belongs to view i // (nimg // 2)) or None -> the refined copy of kp."""
    out = np.array(kp, dtype=np.float32, copy=True)
    nimg, w = gray.shape[0], weights(half)
    images = [g.tolist() for g in gray]
    for p in range(out.shape[0]):
        image = p // nmask
        rr = None if row_range is None else row_range[image // max(1, nimg // 2)]
        for k in range(min(int(n[p]), out.shape[1])):
            out[p, k] = refine(images[image], out[p, k, 0], out[p, k, 1], half, max_iter, eps, rr, w)
    return out


# ---- the rendered X-corner scene -------------------------------------------------------------------------------------------
def _blur14641(img):
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    pad = np.pad(img, 2, mode="edge")
    rows = sum(k[t] * pad[t:t + img.shape[0], 2:-2] for t in range(5))
    pad = np.pad(rows, ((0, 0), (2, 2)), mode="edge")
    return sum(k[t] * pad[:, t:t + img.shape[1]] for t in range(5))


def render_corner(seed, size=64, centre=31.0, lo=40.0, hi=200.0, sigma=2.0, supersample=8):
    """-> (u8 image [size, size], true corner (x, y)): an X-corner at centre + U(-.5, .5) in both axes, rotated by U(0, pi / 2),
    levels lo / hi, supersampled 8 x 8, blurred with the separable [1 4 6 4 1] / 16 kernel (two passes: along the columns, then
    along the rows; this reading reproduces the iteration counts and errors of the rule's prototype), Gaussian noise, rounded."""
    rng = np.random.default_rng(seed)
    tx, ty = centre + rng.uniform(-0.5, 0.5), centre + rng.uniform(-0.5, 0.5)
    th = rng.uniform(0.0, np.pi / 2.0)
    s = supersample
    g = (np.arange(size * s) + 0.5) / s - 0.5          # sub-sample centres in pixel coordinates (pixel k covers k +- .5)
    X, Y = np.meshgrid(g - tx, g - ty)
    u, v = np.cos(th) * X + np.sin(th) * Y, -np.sin(th) * X + np.cos(th) * Y
    fine = np.where(u * v > 0, hi, lo)
    img = fine.reshape(size, s, size, s).mean(axis=(1, 3))
    img = _blur14641(img)
    img = img + rng.normal(0.0, sigma, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), (tx, ty)
