"""The pyramidal Lucas-Kanade rule of sosvo_gray_pyramid / sosvo_track_lk (include/sosvo.h) in plain Python integers and floats,
line by line: the CPU reference the device stages are compared with bit for bit, and the shifted-texture scene both are
measured on.  numpy int64 arrays stand for the integers of one window (still exact: every sum stays below 2^53)."""
import math

import numpy as np

K5 = (1, 4, 6, 4, 1)


def cut_rows(rows, row_range):
    """Level 0: row_range cut to the image, at least one row; None = all rows."""
    if row_range is None:
        return 0, rows
    r0 = min(max(int(row_range[0]), 0), rows - 1)
    return r0, min(max(int(row_range[1]), r0 + 1), rows)


def next_rows(r0, r1, rows_next):
    """The row range of level l + 1 (of rows_next rows) from that of level l; cut to the level, as at level 0."""
    a = min((r0 + 1) // 2, rows_next - 1)
    return a, min(max((r1 + 1) // 2, a + 1), rows_next)


def level_sizes(rows, cols, levels):
    out = [(rows, cols)]
    for _ in range(levels - 1):
        rows, cols = (rows + 1) // 2, (cols + 1) // 2
        out.append((rows, cols))
    return out


def pyr_down(img, r0, r1, out=None):
    """One level: img [rows, cols] u8 with valid rows [r0, r1) -> (level [ (rows+1)//2, (cols+1)//2 ] u8, its range).  Rows of
    `out` (what the buffer held, default zeros) outside the new range are left as they are."""
    rows, cols = img.shape
    ro, co = (rows + 1) // 2, (cols + 1) // 2
    o0, o1 = next_rows(r0, r1, ro)
    res = np.zeros((ro, co), np.uint8) if out is None else out
    src = img.astype(np.int64)
    xs = [np.clip(2 * np.arange(co) + j, 0, cols - 1) for j in range(-2, 3)]
    for y in range(o0, o1):
        acc = np.zeros(co, np.int64)
        for i in range(-2, 3):
            line = src[min(max(2 * y + i, r0), r1 - 1)]
            acc += K5[i + 2] * sum(K5[j] * line[xs[j]] for j in range(5))
        res[y] = ((acc + 128) >> 8).astype(np.uint8)
    return res, (o0, o1)


def pyramid(img, levels, row_range=None, fill=None):
    """-> (list of levels (level 0 = img itself), list of row ranges).  fill: what the rows outside the ranges hold (a list of
    arrays per level >= 1, e.g. what a device buffer held before the call); default zeros."""
    r = cut_rows(img.shape[0], row_range)
    lv, rr = [img], [r]
    for l in range(1, levels):
        nxt, r = pyr_down(lv[-1], r[0], r[1], None if fill is None else fill[l - 1].copy())
        lv.append(nxt)
        rr.append(r)
    return lv, rr


def pyramid_set(gray, levels, row_range=None):
    """gray [nimg, rows, cols] u8, row_range [2, 2] (view-major) or None -> per image (levels, ranges)."""
    nimg = gray.shape[0]
    per = max(1, nimg // 2)
    return [pyramid(gray[i], levels, None if row_range is None else row_range[i // per]) for i in range(nimg)]


def _grid(cx, cy, cols, r0, r1):
    """-> (tqx, tqy, inside): the position on the 1/32-px grid; NaN is outside."""
    vx, vy = 32.0 * cx + 0.5, 32.0 * cy + 0.5
    if not (math.isfinite(vx) and math.isfinite(vy)):
        return 0, 0, False
    tqx, tqy = math.floor(vx), math.floor(vy)
    return tqx, tqy, (0 <= tqx <= 32 * (cols - 1) and 32 * r0 <= tqy <= 32 * (r1 - 1))


def _samples(img, r0, r1, tqx, tqy, reach):
    """The (2 reach + 1)^2 integer bilinear samples around the grid position, as an int64 array."""
    rows, cols = img.shape
    bx, fx, by, fy = tqx >> 5, tqx & 31, tqy >> 5, tqy & 31
    x = bx + np.arange(-reach, reach + 1)
    y = by + np.arange(-reach, reach + 1)
    xa, xb = np.clip(x, 0, cols - 1), np.clip(x + 1, 0, cols - 1)
    ya, yb = np.clip(y, r0, r1 - 1), np.clip(y + 1, r0, r1 - 1)
    im = img.astype(np.int64)
    p00, p01 = im[np.ix_(ya, xa)], im[np.ix_(ya, xb)]
    p10, p11 = im[np.ix_(yb, xa)], im[np.ix_(yb, xb)]
    return (32 - fy) * ((32 - fx) * p00 + fx * p01) + fy * ((32 - fx) * p10 + fx * p11)


def _note(stats, *sums):
    if stats is not None:
        stats["max_sum"] = max(stats.get("max_sum", 0), *(abs(int(v)) for v in sums))


def track(prev, nxt, x0, y0, half, max_iter=30, eps=0.01, min_eig=1e-4, guess=None, stats=None):
    """prev, nxt: (levels, ranges) of the two images (pyramid()); (x0, y0): the start as float32 values; guess: the starting
    guess (float32 values) of the initial-flow flag -> (x, y as float32, status, err as float32).
    stats (a dict): receives max_sum (the largest |sum| seen) and iterations (per level, coarse to fine)."""
    L = len(prev[0])
    N = (2 * half + 1) ** 2
    if stats is not None:
        stats.setdefault("max_sum", 0)
        stats["iterations"] = []
    px, py = float(x0), float(y0)
    gx0, gy0 = (px, py) if guess is None else (float(guess[0]), float(guess[1]))
    if not all(math.isfinite(v) for v in (px, py, gx0, gy0)):
        return np.float32(x0), np.float32(y0), 0, np.float32(0.0)
    top = 1.0 / float(1 << (L - 1))
    cx, cy = gx0 * top, gy0 * top
    eps2 = eps * eps
    den = float(N) * 2147483648.0
    lost = lambda: (np.float32(cx), np.float32(cy), 0, np.float32(0.0))  # noqa: E731
    for l in range(L - 1, -1, -1):
        ia, (ra0, ra1) = prev[0][l], prev[1][l]
        ib, (rb0, rb1) = nxt[0][l], nxt[1][l]
        cols = ia.shape[1]
        scale = 1.0 / float(1 << l)
        tqx, tqy, inside = _grid(px * scale, py * scale, cols, ra0, ra1)
        run = inside
        if not inside and l == 0:
            return lost()
        if run:
            T = _samples(ia, ra0, ra1, tqx, tqy, half + 1)
            gx = 3 * (T[:-2, 2:] - T[:-2, :-2]) + 10 * (T[1:-1, 2:] - T[1:-1, :-2]) + 3 * (T[2:, 2:] - T[2:, :-2])
            gy = 3 * (T[2:, :-2] - T[:-2, :-2]) + 10 * (T[2:, 1:-1] - T[:-2, 1:-1]) + 3 * (T[2:, 2:] - T[:-2, 2:])
            Tc = T[1:-1, 1:-1]
            a, b, c = int((gx * gx).sum()), int((gx * gy).sum()), int((gy * gy).sum())
            _note(stats, a, b, c)
            A, B, C = float(a), float(b), float(c)
            det = A * C - B * B
            diff = A - C
            eig = (A + C - math.sqrt(diff * diff + 4.0 * B * B)) / den
            if det == 0.0 or eig < min_eig:
                run = False
                if l == 0:
                    return lost()
        iters = 0
        if run:
            pdx = pdy = 0.0
            for it in range(max_iter):
                qx, qy, inside = _grid(cx, cy, cols, rb0, rb1)
                if not inside:
                    if l == 0:
                        return lost()
                    break
                d = _samples(ib, rb0, rb1, qx, qy, half) - Tc
                s1, s2 = int((d * gx).sum()), int((d * gy).sum())
                _note(stats, s1, s2)
                b1, b2 = float(s1), float(s2)
                dx = -32.0 * (C * b1 - B * b2) / det
                dy = -32.0 * (A * b2 - B * b1) / det
                cx, cy = qx * 0.03125 + dx, qy * 0.03125 + dy
                iters += 1
                if dx * dx + dy * dy <= eps2:
                    break
                if it > 0 and abs(dx + pdx) < 0.01 and abs(dy + pdy) < 0.01:
                    cx -= dx * 0.5
                    cy -= dy * 0.5
                    break
                pdx, pdy = dx, dy
        if stats is not None:
            stats["iterations"].append(iters)
        if l > 0:
            cx *= 2.0
            cy *= 2.0
        else:
            qx, qy, inside = _grid(cx, cy, cols, rb0, rb1)
            if not inside:
                return lost()
            s = int(np.abs(_samples(ib, rb0, rb1, qx, qy, half) - Tc).sum())
            _note(stats, s)
            return np.float32(cx), np.float32(cy), 1, np.float32(float(s) / (1024.0 * float(N)))


def track_problems(pyrs, prev_img, next_img, prev_pts, n, half, max_iter=30, eps=0.01, min_eig=1e-4, next_pts=None, fb_max=None,
                   out=None):
    """The stage on host arrays: pyrs = pyramid_set(); prev_img, next_img [nprob]; prev_pts [nprob, cap, 2] f32; n [nprob];
    next_pts: the guesses of the initial-flow flag or None; out: (next, status, err[, back]) as the buffers held them (rows at
    and beyond n stay) -> (next, status, err) or, with fb_max, (next, status, err, back)."""
    nprob, cap = prev_pts.shape[:2]
    if out is None:
        out = (np.zeros((nprob, cap, 2), np.float32), np.zeros((nprob, cap), np.uint8), np.zeros((nprob, cap), np.float32),
               np.zeros((nprob, cap, 2), np.float32))
    nx, st, er = (np.array(o, copy=True) for o in out[:3])
    bk = np.array(out[3], copy=True) if fb_max is not None else None
    for p in range(nprob):
        a, b = int(prev_img[p]), int(next_img[p])
        if not (0 <= a < len(pyrs) and 0 <= b < len(pyrs)):
            continue
        for k in range(min(int(n[p]), cap)):
            g = None if next_pts is None else next_pts[p, k]
            x, y, s, e = track(pyrs[a], pyrs[b], prev_pts[p, k, 0], prev_pts[p, k, 1], half, max_iter, eps, min_eig, g)
            nx[p, k], st[p, k], er[p, k] = (x, y), s, e
            if fb_max is not None:
                bk[p, k] = (x, y)
                if s:
                    bx, by, sb, _ = track(pyrs[b], pyrs[a], x, y, half, max_iter, eps, min_eig)
                    bk[p, k] = (bx, by)
                    ddx, ddy = float(bx) - float(prev_pts[p, k, 0]), float(by) - float(prev_pts[p, k, 1])
                    if not sb or not (ddx * ddx + ddy * ddy <= fb_max * fb_max):
                        st[p, k] = 0
    return (nx, st, er) if fb_max is None else (nx, st, er, bk)


# ---- the shifted-texture scene ---------------------------------------------------------------------------------------------
def texture(seed, rows, cols, shift=(0.0, 0.0), waves=40, lo=3.0, hi=40.0):
    """A u8 image of `waves` random sinusoids (wavelengths lo .. hi px) evaluated analytically at (x - shift_x, y - shift_y):
    texture(seed, ..., shift=(dx, dy)) is texture(seed, ...) moved by exactly (dx, dy) -- a point at p in the first is at
    p + (dx, dy) in the second -- up to the u8 quantisation."""
    rng = np.random.default_rng(seed)
    lam = rng.uniform(lo, hi, waves)
    th = rng.uniform(0.0, 2.0 * np.pi, waves)
    ph = rng.uniform(0.0, 2.0 * np.pi, waves)
    amp = rng.uniform(0.5, 1.0, waves) * (lam / hi) ** 0.5          # (long waves carry more: what a coarse level still sees)
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    x, y = x - shift[0], y - shift[1]
    img = np.zeros((rows, cols))
    for k in range(waves):
        w = 2.0 * np.pi / lam[k]
        img += amp[k] * np.sin(w * (np.cos(th[k]) * x + np.sin(th[k]) * y) + ph[k])
    img = 127.5 + img * (100.0 / (np.sqrt((amp ** 2).sum() / 2.0) * 3.0))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def grid_points(rows, cols, margin, step):
    """Points on a regular grid `margin` px inside the image, as [n, 2] float32 (x, y)."""
    ys, xs = np.mgrid[margin:rows - margin:step, margin:cols - margin:step]
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
