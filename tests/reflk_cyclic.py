"""The CYCLIC form of the pyramidal Lucas-Kanade rule (sosvo_gray_pyramid_cyclic, sosvo_track_lk with
SOSVO_LK_CYCLIC_COLUMNS, include/sosvo.h) restated over tests/reflk.py: column W of a panorama is column
0 again.  Rows, row ranges, sums and floating-point steps are reflk's; only the column index and the x component of a
position change.  Plain Python integers and floats, the CPU reference the device is compared with bit for bit; and the
periodic texture both are measured on."""
import math

import numpy as np

import reflk
from reflk import K5, _note, cut_rows, next_rows

X_LIMIT = float(1 << 40)          # |32 x + 0.5| at and beyond it is "outside", as a column off the image is today


def level_sizes(rows, cols, levels):
    """reflk.level_sizes for a width that is a multiple of 2^(levels - 1): level l has exactly cols >> l columns."""
    if levels < 1 or cols < 1 or cols % (1 << (levels - 1)):
        raise ValueError("cyclic columns need a width that is a multiple of 2^(levels - 1), got %d with %d levels" % (cols, levels))
    return reflk.level_sizes(rows, cols, levels)


def pyr_down(img, r0, r1, out=None):
    """reflk.pyr_down with the column index (2 x + j) mod cols in place of the clamp; cols even."""
    rows, cols = img.shape
    if cols % 2:
        raise ValueError("a cyclic level needs an even width, got %d" % cols)
    ro, co = (rows + 1) // 2, cols // 2
    o0, o1 = next_rows(r0, r1, ro)
    res = np.zeros((ro, co), np.uint8) if out is None else out
    src = img.astype(np.int64)
    xs = [np.mod(2 * np.arange(co) + j, cols) for j in range(-2, 3)]
    for y in range(o0, o1):
        acc = np.zeros(co, np.int64)
        for i in range(-2, 3):
            line = src[min(max(2 * y + i, r0), r1 - 1)]
            acc += K5[i + 2] * sum(K5[j] * line[xs[j]] for j in range(5))
        res[y] = ((acc + 128) >> 8).astype(np.uint8)
    return res, (o0, o1)


def pyramid(img, levels, row_range=None, fill=None):
    """reflk.pyramid, cyclic in the columns."""
    level_sizes(img.shape[0], img.shape[1], levels)
    r = cut_rows(img.shape[0], row_range)
    lv, rr = [img], [r]
    for l in range(1, levels):
        nxt, r = pyr_down(lv[-1], r[0], r[1], None if fill is None else fill[l - 1].copy())
        lv.append(nxt)
        rr.append(r)
    return lv, rr


def pyramid_set(gray, levels, row_range=None):
    nimg = gray.shape[0]
    per = max(1, nimg // 2)
    return [pyramid(gray[i], levels, None if row_range is None else row_range[i // per]) for i in range(nimg)]


def _grid(cx, cy, cols, r0, r1):
    """-> (tqx, tqy, inside): tqx reduced to [0, 32 cols); "outside" is a matter of the rows (and of a value that is no
    position at all: non-finite, or |32 x + 0.5| >= 2^40)."""
    vx, vy = 32.0 * cx + 0.5, 32.0 * cy + 0.5
    if not (math.isfinite(vx) and math.isfinite(vy)) or abs(vx) >= X_LIMIT:
        return 0, 0, False
    tqx, tqy = math.floor(vx) % (32 * cols), math.floor(vy)
    return tqx, tqy, 32 * r0 <= tqy <= 32 * (r1 - 1)


def _samples(img, r0, r1, tqx, tqy, reach):
    rows, cols = img.shape
    bx, fx, by, fy = tqx >> 5, tqx & 31, tqy >> 5, tqy & 31
    x = bx + np.arange(-reach, reach + 1)
    y = by + np.arange(-reach, reach + 1)
    xa, xb = np.mod(x, cols), np.mod(x + 1, cols)
    ya, yb = np.clip(y, r0, r1 - 1), np.clip(y + 1, r0, r1 - 1)
    im = img.astype(np.int64)
    p00, p01 = im[np.ix_(ya, xa)], im[np.ix_(ya, xb)]
    p10, p11 = im[np.ix_(yb, xa)], im[np.ix_(yb, xb)]
    return (32 - fy) * ((32 - fx) * p00 + fx * p01) + fy * ((32 - fx) * p10 + fx * p11)


def wrap_x(gx, W):
    """The x a result is written with: g.x - W floor(g.x / W) in double, as float32; W itself (a value that rounds up to the
    period) is written as 0."""
    w = np.float32(gx - float(W) * float(math.floor(gx / float(W))))
    return np.float32(0.0) if w == np.float32(W) else w


def cyclic_distance(a, b, W):
    d = abs(float(a) - float(b))
    return min(d, float(W) - d)


def check_window(cols, levels, half):
    """The template of 2 half + 3 columns fits one period of the top level: no column is sampled twice in one row."""
    if (cols >> (levels - 1)) < 2 * half + 3:
        raise ValueError("the top level's %d columns are fewer than the template's %d" % (cols >> (levels - 1), 2 * half + 3))


def track(prev, nxt, x0, y0, half, max_iter=30, eps=0.01, min_eig=1e-4, guess=None, stats=None):
    """reflk.track with the five changes of the cyclic rule (the numbers are those of the header)."""
    L = len(prev[0])
    N = (2 * half + 1) ** 2
    W = prev[0][0].shape[1]
    level_sizes(prev[0][0].shape[0], W, L)
    check_window(W, L, half)
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
    lost = lambda: (wrap_x(cx, W), np.float32(cy), 0, np.float32(0.0))  # noqa: E731   (4.)
    for l in range(L - 1, -1, -1):
        ia, (ra0, ra1) = prev[0][l], prev[1][l]
        ib, (rb0, rb1) = nxt[0][l], nxt[1][l]
        cols = ia.shape[1]
        scale = 1.0 / float(1 << l)
        tqx, tqy, inside = _grid(px * scale, py * scale, cols, ra0, ra1)          # (1.)
        run = inside
        if not inside and l == 0:
            return lost()
        if run:
            T = _samples(ia, ra0, ra1, tqx, tqy, half + 1)                        # (2.)
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
                cx, cy = qx * 0.03125 + dx, qy * 0.03125 + dy                      # (3.: qx is the wrapped one)
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
            return wrap_x(cx, W), np.float32(cy), 1, np.float32(float(s) / (1024.0 * float(N)))


def track_problems(pyrs, prev_img, next_img, prev_pts, n, half, max_iter=30, eps=0.01, min_eig=1e-4, next_pts=None, fb_max=None,
                   out=None):
    """reflk.track_problems; the x part of |back - prev|^2 is the cyclic distance (5.)."""
    nprob, cap = prev_pts.shape[:2]
    W = pyrs[0][0][0].shape[1]
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
                    ddx, ddy = cyclic_distance(bx, prev_pts[p, k, 0], W), float(by) - float(prev_pts[p, k, 1])
                    if not sb or not (ddx * ddx + ddy * ddy <= fb_max * fb_max):
                        st[p, k] = 0
    return (nx, st, er) if fb_max is None else (nx, st, er, bk)


# ---- the |du| gate -------------------------------------------------------------------------------------------------------------
def du_gate(u_a, u_b, max_du, W):
    """The cyclic frame-to-frame gate on float32 columns: d = |a - b| in double; a pair passes iff d <= max_du or
    W - d <= max_du.  The switch is the plain gate's: max_du <= 0 disables it.  Exact: no tolerance anywhere."""
    d = np.abs(np.asarray(u_a, np.float32).astype(np.float64) - np.asarray(u_b, np.float32).astype(np.float64))
    if not max_du > 0:
        return np.ones(d.shape, bool)
    return (d <= max_du) | (float(W) - d <= max_du)


def du_gate_plain(u_a, u_b, max_du):
    d = np.abs(np.asarray(u_a, np.float32).astype(np.float64) - np.asarray(u_b, np.float32).astype(np.float64))
    return np.ones(d.shape, bool) if not max_du > 0 else d <= max_du


# ---- the periodic shifted-texture scene ------------------------------------------------------------------------------------------
def texture(seed, rows, cols, shift=(0.0, 0.0), waves=40, lo=3.0, hi=40.0):
    """reflk.texture with every wave's x wavenumber snapped to whole cycles across the width: the image is one period of a
    pattern that repeats every `cols` columns, and texture(seed, ..., shift) is texture(seed, ...) moved by exactly `shift`
    AROUND the cylinder.  (The random draws are reflk.texture's, in its order.)"""
    rng = np.random.default_rng(seed)
    lam = rng.uniform(lo, hi, waves)
    th = rng.uniform(0.0, 2.0 * np.pi, waves)
    ph = rng.uniform(0.0, 2.0 * np.pi, waves)
    amp = rng.uniform(0.5, 1.0, waves) * (lam / hi) ** 0.5
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    x, y = x - shift[0], y - shift[1]
    img = np.zeros((rows, cols))
    for k in range(waves):
        w = 2.0 * np.pi / lam[k]
        wx = 2.0 * np.pi * np.rint(w * np.cos(th[k]) * cols / (2.0 * np.pi)) / cols
        img += amp[k] * np.sin(wx * x + w * np.sin(th[k]) * y + ph[k])
    img = 127.5 + img * (100.0 / (np.sqrt((amp ** 2).sum() / 2.0) * 3.0))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def seam_grid(rows=96, cols=128):
    """The issue's 256 grid points: x from 0 in steps of 4 (all around), y from 16 to 72 in steps of 8, as [n, 2] float32."""
    ys, xs = np.mgrid[16:73:8, 0:cols:4]
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
