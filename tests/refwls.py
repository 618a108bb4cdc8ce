"""The WLS disparity filter of include/sosvo_dense_filter.h (sosvo_dense_confidence, sosvo_dense_wls),
stated in numpy stage by stage for one frame: confidence -> right-hand sides -> line solves (rows, then columns, per
iteration) -> the filtered map.  Every floating-point operation below is one IEEE double operation, written in the order the
header gives, so that the device reproduces N, D and d16 bit for bit (tests/test_gpu_wls.py)."""
import math

import numpy as np


def weight_table(sigma):
    """The 256 affinities exp(-k / sigma), k = the absolute gray difference of two neighbours (what WlsOptions.weight_table
    returns)."""
    return np.array([math.exp(-k / sigma) for k in range(256)], dtype=np.float64)


def iteration_lambdas(lam, iters):
    """lam_t for t = 0 .. iters - 1: ((1.5 lambda) 4^(iters-1-t)) / (4^iters - 1)."""
    return [((1.5 * float(lam)) * float(4 ** (iters - 1 - t))) / float(4 ** iters - 1) for t in range(iters)]


def confidence(d16, radius=3, roll_ppm=1000, cyclic=False):
    """d16 [rows, cols] i16 -> u8.  Over the valid taps of the (2 radius + 1)^2 window (rows outside do not exist; columns
    outside do not exist, or wrap): m, s1, s2 in int64, V = (m s2 - s1^2) // m^2, conf = max(0, 255 - (255 roll_ppm V) // 10^6)."""
    d = np.asarray(d16).astype(np.int64)
    rows, cols = d.shape
    valid = d >= 0
    m, s1, s2 = (np.zeros((rows, cols), dtype=np.int64) for _ in range(3))
    cc = np.arange(cols)
    for dy in range(-radius, radius + 1):
        r0, r1 = max(0, -dy), min(rows, rows - dy)       # the rows r with 0 <= r + dy < rows
        if r0 >= r1:
            continue
        for dx in range(-radius, radius + 1):
            ci = cc + dx
            inside = np.ones(cols, dtype=bool) if cyclic else (ci >= 0) & (ci < cols)
            ci = ci % cols
            tap = d[r0 + dy:r1 + dy][:, ci]
            ok = valid[r0 + dy:r1 + dy][:, ci] & inside[None, :]
            m[r0:r1] += ok
            s1[r0:r1] += np.where(ok, tap, 0)
            s2[r0:r1] += np.where(ok, tap * tap, 0)
    mm = np.maximum(m, 1)
    V = (m * s2 - s1 * s1) // (mm * mm)
    conf = np.maximum(0, 255 - (255 * int(roll_ppm) * V) // 1000000)
    return np.where(valid, conf, 0).astype(np.uint8)


def line_weights(g, lam_t, weights):
    """g [..., n] u8 -> (wl, wr) [..., n]: lam_t * weights[|g_i - g_(i-1)|] (0 at i = 0) and lam_t * weights[|g_(i+1) - g_i|]
    (0 at i = n - 1)."""
    g = np.asarray(g).astype(np.int64)
    w = lam_t * np.asarray(weights, dtype=np.float64)[np.abs(np.diff(g, axis=-1))]
    zero = np.zeros(g.shape[:-1] + (1,))
    return np.concatenate([zero, w], axis=-1), np.concatenate([w, zero], axis=-1)


def _sweep(a, b, c, fs):
    """The forward and the backward sweep over the last axis, one reciprocal per step shared by the right-hand sides fs."""
    n = b.shape[-1]
    cp = np.empty_like(b)
    fp = [np.empty_like(b) for _ in fs]
    r = 1.0 / b[..., 0]
    cp[..., 0] = c[..., 0] * r
    for k, f in enumerate(fs):
        fp[k][..., 0] = f[..., 0] * r
    for i in range(1, n):
        r = 1.0 / (b[..., i] - a[..., i] * cp[..., i - 1])
        cp[..., i] = c[..., i] * r
        for k, f in enumerate(fs):
            fp[k][..., i] = (f[..., i] - a[..., i] * fp[k][..., i - 1]) * r
    us = [np.empty_like(b) for _ in fs]
    for k in range(len(fs)):
        us[k][..., n - 1] = fp[k][..., n - 1]
        for i in range(n - 2, -1, -1):
            us[k][..., i] = fp[k][..., i] - cp[..., i] * us[k][..., i + 1]
    return us


def solve_lines(fs, g, lam_t, weights, cyclic=False):
    """(I + lam_t A) u = f along the last axis for every right-hand side of the list fs ([..., n] f64 each), A the weighted
    graph Laplacian of the line under the guide g [..., n] u8.  cyclic (and n >= 3): element n - 1 neighbours element 0, by
    Sherman-Morrison with the third right-hand side (gamma, 0, ..., 0, -ws)."""
    g = np.asarray(g)
    n = g.shape[-1]
    fs = [np.asarray(f, dtype=np.float64) for f in fs]
    wl, wr = line_weights(g, lam_t, weights)
    b = (1.0 + wl) + wr
    a, c = -wl, -wr
    if not (cyclic and n >= 3):
        return _sweep(a, b, c, fs)
    gi = g.astype(np.int64)
    ws = lam_t * np.asarray(weights, dtype=np.float64)[np.abs(gi[..., 0] - gi[..., n - 1])]
    b = b.copy()
    b[..., 0] = (1.0 + ws) + wr[..., 0]
    b[..., n - 1] = (1.0 + wl[..., n - 1]) + ws
    gamma = -b[..., 0]
    b[..., 0] = b[..., 0] - gamma
    b[..., n - 1] = b[..., n - 1] - ((-ws) * (-ws)) / gamma
    fz = np.zeros_like(b)
    fz[..., 0] = gamma
    fz[..., n - 1] = -ws
    *ys, z = _sweep(a, b, c, fs + [fz])
    q = (-ws) / gamma
    vz = 1.0 + (z[..., 0] + q * z[..., n - 1])
    out = []
    for y in ys:
        vy = y[..., 0] + q * y[..., n - 1]
        out.append(y - z * (vy / vz)[..., None])
    return out


def line_matrix(g, lam_t, weights, cyclic=False):
    """The matrix I + lam_t A of one line, built entry by entry (the outside truth of the line solves: numpy.linalg.solve)."""
    g = np.asarray(g).astype(np.int64)
    n = g.shape[0]
    w = np.asarray(weights, dtype=np.float64)
    M = np.eye(n)
    pairs = [(i, i + 1) for i in range(n - 1)] + ([(n - 1, 0)] if cyclic and n >= 3 else [])
    for i, j in pairs:
        v = lam_t * w[abs(int(g[i]) - int(g[j]))]
        M[i, i] += v
        M[j, j] += v
        M[i, j] -= v
        M[j, i] -= v
    return M


def wls(d16, guide, conf=None, mask=None, lam=8000.0, weights=None, iters=3, min_weight=2.0 ** -20, cyclic=False):
    """One frame: d16 [rows, cols] i16, guide u8, conf u8 or None (255 on every valid pixel), mask u8 or None ->
    (d16_out i16, planes [2, rows, cols] f64: the final numerator and denominator)."""
    d = np.asarray(d16).astype(np.int64)
    guide = np.asarray(guide, dtype=np.uint8)
    weights = weight_table(1.0) if weights is None else np.asarray(weights, dtype=np.float64)
    w = np.where(d >= 0, 255 if conf is None else np.asarray(conf).astype(np.int64), 0)
    N, D = (w * d).astype(np.float64), w.astype(np.float64)
    for lam_t in iteration_lambdas(lam, iters):
        N, D = solve_lines([N, D], guide, lam_t, weights, cyclic)
        N, D = (u.T for u in solve_lines([N.T, D.T], guide.T, lam_t, weights, False))
    keep = D >= 255.0 * min_weight
    if mask is not None:
        keep &= np.asarray(mask) != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.clip(np.floor(N / D + 0.5), 0.0, 32767.0)
    out = np.where(keep, np.where(keep, v, 0.0), -1.0).astype(np.int16)
    return out, np.stack([np.ascontiguousarray(N), np.ascontiguousarray(D)])
