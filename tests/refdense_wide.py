"""Dense omnistereo with D = 16 .. 256 disparities (include/sosvo_dense_wide.h: sosvo_dense_stereo_wide),
stated in numpy beside refdense and refdense8, which stay as they are.  The census is refdense's.  The recurrence
(refdense._path) and the diagonal lines (refdense8.diagonal) are written over the last axis, whatever its length; the stages
that have 64 in their text are stated here: cost_volume, aggregate (its bound), select and accuracy.  With D = 64 every stage
equals refdense / refdense8 (tests/test_dense_wide_reference.py).  Small integers throughout: the device reproduces S and d16
bit for bit (tests/test_gpu_dense_wide.py)."""
import numpy as np

import refdense
import refdense8

DISPARITIES = tuple(range(16, 257, 16))
MAX_P2 = {4: 8191, 8: 8127}       # S = the sum of `paths` L <= paths * (64 + P2) stays u16, whatever D


def _check_D(D):
    if D not in DISPARITIES:
        raise ValueError("disparities must be a multiple of 16 in 16 .. 256, got %r" % (D,))
    return D


def cost_volume(census_top, census_bot, d0, D):
    """C [rows, cols, D] u8: the Hamming distance of census_top(r, c) and census_bot(r - d0 - k, c); 64 where that row < 0
    (the census has 62 bits: 64 is a constant of the cost, not of D)."""
    rows, cols = census_top.shape
    C = np.full((rows, cols, _check_D(D)), 64, dtype=np.uint8)
    for k in range(D):
        d = d0 + k
        if d < rows:
            C[d:, :, k] = refdense._popcount(census_top[d:] ^ census_bot[:rows - d])
    return C


def aggregate(C, P1, P2, paths=4, cyclic=False):
    """S [rows, cols, D] u16 of C [rows, cols, D]: the sum of the four paths (down, up, left to right, right to left) and, with
    paths = 8, of the four diagonals; in each, k = 0 has no k - 1 and k = D - 1 has no k + 1."""
    if paths not in (4, 8):
        raise ValueError("paths must be 4 or 8, got %r" % (paths,))
    assert P2 <= MAX_P2[paths]
    C = C.astype(np.int32)
    Ct = C.transpose(1, 0, 2)
    path = refdense._path
    S = path(C, P1, P2) + path(C[::-1], P1, P2)[::-1]
    S = S + path(Ct, P1, P2).transpose(1, 0, 2) + path(Ct[::-1], P1, P2)[::-1].transpose(1, 0, 2)
    if paths == 8:
        for dr, dc in refdense8.DIAGONALS:
            S = S + refdense8.diagonal(C, P1, P2, dr, dc, cyclic)
    assert S.max() <= paths * (64 + P2) <= 65528
    return S.astype(np.uint16)


def select(S, d0, uniqueness, lr_max, mask=None):
    """d16 [rows, cols] i16 of S [rows, cols, D]: the winner over the D values, uniqueness / reach / mask, the left-right check
    (lr_max >= 0), and the 1/16-row parabola, skipped at k* = 0 and k* = D - 1."""
    S = S.astype(np.int32)
    rows, cols, D = S.shape
    ks = S.argmin(axis=-1)                      # the smallest k among the minimal S
    mS = S.min(axis=-1)
    kk = np.arange(D)
    far = np.abs(kk[None, None, :] - ks[..., None]) > 1
    ok = ~(far & (S * (100 - uniqueness) < (mS * 100)[..., None])).any(axis=-1)
    rb = np.arange(rows)[:, None] - (d0 + ks)
    ok &= rb >= 0
    if mask is not None:
        ok &= np.asarray(mask) != 0
    if lr_max >= 0:
        cc = np.arange(cols)
        best_mS = np.full((rows, cols), np.iinfo(np.int32).max, dtype=np.int32)
        kept = np.zeros((rows, cols), dtype=np.int64)
        for r in range(rows):                   # ascending r: a tie stays with the smaller r
            take = ok[r].copy()
            take[take] = mS[r, take] < best_mS[rb[r, take], cc[take]]
            best_mS[rb[r, take], cc[take]] = mS[r, take]
            kept[rb[r, take], cc[take]] = ks[r, take]
        r_i, c_i = np.nonzero(ok)
        bad = np.abs(kept[rb[r_i, c_i], c_i] - ks[r_i, c_i]) > lr_max
        ok[r_i[bad], c_i[bad]] = False
    a = np.take_along_axis(S, np.maximum(ks - 1, 0)[..., None], axis=-1)[..., 0]
    b = np.take_along_axis(S, np.minimum(ks + 1, D - 1)[..., None], axis=-1)[..., 0]
    den = np.maximum(a + b - 2 * mS, 1)
    off = ((a - b) * 16 + den) // (2 * den)     # floor division
    off[(ks < 1) | (ks > D - 2)] = 0
    assert off.min() >= -8 and off.max() <= 8
    d16 = np.where(ok, (d0 + ks) * 16 + off, -1)
    assert d16.max() <= (1024 + 255) * 16 + 8
    return d16.astype(np.int16)


def winners(S, d0, uniqueness, lr_max, mask=None):
    """k* [rows, cols] of the pixels select keeps, -1 elsewhere (what the device's k* plane holds after the left-right check)."""
    d16 = select(S, d0, uniqueness, lr_max, mask)
    return np.where(d16 >= 0, S.argmin(axis=-1), -1)


def dense_stereo(top, bot, mask=None, min_disparity=1, P1=8, P2=48, uniqueness=15, lr_max=1, cyclic=False, want_volume=False, paths=4,
                 disparities=64):
    """One frame: top, bot [rows, cols] u8 -> d16 (and S [rows, cols, disparities])."""
    C = cost_volume(refdense.census(top, cyclic), refdense.census(bot, cyclic), min_disparity, disparities)
    S = aggregate(C, P1, P2, paths, cyclic)
    d16 = select(S, min_disparity, uniqueness, lr_max, mask)
    return (d16, S) if want_volume else d16


def accuracy(d16, true, valid_top, valid_bot, lo=0.0, hi=63.0):
    """refdense.accuracy's figures on the comparable pixels whose true disparity lies in [lo, hi): inside the top mask, the true
    partner (r - d, c) inside the bottom mask and the panorama.  -> (comparable, share of them with a disparity, share of them
    with a disparity within 1 row of the truth, share of those with a disparity that lie within 1 row, their median |error| in
    rows; the last two NaN when no pixel has a disparity)."""
    rows, cols = true.shape
    rr, cc = np.mgrid[0:rows, 0:cols]
    rb = np.clip(np.rint(rr - true).astype(np.int64), 0, rows - 1)
    comparable = (valid_top != 0) & (valid_bot[rb, cc] != 0) & (rr - true >= 0) & (true >= lo) & (true < hi)
    ok = comparable & (d16 >= 0)
    err = np.abs(d16[ok] / 16.0 - true[ok])
    count = int(comparable.sum())
    if err.size == 0:
        return count, 0.0, 0.0, float("nan"), float("nan")
    return count, float(ok.sum() / count), float((err <= 1.0).sum() / count), float((err <= 1.0).mean()), float(np.median(err))
