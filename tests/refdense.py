"""The dense omnistereo algorithm of include/sosvo.h (sosvo_dense_stereo), stated in numpy stage by
stage: census -> cost_volume -> aggregate (S) -> select (d16), and triangulate composed from the CPU oracle's geometry.
Small integers throughout: the device reproduces every stage bit for bit (tests/test_gpu_dense.py).  Single images
[rows, cols]; dense_stereo() runs the stages for one frame."""
import numpy as np

D = 64
_BIG = 1 << 20


def census(g, cyclic=False):
    """g [..., rows, cols] u8 -> u64: 9 x 7 window, dy = -4 .. 4 outer, dx = -3 .. 3 inner, centre skipped, each tap
    appending (tap < centre); rows clamp, columns clamp or wrap (cyclic)."""
    g = np.asarray(g, dtype=np.uint8)
    rows, cols = g.shape[-2:]
    rr, cc = np.arange(rows), np.arange(cols)
    out = np.zeros(g.shape, dtype=np.uint64)
    for dy in range(-4, 5):
        ri = np.clip(rr + dy, 0, rows - 1)
        for dx in range(-3, 4):
            if dy == 0 and dx == 0:
                continue
            ci = (cc + dx) % cols if cyclic else np.clip(cc + dx, 0, cols - 1)
            tap = g[..., ri[:, None], ci[None, :]]
            out = (out << np.uint64(1)) | (tap < g).astype(np.uint64)
    return out


def _popcount(x):
    x = np.ascontiguousarray(x, dtype=np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(x.shape + (8,)), axis=-1).sum(axis=-1)


def cost_volume(census_top, census_bot, d0):
    """C [rows, cols, 64] u8: the Hamming distance of census_top(r, c) and census_bot(r - d0 - k, c); 64 where that row < 0."""
    rows, cols = census_top.shape
    C = np.full((rows, cols, D), 64, dtype=np.uint8)
    for k in range(D):
        d = d0 + k
        if d < rows:
            C[d:, :, k] = _popcount(census_top[d:] ^ census_bot[:rows - d])
    return C


def _path(Cseq, P1, P2):
    """Cseq [len, lines, 64] int32, the costs along each line in path order -> L of the same shape."""
    L = np.empty_like(Cseq)
    L[0] = Cseq[0]
    for i in range(1, Cseq.shape[0]):
        Lp = L[i - 1]
        m = Lp.min(axis=-1, keepdims=True)
        a = np.full_like(Lp, _BIG)
        b = np.full_like(Lp, _BIG)
        a[:, 1:] = Lp[:, :-1]      # L_prev(k - 1); none at k = 0
        b[:, :-1] = Lp[:, 1:]      # L_prev(k + 1); none at k = 63
        L[i] = Cseq[i] + np.minimum(np.minimum(Lp, m + P2), np.minimum(a, b) + P1) - m
    return L


def aggregate(C, P1, P2):
    """S [rows, cols, 64] u16: the sum of the four paths (down, up, left to right, right to left)."""
    C = C.astype(np.int32)
    Ct = C.transpose(1, 0, 2)
    S = _path(C, P1, P2) + _path(C[::-1], P1, P2)[::-1]
    S = S + _path(Ct, P1, P2).transpose(1, 0, 2) + _path(Ct[::-1], P1, P2)[::-1].transpose(1, 0, 2)
    assert S.max() <= 4 * (64 + P2)
    return S.astype(np.uint16)


def select(S, d0, uniqueness, lr_max, mask=None):
    """d16 [rows, cols] i16: winner, uniqueness / reach / mask, left-right check (lr_max >= 0), 1/16-row parabola."""
    S = S.astype(np.int32)
    rows, cols = S.shape[:2]
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
    return np.where(ok, (d0 + ks) * 16 + off, -1).astype(np.int16)


def dense_stereo(top, bot, mask=None, min_disparity=1, P1=8, P2=48, uniqueness=15, lr_max=1, cyclic=False, want_volume=False):
    """One frame: top, bot [rows, cols] u8 -> d16 (and S)."""
    S = aggregate(cost_volume(census(top, cyclic), census(bot, cyclic), min_disparity), P1, P2)
    d16 = select(S, min_disparity, uniqueness, lr_max, mask)
    return (d16, S) if want_volume else d16


def triangulate(rig, d16, min_d16=16, max_d16=0):
    """X [..., rows, cols, 3] f64 of d16 [..., rows, cols]: for d16 >= 0 inside [min_d16, max_d16] (max_d16 <= 0: no upper gate)
    the top pixel (c, r) and the bottom pixel (c, r - d16 / 16) -> oracle.pano_to_angles -> oracle.triangulate_midpoint ->
    oracle.range_filter_homo; NaN everywhere else.  rig: anything with pano_top, pano_bot, F_top, F_bot, min_range, max_range."""
    import oracle
    d16 = np.asarray(d16)
    rows, cols = d16.shape[-2:]
    X = np.full(d16.shape + (3,), np.nan)
    sel = (d16 >= 0) & (d16 >= min_d16)
    if max_d16 > 0:
        sel &= d16 <= max_d16
    idx = np.nonzero(sel)
    r, c, d = idx[-2].astype(np.float64), idx[-1].astype(np.float64), d16[idx].astype(np.float64)
    az1, el1 = oracle.pano_to_angles(c, r, *[float(v) for v in rig.pano_top])
    az2, el2 = oracle.pano_to_angles(c, r - d / 16.0, *[float(v) for v in rig.pano_bot])
    P = oracle.triangulate_midpoint(az1, el1, az2, el2, [float(v) for v in rig.F_top], [float(v) for v in rig.F_bot])
    good = oracle.range_filter_homo(P, float(rig.min_range), float(rig.max_range))
    P[~good] = np.nan
    X[idx] = P
    return X


def true_disparity(gums, room, t):
    """Ray-cast truth for a frame of synthetic.render_omni(gums, room, identity, t): [rows, cols] f64, the disparity in rows of
    every top-panorama pixel = baseline / (rho * pixel_size), rho = the horizontal distance from the top focus to what
    synthetic.Room.cast hits along the pixel's bearing."""
    pano = gums.top_model.panorama
    rr, cc = np.mgrid[0:pano.rows, 0:pano.cols].astype(np.float64)
    az, h = 2 * np.pi - pano.pixel_size * cc, pano.cyl_height_max - pano.pixel_size * rr
    dirs = np.stack([np.cos(az), np.sin(az), h], axis=-1).reshape(-1, 3)   # unit horizontal length: the ray parameter is rho
    _, rho = room.cast(gums.top_model.F[:3, 0] + np.asarray(t, dtype=np.float64), dirs)
    return (gums.get_baseline() / (rho * pano.pixel_size)).reshape(pano.rows, pano.cols)


def accuracy(d16, true, valid_top, valid_bot):
    """The three figures against ray-cast truth.  Comparable pixels: inside the top mask, their true partner (r - d, c) inside
    the bottom mask and the panorama, true d < 63.  -> (comparable, share of them with a disparity, share of those within 1 row
    of the truth, their median |error| in rows)."""
    rows, cols = true.shape
    rr, cc = np.mgrid[0:rows, 0:cols]
    rb = np.clip(np.rint(rr - true).astype(np.int64), 0, rows - 1)
    comparable = (valid_top != 0) & (valid_bot[rb, cc] != 0) & (rr - true >= 0) & (true < 63)
    ok = comparable & (d16 >= 0)
    err = np.abs(d16[ok] / 16.0 - true[ok])
    return int(comparable.sum()), float(ok.sum() / comparable.sum()), float((err <= 1.0).mean()), float(np.median(err))
