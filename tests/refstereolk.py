"""The rule of sosvo_refine_stereo_lk (include/sosvo.h) on numpy arrays, built on reflk.track: the CPU reference the device
stage is compared with bit for bit, and the planted-shift scene both are measured on."""
import numpy as np

import reflk

KEY_NONE, KEY_IDX_MASK = 0xFFFFFFFF, 0xFFFFF
DEFAULTS = dict(half=4, max_iter=30, eps=0.01, min_eig=1e-4, max_shift=None)
SLACK = 2.0 ** -40


def bound(half, max_shift):
    """The acceptance bound: max_shift, or half where it is None or 0."""
    return float(max_shift) if max_shift else float(half)


def pre_gate_skips(ut, vt, ub, vb, s, min_disp, max_hdiff):
    """The pre-gate on float32 values, in double: True = the pair cannot pass the assemble gates after a move of at most s per
    axis.  Each side is on exactly when sv_pixel_gate's is.  (A NaN difference compares false: not skipped here.)"""
    du, dv = float(ut) - float(ub), float(vt) - float(vb)
    if max_hdiff > 0 and abs(du) > (max_hdiff + s) * (1.0 + SLACK):
        return True
    if min_disp >= 0 and dv + s < min_disp - SLACK * (abs(dv) + s + min_disp):
        return True
    return False


def passes_gates(ut, vt, ub, vb, min_disp, max_hdiff):
    """sv_pixel_gate of the assemble stage (geom_core.h)."""
    good = True
    if max_hdiff > 0:
        good = abs(float(ut) - float(ub)) <= max_hdiff
    if min_disp >= 0:
        good = good and (float(vt) - float(vb) >= min_disp)
    return good


def refine(gray, nmask, kp_top, n_top, kp_bot, n_bot, keys, half=4, max_iter=30, eps=0.01, min_eig=1e-4, max_shift=None,
           min_disp=-1.0, max_hdiff=0.0, row_range=None, pre_gate=True, status=None):
    """gray [2F, rows, cols] u8 view-major; kp_* [F*nmask, cap, 2] f32; n_* [F*nmask]; keys [F*nmask, cap] u32 ->
    (kp_bot, status [F*nmask, cap] u8) as NEW arrays (status: what the buffer held; rows at and beyond n_bot stay)."""
    F = gray.shape[0] // 2
    P, cap = kp_bot.shape[:2]
    assert P == F * nmask
    pyrs = reflk.pyramid_set(gray, 1, row_range)
    s = bound(half, max_shift)
    out = np.array(kp_bot, dtype=np.float32, copy=True)
    st = np.zeros((P, cap), np.uint8) if status is None else np.array(status, copy=True)
    for p in range(P):
        f = p // nmask
        nb, nt = min(max(int(n_bot[p]), 0), cap), min(max(int(n_top[p]), 0), cap)
        for q in range(nb):
            st[p, q] = 0
            key = int(keys[p, q])
            t = key & KEY_IDX_MASK
            if key == KEY_NONE or t >= nt:
                continue
            (ut, vt), (ub, vb) = kp_top[p, t], kp_bot[p, q]
            if pre_gate and pre_gate_skips(ut, vt, ub, vb, s, min_disp, max_hdiff):
                continue
            x, y, ok, _ = reflk.track(pyrs[f], pyrs[F + f], ut, vt, half, max_iter, eps, min_eig, guess=(ub, vb))
            if not ok:
                continue
            dx, dy = float(x) - float(ub), float(y) - float(vb)
            if not (abs(dx) <= s and abs(dy) <= s):       # (a NaN fails)
                continue
            out[p, q] = (x, y)
            st[p, q] = 1
    return out, st


# ---- the planted-shift scene -------------------------------------------------------------------------------------------------
SHIFTS = ((0.37, -7.21), (-1.6, -12.45), (2.2, -1.3))
ROWS, COLS = 96, 128
# the largest error of reflk.track on this scene (one level, 120 tracks per shift: the guess at the rounded true partner and at
# that + (1, -1); max_iter 30, eps 0.01, min_eig 1e-4), in pixels, per half and shift -- measured with reflk.track on the CPU
MEASURED_MAX = {2: (0.182, 0.223, 0.249), 4: (0.0653, 0.0716, 0.0719), 10: (0.0306, 0.0306, 0.0389)}


def planted(shift):
    """-> (gray [2, 96, 128] u8: top = the texture, bottom = the texture moved by `shift`; the 60 grid points; their true
    partners as float64 [60, 2])."""
    top = reflk.texture(7, ROWS, COLS)
    bot = reflk.texture(7, ROWS, COLS, shift=shift)
    pts = reflk.grid_points(ROWS, COLS, 24, 8)
    return np.stack([top, bot]), pts, pts.astype(np.float64) + np.asarray(shift, np.float64)


def planted_tables(shift, cap=128):
    """One frame, one mask: the 60 points as top keypoints, 120 bottom keypoints -- the rounded true partner and that + (1, -1)
    -- matched to them -> dict(gray, kp_top, n_top, kp_bot, n_bot, keys, truth [120, 2])."""
    gray, pts, true = planted(shift)
    n = len(pts)
    guess = np.rint(true)
    kp_top = np.zeros((1, cap, 2), np.float32)
    kp_bot = np.zeros((1, cap, 2), np.float32)
    kp_top[0, :n] = pts
    kp_bot[0, :n] = guess
    kp_bot[0, n:2 * n] = guess + (1.0, -1.0)
    keys = np.full((1, cap), KEY_NONE, np.uint32)
    keys[0, :2 * n] = np.concatenate([np.arange(n), np.arange(n)]).astype(np.uint32) | np.uint32(17 << 20)
    return dict(gray=gray, kp_top=kp_top, n_top=np.array([n], np.int32), kp_bot=kp_bot, n_bot=np.array([2 * n], np.int32),
                keys=keys, truth=np.concatenate([true, true]))


def errors(kp_bot, truth):
    """Distance of the first len(truth) bottom keypoints of problem 0 from the truth."""
    d = kp_bot[0, :len(truth)].astype(np.float64) - truth
    return np.hypot(d[:, 0], d[:, 1])
