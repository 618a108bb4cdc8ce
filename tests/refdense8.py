"""The eight-path form of the dense omnistereo algorithm (include/sosvo.h: sosvo_dense_stereo_paths),
stated in numpy on top of refdense, which stays as it is: every stage but the aggregation is refdense's.  The four diagonal
paths are stated as skewed lines, the form the kernel has; tests/test_dense8_reference.py checks that form against a per-pixel
loop over predecessors.  Small integers throughout: the device reproduces S and d16 bit for bit (tests/test_gpu_dense8.py)."""
import numpy as np

import refdense

D = refdense.D
MAX_P2 = 8127                      # S = the sum of eight L <= 8 * (64 + P2) stays u16
DIAGONALS = ((1, 1), (1, -1), (-1, 1), (-1, -1))      # (dr, dc): the predecessor of (r, c) is (r - dr, c - dc)


def diagonal(C, P1, P2, dr, dc, cyclic):
    """L [rows, cols, 64] int32 of the path (dr, dc) over C [rows, cols, 64].  Line j in [0, cols) at step i in [0, rows) visits
    row i (dr = +1) or rows - 1 - i (dr = -1) and column (j + dc * i) mod cols; clamped, it starts again with L = C at every
    step i > 0 whose column is 0 (dc = +1) or cols - 1 (dc = -1): there c - dc lies outside [0, cols)."""
    C = C.astype(np.int32)
    rows, cols = C.shape[:2]
    i = np.arange(rows)
    r = (i if dr > 0 else rows - 1 - i)[:, None]
    col = (np.arange(cols)[None, :] + dc * i[:, None]) % cols           # [step, line]
    Cseq = C[r, col]
    if cyclic:
        L = refdense._path(Cseq, P1, P2)
    else:
        L = np.empty_like(Cseq)
        L[0] = Cseq[0]
        for s in range(1, rows):
            step = refdense._path(np.stack([L[s - 1], Cseq[s]]), P1, P2)[1]     # one step of the recurrence on L[s - 1]
            L[s] = np.where((col[s] == (0 if dc > 0 else cols - 1))[:, None], Cseq[s], step)
    out = np.empty_like(C)
    out[r, col] = L                # every pixel is visited by exactly one line, exactly once
    return out


def aggregate(C, P1, P2, paths=4, cyclic=False):
    """S [rows, cols, 64] u16: refdense.aggregate's four paths, and with paths = 8 the four diagonals as well."""
    if paths not in (4, 8):
        raise ValueError("paths must be 4 or 8, got %r" % (paths,))
    S = refdense.aggregate(C, P1, P2)
    if paths == 4:
        return S
    assert P2 <= MAX_P2
    S = S.astype(np.int32)
    for dr, dc in DIAGONALS:
        S = S + diagonal(C, P1, P2, dr, dc, cyclic)
    assert S.max() <= 8 * (64 + P2) <= 65528
    return S.astype(np.uint16)


def dense_stereo(top, bot, mask=None, min_disparity=1, P1=8, P2=48, uniqueness=15, lr_max=1, cyclic=False, want_volume=False, paths=4):
    """One frame: top, bot [rows, cols] u8 -> d16 (and S): refdense.dense_stereo with `paths` aggregation paths."""
    C = refdense.cost_volume(refdense.census(top, cyclic), refdense.census(bot, cyclic), min_disparity)
    S = aggregate(C, P1, P2, paths, cyclic)
    d16 = refdense.select(S, min_disparity, uniqueness, lr_max, mask)
    return (d16, S) if want_volume else d16
