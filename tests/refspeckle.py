"""The speckle filter of the dense disparity map in numpy: the text of include/sosvo.h at
sosvo_dense_speckle, as union-find over the edge list (hook every root to the smaller root across an edge, compress, repeat).
The device reproduces it bit for bit; tests/test_speckle_reference.py pins it against scipy.ndimage.label and a flood fill."""
import numpy as np

NONE = np.uint32(0xFFFFFFFF)      # the label of an invalid pixel


def edges(d16, max_diff, cyclic=False):
    """-> (a, b): the row-major indices of every joined pair of one frame d16 [rows, cols] (a: the upper / left pixel, or
    across the seam the pixel of the last column)."""
    d = np.asarray(d16).astype(np.int32)
    rows, cols = d.shape
    idx = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
    valid = d >= 0

    def pairs(sa, sb):
        ok = valid[sa] & valid[sb] & (np.abs(d[sa] - d[sb]) <= int(max_diff))
        return idx[sa][ok], idx[sb][ok]
    both = [pairs((slice(0, rows - 1), slice(None)), (slice(1, rows), slice(None))),
            pairs((slice(None), slice(0, cols - 1)), (slice(None), slice(1, cols)))]
    if cyclic and cols > 1:
        both.append(pairs((slice(None), slice(cols - 1, cols)), (slice(None), slice(0, 1))))
    return np.concatenate([p[0] for p in both]), np.concatenate([p[1] for p in both])


def labels_of(d16, max_diff, cyclic=False):
    """-> labels [rows, cols] u32 of one frame: the smallest row-major index of the pixel's component, NONE where d16 < 0."""
    d = np.asarray(d16)
    a, b = edges(d, max_diff, cyclic)
    parent = np.arange(d.size, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]          # (roots: the forest is fully compressed here)
        lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
        if np.array_equal(lo, hi):
            break
        np.minimum.at(parent, hi, lo)          # hook: a root goes below the smallest root it shares an edge with
        while True:                            # compress
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    return np.where(d.reshape(-1) >= 0, parent, int(NONE)).astype(np.uint32).reshape(d.shape)


def speckle(d16, max_size, max_diff, cyclic=False, want_labels=False):
    """d16 [rows, cols] or [n, rows, cols] int16 -> the filtered map (and the labels): a valid pixel (d16 >= 0) whose component
    has at most max_size pixels becomes -1; everything else is copied."""
    d = np.asarray(d16)
    assert d.dtype == np.int16 and d.ndim in (2, 3)
    if d.ndim == 3:
        res = [speckle(f, max_size, max_diff, cyclic, True) for f in d]
        out, lab = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
        return (out, lab) if want_labels else out
    lab = labels_of(d, max_diff, cyclic)
    valid = lab != NONE
    size = np.bincount(lab[valid].astype(np.int64), minlength=d.size)
    drop = np.zeros(d.shape, bool)
    drop[valid] = size[lab[valid].astype(np.int64)] <= int(max_size)
    out = np.where(drop, np.int16(-1), d).astype(np.int16)
    return (out, lab) if want_labels else out
