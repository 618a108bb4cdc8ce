"""The disparity maps on which the speckle filter is tested, for tests/test_speckle_reference.py (numpy
against a flood fill) and tests/test_gpu_speckle.py (the device against numpy).  Every frame is built for max_diff 16: joined
neighbours differ by at most 16, separated ones by more."""
import numpy as np

# rows x cols: one pixel, one row, one column, a small odd shape, a whole number of waves per row, more than one 256-column
# round of the row kernel with a remainder, several blocks that are no multiple of anything
SHAPES = [(1, 1), (1, 70), (70, 1), (12, 9), (64, 64), (65, 257), (130, 33)]
INVALID = np.array([-1, -2, -32768], np.int16)


def _invalid(rng, shape):
    return INVALID[rng.integers(0, 3, shape)]


def frames(rows, cols):
    """-> (names, d16 [k, rows, cols] int16)."""
    rng = np.random.default_rng(rows * 1000 + cols)
    rr, cc = np.mgrid[0:rows, 0:cols]
    out = []

    def add(name, valid, value):
        out.append((name, np.where(valid, value, _invalid(rng, (rows, cols))).astype(np.int16)))

    for k in range(2):      # many small components: 30 % invalid, disparities from a small set (steps of 8, 16, 24 and more)
        add("random%d" % k, rng.random((rows, cols)) >= 0.3, np.array([160, 168, 176, 200, 400])[rng.integers(0, 5, (rows, cols))])
    add("ramp", np.ones((rows, cols), bool), 16 * (rr + cc))                      # one component through steps of exactly 16
    add("checkerboard", np.ones((rows, cols), bool), np.where((rr + cc) & 1, 100, 200))
    # a corridor one pixel wide: the even rows, joined at the right end after rows 0, 4, .. and at the left end after rows 2, 6, ..
    link = np.where((rr % 4) == 1, cc == cols - 1, cc == 0)
    add("serpentine", ((rr & 1) == 0) | link, 300 + (rr & 3))
    # a comb whose back is the LAST row: every tooth starts a tree of its own and the trees meet at the bottom
    add("comb", ((cc & 1) == 0) | (rr == rows - 1), 500)
    # two blobs in the first and the last columns that meet only across the seam (where the image is wide enough)
    w = max(1, min(2, cols // 3))
    add("seam_blobs", ((cc < w) | (cc >= cols - w)) & (rr >= rows // 3), np.where(cc < w, 300, 310))
    # a row that is one component only through the seam (a gap in the middle), and a whole row (already closed without it)
    gap = cols // 2
    add("ring", ((rr == 0) & (cc != gap)) | ((rr == rows - 1) & (rows >= 3)), 700 + 16 * (rr == 0) * (cc > gap))
    add("all_invalid", np.zeros((rows, cols), bool), 0)
    add("constant", np.ones((rows, cols), bool), 321)
    add("zero_and_max", rng.random((rows, cols)) >= 0.2, np.where(rng.random((rows, cols)) < 0.5, 0, 32767))
    add("random2", rng.random((rows, cols)) >= 0.3, 16 * rng.integers(0, 6, (rows, cols)))
    return [n for n, _ in out], np.stack([f for _, f in out])


def batches(rows, cols):
    """The frames in calls of n = 3 frames of different content -> [(names, d16 [3, rows, cols])]."""
    names, d = frames(rows, cols)
    assert len(names) % 3 == 0
    return [(names[i:i + 3], np.ascontiguousarray(d[i:i + 3])) for i in range(0, len(names), 3)]
