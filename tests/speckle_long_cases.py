"""Disparity maps for the speckle filter at many 256-column rounds, the row and column limits, the working
size and large batches: the families of tests/speckle_cases.py at those shapes and three more that are built for what the row
kernel carries from round to round and for deep trees.  For tests/test_dense_long_reference.py and
tests/test_gpu_speckle_long.py.  Built for max_diff 16 like the others: joined neighbours differ by at most 16."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import speckle_cases  # noqa: E402

# rows x cols: four rounds of the row kernel; 64 rounds, the column limit; the row limit (rel0 = r * cols at its largest with
# two columns); the working size (822 workgroups per frame, `constant` one component of 210240 pixels)
SHAPES = [(3, 1000), (2, 16384), (16384, 2), (146, 1440)]
MANY = (3, 5, 201)                  # rows, cols, n of the one large batch
# a break immediately before each of these columns: the last column of a round, the first of the next, the one after
ROUND_EDGES = (255, 256, 257, 511, 512, 513, 767, 768, 769)

_FRAMES = {}


def round_edges(rows, cols):
    """Every pixel valid: 500, stepping up by 17 at each of ROUND_EDGES (inside the width) and nowhere else; the odd rows one
    column later, so that the vertical joins beside a break are not implied by the pair to their left."""
    cc = np.arange(cols)
    even = 500 + 17 * (cc[:, None] >= np.array(ROUND_EDGES)[None, :]).sum(axis=1)
    odd = 500 + 17 * (cc[:, None] >= np.array(ROUND_EDGES)[None, :] + 1).sum(axis=1)
    return np.where((np.arange(rows) & 1)[:, None] == 1, odd[None, :], even[None, :]).astype(np.int16)


def long_runs(rows, cols):
    """Every pixel valid: the even rows one unbroken run of 600 across the whole width, the odd rows 600 up to a single break in
    the last round of 256 columns and 617 from there (the last break carried through every round with none in between)."""
    rr, cc = np.mgrid[0:rows, 0:cols]
    last_round = (cols - 1) // 256 * 256
    brk = min(cols - 1, last_round + 5)
    return np.where(((rr & 1) == 1) & (cc >= brk), 617, 600).astype(np.int16)


def spiral(rows, cols):
    """A corridor one pixel wide from (0, 0) winding inward clockwise, walls one pixel wide: one component, and a tree as deep
    as the corridor is long.  -> valid [rows, cols] bool."""
    seen = np.zeros((rows + 2, cols + 2), bool)     # (a border, so that the neighbours of an edge pixel exist)
    r, c, dr, dc = 1, 1, 0, 1
    seen[r, c] = True

    def free(r1, c1, r0, c0):
        """(r1, c1) is inside, new, and touches nothing of the corridor but (r0, c0)."""
        if not (1 <= r1 <= rows and 1 <= c1 <= cols) or seen[r1, c1]:
            return False
        return int(seen[r1 - 1, c1]) + int(seen[r1 + 1, c1]) + int(seen[r1, c1 - 1]) + int(seen[r1, c1 + 1]) == 1

    while True:
        if not free(r + dr, c + dc, r, c):
            dr, dc = dc, -dr                         # turn right
            if not free(r + dr, c + dc, r, c):
                break
        r, c = r + dr, c + dc
        seen[r, c] = True
    return seen[1:-1, 1:-1]


def new_frames(rows, cols):
    """-> (names, d16 [3, rows, cols] int16): the three families of this file."""
    rng = np.random.default_rng(rows * 1000 + cols + 1)
    walls = speckle_cases.INVALID[rng.integers(0, 3, (rows, cols))]
    return ["round_edges", "long_runs", "spiral"], np.stack([round_edges(rows, cols), long_runs(rows, cols),
                                                              np.where(spiral(rows, cols), np.int16(900), walls)])


def batches(rows, cols):
    """The frames of speckle_cases.frames and new_frames in calls of n = 3 -> [(names, d16 [3, rows, cols])], built once per
    shape (do not write to them)."""
    if (rows, cols) not in _FRAMES:
        names, d = speckle_cases.frames(rows, cols)
        more, e = new_frames(rows, cols)
        names, d = names + more, np.concatenate([d, e])
        assert len(names) % 3 == 0
        _FRAMES[rows, cols] = [(names[i:i + 3], np.ascontiguousarray(d[i:i + 3])) for i in range(0, len(names), 3)]
    return _FRAMES[rows, cols]


def many():
    """One call of MANY[2] frames: the families at MANY[0] x MANY[1], cycled -> (names, d16 [n, rows, cols])."""
    rows, cols, n = MANY
    names, d = speckle_cases.frames(rows, cols)
    more, e = new_frames(rows, cols)
    names, d = names + more, np.concatenate([d, e])
    pick = np.arange(n) % len(names)
    return [names[i] for i in pick], np.ascontiguousarray(d[pick])
