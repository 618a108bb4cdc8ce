"""The one-wave form of the greedy minimum-distance pass on its integer grid (gft_select_kernel with four-wave workgroups)
against the oracle, bit for bit.  That form only runs in launches of MORE THAN 1024 problems, so every case is one launch
of 132 images x 8 masks of a small image -- three strips of 58 columns, two row chunks -- drawn from a few distinct images
repeated; every problem of the launch is compared.  The oracle runs once per distinct (image, mask).

From the oracle alone every case keeps status 0 (no more candidates than the selection sorts; the third points of a cell
fit the overflow list); that is asserted here as well as on the device's status words."""
import functools

import numpy as np
import pytest

import oracle
from test_gpu_image import _textured, _to

pytestmark = pytest.mark.gpu

NI, NMASK, CAP = 132, 8, 256          # 1056 problems: four-wave workgroups, one-wave greedy pass
ROWS, COLS = 48, 130
QUALITY = 0.002


def _masks(rows, cols):
    """Eight masks: 0 starts at column 1 / row 1, 1 ends at cols - 2 / rows - 2 (the border of the bordered grid), 2 is the
    whole image (hundreds of candidates on noise: several rounds of 64), 3 is empty, 4 .. 7 are azimuthal sectors that share
    their boundary columns."""
    bits = np.zeros((rows, cols), np.uint32)
    bits[1:rows // 2, 1:cols // 2] |= 1 << 0
    bits[rows // 3:rows - 1, cols // 2:cols - 1] |= 1 << 1
    bits[:, :] |= 1 << 2
    edges = np.linspace(0, cols - 1, 5).astype(int)
    for k in range(4):
        bits[3:rows - 4, edges[k]:edges[k + 1] + 1] |= np.uint32(1 << (4 + k))
    return bits


def _periodic(rows, cols):
    """An exactly periodic checkerboard: the responses of its junctions tie exactly, within a row and across rows."""
    y, x = np.mgrid[0:rows, 0:cols]
    return (40 + 160 * (((x % 8) < 4) ^ ((y % 8) < 4))).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _images(rows=ROWS, cols=COLS):
    rng = np.random.default_rng(rows * 1000 + cols)
    noise = rng.integers(0, 256, size=(rows, cols), dtype=np.uint8)
    smooth = oracle.median_gray(_textured(rng, (rows, cols, 3)), 0)
    flat = np.full((rows, cols), 17, np.uint8)
    return np.stack([noise, smooth, _periodic(rows, cols), flat])


@functools.lru_cache(maxsize=None)
def _eigs(rows=ROWS, cols=COLS):
    return [oracle.min_eigen(im) for im in _images(rows, cols)]


def _run(ctx, imgs, bits, nimg, **kw):
    """One launch of nimg images (the distinct ones repeated in turn) -> kp, n, status on the host."""
    reps = np.stack([imgs[i % len(imgs)] for i in range(nimg)])
    t_img, t_bits = _to(ctx.device, reps, bits[None])
    kp, n, status = ctx.detect_gft(t_img, t_bits, nimg, NMASK, CAP, quality=QUALITY, **kw)
    ctx.synchronize()
    return kp.cpu().numpy(), n.cpu().numpy(), status.cpu().numpy()


def _compare(got, eigs, bits, nimg, min_distance, max_corners):
    """Every problem of the launch against the oracle; returns the oracle's lists per (distinct image, mask)."""
    kp, n, status = got
    want = {}
    for d, eig in enumerate(eigs):
        for m in range(NMASK):
            w, _, count = oracle.gft_select(eig, bits, m, QUALITY, min_distance, max_corners, cand_cap=oracle.gft_cand_cap(CAP),
                                            with_count=True)
            assert count <= oracle.gft_cand_cap(CAP), (d, m, count)      # status 0 from the oracle alone
            want[d, m] = w[:CAP]
    assert not status.any(), np.flatnonzero(status)
    for i in range(nimg):
        for m in range(NMASK):
            w, p = want[i % len(eigs), m], i * NMASK + m
            assert n[p] == len(w), (i, m, n[p], len(w))
            assert np.array_equal(kp[p, : n[p]], w), (i, m)
    return want


@pytest.mark.parametrize("min_distance", [0.0, 0.5, 1.0, 1.5, 5.0, 7.5, 31.0])
def test_one_wave_greedy_pass_minimum_distances(ctx, min_distance):
    """Unspaced (0, 0.5: the float form, no distance test), cell 1 (the whole-image mask's grid does not fit: float form with
    the list), non-integer md^2 against ceil (1.5, 7.5), cells of several pixels; masks that touch the grid's border; an
    empty mask; a flat image; a mask of several rounds."""
    bits = _masks(ROWS, COLS)
    want = _compare(_run(ctx, _images(), bits, NI, min_distance=min_distance, max_corners=0), _eigs(), bits, NI, min_distance, 0)
    assert all(len(want[3, m]) == 0 for m in range(NMASK)) and all(len(want[d, 3]) == 0 for d in range(4))
    if min_distance <= 1.5:
        assert len(want[0, 2]) > 128                                    # several rounds, conflicts with earlier rounds
    assert sum(len(w) for w in want.values()) > (40 if min_distance > 10 else 200)


@pytest.mark.parametrize("max_corners", [0, 37, 100])
def test_one_wave_greedy_pass_budgets(ctx, max_corners):
    """A budget that is reached in the middle of a round of 64 (37: the first round; 100: the second)."""
    bits = _masks(ROWS, COLS)
    want = _compare(_run(ctx, _images(), bits, NI, min_distance=2.0, max_corners=max_corners), _eigs(), bits, NI, 2.0, max_corners)
    if max_corners:
        assert len(want[0, 2]) == max_corners and len(want[1, 2]) == max_corners    # the budget ended the pass
    else:
        assert len(want[0, 2]) > 128


def test_packed_keys_keep_the_order_of_tied_responses(ctx):
    """The periodic image's junctions have exactly equal responses in one row and in different rows: the sort must take
    them 'higher address first' with the packed (y << 16 | x) keys as with the linear ones.  The oracle's list of the
    whole-image mask holds such ties next to each other; the device's equals it in order."""
    bits = _masks(ROWS, COLS)
    eig = _eigs()[2]
    want = _compare(_run(ctx, _images(), bits, NI, min_distance=3.0, max_corners=0), _eigs(), bits, NI, 3.0, 0)
    w = want[2, 2].astype(int)
    vals = eig[w[:, 1], w[:, 0]]
    tied = vals[1:] == vals[:-1]
    same_row = tied & (w[1:, 1] == w[:-1, 1])
    other_row = tied & (w[1:, 1] != w[:-1, 1])
    assert same_row.sum() >= 5 and other_row.sum() >= 3
    assert (w[1:, 0][same_row] < w[:-1, 0][same_row]).all() and (w[1:, 1][other_row] < w[:-1, 1][other_row]).all()


def test_third_point_of_a_cell_suppresses_in_a_later_round(ctx):
    """minDistance 31: three corners at 31.05 / 31.05 / 31.1 pixels inside ONE cell of 31 x 31; the third goes to the overflow
    list, and a weaker corner 24.6 pixels from it only -- more than 64 candidates later -- must still be rejected."""
    rows, cols = 64, 130
    img = np.zeros((rows, cols), np.uint8)

    def blob(x, y, v):
        img[y - 1:y + 2, x - 1:x + 2] = v
    blob(92, 39, 250), blob(70, 61, 247), blob(62, 31, 244)     # the cell x 62 .. 92, y 31 .. 61
    blob(40, 20, 120)                                           # 24.6 px from (62, 31), far from the other two
    for i in range(72):                                         # > 64 candidates in between
        blob(100 + 5 * (i % 6), 3 + 5 * (i // 6), 200)
    bits = np.full((rows, cols), 0xFF, np.uint32)
    imgs = img[None]
    eigs = [oracle.min_eigen(img)]
    want = _compare(_run(ctx, imgs, bits, NI, min_distance=31.0, max_corners=0), eigs, bits, NI, 31.0, 0)
    got = {(int(x), int(y)) for x, y in want[0, 0]}
    assert {(92, 39), (70, 61), (62, 31)} <= got and (40, 20) not in got
    order, _ = oracle.gft_select(eigs[0], bits, 0, QUALITY, 0.0, 0)
    rank = {(int(x), int(y)): k for k, (x, y) in enumerate(order)}
    assert rank[40, 20] - rank[62, 31] > 64 and rank[62, 31] < 64


def test_one_launch_mixes_the_small_and_the_full_variant(ctx):
    """A noise image beside smooth ones: its whole-image mask has more candidates than the first pass sorts (2048) and goes
    to the 4096 variant, the others stay with the first pass -- in one launch."""
    rows, cols = 128, 260
    bits = _masks(rows, cols)
    keep = [0, 1, 3]                  # (the periodic image's plateaus would be more candidates than any variant sorts)
    imgs, eigs = _images(rows, cols)[keep], [_eigs(rows, cols)[k] for k in keep]
    counts = [oracle.gft_select(e, bits, 2, QUALITY, 5.0, 0, with_count=True)[2] for e in eigs]
    assert 2048 < counts[0] <= 4096 and max(counts[1:]) <= 2048, counts
    _compare(_run(ctx, imgs, bits, NI, min_distance=5.0, max_corners=0), eigs, bits, NI, 5.0, 0)


def test_spread_and_one_wave_forms_agree(ctx):
    """The same images through a launch of 64 problems (eight-wave workgroups: the spread form) and of 1056 (the one-wave
    form): identical kp, n and status."""
    bits = _masks(ROWS, COLS)
    few = _run(ctx, _images(), bits, 8, min_distance=5.0, max_corners=0)
    many = _run(ctx, _images(), bits, NI, min_distance=5.0, max_corners=0)
    P = 8 * NMASK
    assert np.array_equal(few[1], many[1][:P]) and np.array_equal(few[2], many[2][:P])
    for p in range(P):
        assert np.array_equal(few[0][p, : few[1][p]], many[0][p, : few[1][p]]), p
    assert few[1].sum() > 200 and not few[2].any()
