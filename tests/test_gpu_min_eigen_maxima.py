"""Per-mask maxima and candidate records of the two-columns-per-lane corner-response kernel against the oracle, bit for bit,
on small images whose mask word changes along the rows of a column (the kernel keeps the running
maximum of a run of equal mask words as a float and the run's word in the ring of the rows' mask words; the ordered key is
made where a run ends).

Every call has two images with a mask set each, six masks:
  0, 1  two overlapping masks: the columns of the middle third carry both bits in one word, mask 1 without the first and the
        last row, so the word of those columns changes from 1 to 3 and back;
  2     starts and ends inside the row chunk (three rows in the middle, the middle half of the columns);
  3     only pixels with a non-positive response: in image 0 the interior of a FLAT block (response +0.0 exactly: key
        0x80000000), in image 1 the interior of a LINEAR RAMP (gradient tensor of rank one: the response is the rounding
        error of (a + c) - sqrt((a - c)^2 + b^2); the slopes are searched for one that makes it NEGATIVE, so the maximum of the
        mask is negative and its key the inverted form);
  4     a lattice, (x + y) % 3 == 0, whose bit changes the word on every row; EMPTY in image 1's set;
  5     empty in both sets.
Image 1's set also leaves the first and the last two rows without any mask (rows the kernel steps over with cleared words).
A second call per shape keeps image 0's set and gives image 1 a set that is empty altogether.

Shapes: 9 and 40 rows; 8 (the narrowest the two-column form takes), 61 (one strip), 62 (the pair boundary), 123 (an odd
strip count) and 250 columns (an image-border strip on both sides).  The oracle's response is computed once per image."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

ROWS = [9, 40]
COLS = [8, 61, 62, 123, 250]
NMASK = 6
SLOPES = [(1, 2), (2, 1), (1, 3), (3, 1), (2, 3), (3, 2), (1, 4), (4, 1), (3, 4), (4, 3), (1, 5), (5, 1), (2, 5), (5, 2)]


def _ordered(f):
    u = int(np.float32(f).view(np.uint32))
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def _local_maxima(eig):
    rows, cols = eig.shape
    out = np.zeros(eig.shape, bool)
    nb = np.full((rows - 2, cols - 2), -np.inf, np.float32)
    for dy in range(3):
        for dx in range(3):
            nb = np.maximum(nb, eig[dy:dy + rows - 2, dx:dx + cols - 2])
    c = eig[1:-1, 1:-1]
    out[1:-1, 1:-1] = (c == nb) & (c > 0)
    return out


def _block(rows, cols):
    """The 7 x min(cols, 9) block that holds the flat patch / the ramp: rows y0 .. y0 + 6, columns x0 .. x0 + bw - 1."""
    bw = min(cols, 9)
    return rows - 7 if rows < 20 else 21, (cols - bw) // 2, bw


_SCENES = {}


def _scene(rows, cols):
    """(images [2, rows, cols], responses, mask sets [2, rows, cols]) of one shape; made once."""
    if (rows, cols) in _SCENES:
        return _SCENES[(rows, cols)]
    rng = np.random.default_rng(1000 * rows + cols)
    imgs = rng.integers(0, 256, (2, rows, cols), dtype=np.uint8)
    y0, x0, bw = _block(rows, cols)
    imgs[0, y0:y0 + 7, x0:x0 + bw] = 93
    yy, xx = np.mgrid[0:7, 0:bw]
    inner = (slice(y0 + 2, y0 + 5), slice(x0 + 2, x0 + bw - 2))   # the pixels whose 5 x 5 support lies inside the block
    for sx, sy in SLOPES:                                         # a ramp whose (rounding-error) response is negative
        imgs[1, y0:y0 + 7, x0:x0 + bw] = (20 + sx * xx + sy * yy).astype(np.uint8)
        if oracle.min_eigen(imgs[1])[inner].max() < 0:
            break
    eigs = [oracle.min_eigen(im) for im in imgs]
    assert (eigs[0][inner] == 0).all() and not np.signbit(eigs[0][inner]).any(), "the flat block's response is +0.0"
    assert eigs[1][inner].max() < 0, "no slope of the list gives a negative response on the ramp"

    bits = np.zeros((2, rows, cols), np.uint32)
    y, x = np.mgrid[0:rows, 0:cols]
    for s in range(2):
        bits[s, :, : -(-2 * cols // 3)] |= np.uint32(1)
        bits[s, 1:rows - 1, cols // 3:] |= np.uint32(2)
        bits[s, rows // 3: rows // 3 + 3, cols // 4: cols - cols // 4] |= np.uint32(4)
        bits[s][inner] |= np.uint32(8)
    bits[0][(x + y) % 3 == 0] |= np.uint32(16)
    bits[1, :2] = 0
    bits[1, rows - 2:] = 0
    assert ((bits[0] & 3) == 3).any() and (bits[1] & 16).max() == 0 and (bits & 32).max() == 0
    assert (np.diff(bits[0].astype(np.int64), axis=0) != 0).any(axis=0).all(), "every column's word changes along the rows"
    _SCENES[(rows, cols)] = (imgs, eigs, bits)
    return _SCENES[(rows, cols)]


def _check(ctx, imgs, eigs, bits, tag):
    NI, rows, cols = imgs.shape
    r = ctx.detect_gft_candidates(torch.from_numpy(imgs.copy()).to(ctx.device), torch.from_numpy(bits.copy()).to(ctx.device), 1, NMASK)
    ctx.synchronize()
    cand, wcnt, mstat = r["cand"].cpu().numpy(), r["wcnt"].cpu().numpy(), r["mstat"].cpu().numpy()
    w, strips, nchunks, cr = r["strip_w"], r["strips"], r["nchunks"], r["chunk_rows"]
    assert w == 61 and strips == -(-cols // 61) and nchunks * cr >= rows and r["regions"] == NI * strips * nchunks, tag
    y2 = rows // 3
    assert y2 // cr == (y2 + 2) // cr and y2 % cr > 0 and (y2 + 3) % cr > 0, "mask 2 starts and ends inside a chunk"
    nrec = 0
    for i in range(NI):
        mb = bits[i] & np.uint32((1 << NMASK) - 1)
        cmap = _local_maxima(eigs[i]) & (mb != 0)
        for c in range(nchunks):
            for s in range(strips):
                reg = (i * nchunks + c) * strips + s
                ys, xs = np.nonzero(cmap[c * cr: (c + 1) * cr, s * w: (s + 1) * w])   # row-major, ascending x
                ys, xs = ys + c * cr, xs + s * w
                want = np.stack([eigs[i][ys, xs].view(np.uint32), (ys.astype(np.uint32) << 16) | xs.astype(np.uint32)], axis=1)
                n = int(wcnt[reg])
                assert n == len(want), "%s: image %d chunk %d strip %d: wcnt %d, oracle %d" % (tag, i, c, s, n, len(want))
                assert np.array_equal(cand[reg, :n], want), "%s: image %d chunk %d strip %d: records differ" % (tag, i, c, s)
                nrec += n
        for m in range(NMASK):
            inside = ((mb >> np.uint32(m)) & 1).astype(bool)
            want_max = _ordered(eigs[i][inside].max()) if inside.any() else 0
            assert int(mstat[i * NMASK + m, 0]) == want_max, \
                "%s: image %d mask %d: maximum key %08x, oracle %08x" % (tag, i, m, int(mstat[i * NMASK + m, 0]), want_max)
    return mstat, nrec


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_maxima_and_records_under_changing_mask_words(ctx, rows, cols):
    imgs, eigs, bits = _scene(rows, cols)
    mstat, nrec = _check(ctx, imgs, eigs, bits, "rows %d cols %d" % (rows, cols))
    assert int(mstat[0 * NMASK + 3, 0]) == 0x80000000                 # the flat block: +0.0
    assert 0 < int(mstat[1 * NMASK + 3, 0]) < 0x80000000             # the ramp: a negative maximum, the inverted key
    assert int(mstat[1 * NMASK + 4, 0]) == 0 and int(mstat[0 * NMASK + 4, 0]) > 0x80000000   # empty in one view only
    assert int(mstat[0 * NMASK + 5, 0]) == 0 and int(mstat[1 * NMASK + 5, 0]) == 0
    assert nrec > 0


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_mask_set_empty_in_one_view(ctx, rows, cols):
    imgs, eigs, bits = _scene(rows, cols)
    bits = bits.copy()
    bits[1] = 0
    mstat, nrec = _check(ctx, imgs, eigs, bits, "rows %d cols %d, view 1 without masks" % (rows, cols))
    assert not mstat[NMASK:, 0].any() and int(mstat[3, 0]) == 0x80000000 and nrec > 0
