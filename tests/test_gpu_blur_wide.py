"""sosvo_gauss7, the descriptor stage's 7x7 blur on its own: the four-columns-per-lane form (gauss7_wide_kernel, the
default from 8 columns on) and the one-column form (below 8 columns, or under SOSVO_HINT_ROLLING_NARROW) against
oracle.gauss7, byte for byte, on the widths where a packed layout can go wrong: the fallback and its threshold, every
cols mod 4, one strip of 250 outputs exactly and the border lane on either side of it, the right border in lanes 0 and 1
of a second strip; heights shorter than the seven-row ring and heights of two row chunks; images that lie further apart
than their size, with sentinel bytes before, between and after the outputs; a row_range inside the image.  Inputs: noise
with runs of 0 and 255, and an all-255 image (the largest sums).  The oracle runs once per distinct image."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

COLS = list(range(3, 13)) + [61, 62, 63, 64] + [250, 251, 253, 256, 257] + [499, 500, 501, 502, 503]
ROWS = [3, 7, 8, 24, 49]
SENTINEL = 0xA5


def _images(rows, cols, seed):
    """Three images: noise with 0 / 255 pixels, all 255, noise of extremes only."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    pick = rng.integers(0, 6, (rows, cols))
    a[pick == 0] = 0
    a[pick == 1] = 255
    b = np.full((rows, cols), 255, np.uint8)
    c = np.where(rng.integers(0, 2, (rows, cols)) == 1, 255, 0).astype(np.uint8)
    return np.stack([a, b, c])


_WANT = {}


def _want(rows, cols, seed):
    key = (rows, cols, seed)
    if key not in _WANT:
        imgs = _images(rows, cols, seed)
        _WANT[key] = (imgs, np.stack([oracle.gauss7(im) for im in imgs]))
        _WANT[key][0].setflags(write=False)
        _WANT[key][1].setflags(write=False)
    return _WANT[key]


def _run(ctx, imgs, rows, cols, pad_in, pad_out, lead, row_range=None):
    """imgs [n, rows, cols] laid out img_stride apart behind `lead` bytes; the output likewise inside a buffer of sentinels.
    Returns (out [n, rows, cols], the whole output buffer, out_stride)."""
    n, px = imgs.shape[0], rows * cols
    s_in, s_out = px + pad_in, px + pad_out
    src = np.full(lead + (n - 1) * s_in + px, 0x3C, np.uint8)
    for i in range(n):
        src[lead + i * s_in: lead + i * s_in + px] = imgs[i].reshape(-1)
    dst = np.full(lead + (n - 1) * s_out + px + lead, SENTINEL, np.uint8)
    t_src, t_dst = torch.from_numpy(src).to(ctx.device), torch.from_numpy(dst).to(ctx.device)
    ctx.gauss7(t_src[lead:], n, rows, cols, out=t_dst[lead:], img_stride=s_in, out_stride=s_out, row_range=row_range)
    ctx.synchronize()
    buf = t_dst.cpu().numpy()
    out = np.stack([buf[lead + i * s_out: lead + i * s_out + px].reshape(rows, cols) for i in range(n)])
    return out, buf, s_out


def _check_sentinels(buf, n, px, s_out, lead):
    assert (buf[:lead] == SENTINEL).all(), "bytes before the first output image were written"
    for i in range(n - 1):
        gap = buf[lead + i * s_out + px: lead + (i + 1) * s_out]
        assert (gap == SENTINEL).all(), "bytes between output images %d and %d were written" % (i, i + 1)
    assert (buf[lead + (n - 1) * s_out + px:] == SENTINEL).all(), "bytes after the last output image were written"


@pytest.fixture
def narrow(ctx):
    """narrow(True / False) switches the session's context between the forms; the default form is restored afterwards."""
    def set_(on):
        ctx.set_hint_rolling_narrow(on)
    yield set_
    ctx.set_hint_rolling_narrow(False)


@pytest.mark.parametrize("cols", COLS)
def test_blur_forms_equal_the_oracle(ctx, narrow, cols):
    for rows in ROWS:
        imgs, want = _want(rows, cols, 1000 * rows + cols)
        for form in (False, True):
            narrow(form)
            # three images 37 / 5 bytes further apart than their size, 19 bytes of lead (odd: no alignment to lean on)
            out, buf, s_out = _run(ctx, imgs, rows, cols, 37, 5, 19)
            tag = "rows %d cols %d %s form" % (rows, cols, "narrow" if form else "default")
            assert np.array_equal(out, want), tag + ": %d bytes differ" % int((out != want).sum())
            _check_sentinels(buf, 3, rows * cols, s_out, 19)


@pytest.mark.parametrize("cols", COLS)
def test_blur_single_image_dense(ctx, narrow, cols):
    """nimg = 1, strides equal to the image size, the output directly followed by sentinels."""
    for rows in (7, 49):
        imgs, want = _want(rows, cols, 1000 * rows + cols)
        for form in (False, True):
            narrow(form)
            out, buf, s_out = _run(ctx, imgs[:1], rows, cols, 0, 0, 4)
            assert np.array_equal(out, want[:1]), "rows %d cols %d narrow=%s" % (rows, cols, form)
            _check_sentinels(buf, 1, rows * cols, s_out, 4)


@pytest.mark.parametrize("cols", [7, 8, 63, 253, 257, 501])
def test_blur_row_range_inside_the_image(ctx, narrow, cols):
    """Two views with a range each (49 rows: two chunks, one range crosses the chunk border, one lies in the second chunk):
    the rows of the range equal the oracle's, every other byte of the output keeps the sentinel."""
    rows = 49
    imgs, want = _want(rows, cols, 1000 * rows + cols)
    rr = np.array([[5, 31], [27, 49]], np.int32)
    t_rr = torch.from_numpy(rr).to(ctx.device)
    for form in (False, True):
        narrow(form)
        out, buf, s_out = _run(ctx, imgs[:2], rows, cols, 11, 3, 7, row_range=t_rr)
        for v in range(2):
            a, b = rr[v]
            assert np.array_equal(out[v, a:b], want[v, a:b]), "cols %d view %d narrow=%s" % (cols, v, form)
            assert (out[v, :a] == SENTINEL).all() and (out[v, b:] == SENTINEL).all(), "rows outside the range were written"
        _check_sentinels(buf, 2, rows * cols, s_out, 7)


def test_blur_dense_batch_tensor(ctx):
    """The [nimg, rows, cols] form of the call (default strides, output allocated by the call)."""
    imgs, want = _want(24, 257, 24257)
    out = ctx.gauss7(torch.from_numpy(imgs.copy()).to(ctx.device), 3, 24, 257)
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(3, 24, 257), want)
