"""The median kernel's rank bookkeeping at its decision boundary: windows whose count of ones at a bit plane is exactly
the number of elements ranked above the median (the wanted bit is 0) or one more (it is 1), at every plane, for
ksize 3 / 5 / 11, in the plain (BGR panorama) and the fused (unwrap table) form, against oracle.median_gray.

With values p(y, x) = (x + K y) mod K^2, every K x K window holds each residue once, so "p < t" has exactly t ones in every
window away from the replicated border: t = K^2 / 2 splits at the rank with the median's bit 0, t + 1 with it 1."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu


def _split_images(k, rows, cols):
    """Two-valued images per (plane, side): channel c's two values differ only at bit b (c-dependent high bits shared),
    or at every bit (0 / 255); plus constant images."""
    y, x = np.mgrid[:rows, :cols]
    half = k * k // 2
    imgs = []
    for b in range(8):
        for t in (half, half + 1):
            img = np.empty((rows, cols, 3), np.uint8)
            for c in range(3):
                ones = ((x + k * y + 7 * c) % (k * k)) < t
                base = (0xA5 ^ (37 * c)) & ~(1 << b) & 0xFF
                img[..., c] = np.where(ones, base | (1 << b), base)
            imgs.append(img)
    for t in (half, half + 1):
        ones = ((x + k * y) % (k * k)) < t
        imgs.append(np.repeat(np.where(ones, 255, 0).astype(np.uint8)[..., None], 3, axis=2))
        imgs.append(np.repeat(np.where(ones, 0, 255).astype(np.uint8)[..., None], 3, axis=2))
    for v in (0, 255, 128, 127):
        imgs.append(np.full((rows, cols, 3), v, np.uint8))
    return np.stack(imgs)


@pytest.mark.parametrize("k", [3, 5, 11])
def test_median_plain_at_rank_split(ctx, k):
    imgs = _split_images(k, 29, 131)
    gray = ctx.median_gray(torch.from_numpy(imgs).to(ctx.device), k)
    ctx.synchronize()
    gray = gray.cpu().numpy()
    for i in range(imgs.shape[0]):
        assert np.array_equal(gray[i], oracle.median_gray(imgs[i], k)), i


@pytest.mark.parametrize("k", [3, 5, 11])
def test_median_fused_at_rank_split(ctx, k):
    """The fused form through an identity unwrap table (one tap of weight 1024 per pixel: the panorama is the frame; the
    last pixels of the frame take the table's edge entries), whole images and per-view row ranges."""
    rows, cols = 27, 118
    omni = _split_images(k, rows, cols)
    nf = omni.shape[0]
    yy, xx = np.mgrid[:rows, :cols].astype(np.float32)
    mx = np.stack([xx, xx])
    my = np.stack([yy, yy])
    dev = ctx.device
    t_omni = torch.from_numpy(omni).to(dev)
    table = ctx.unwrap_prepare(None, torch.from_numpy(mx).to(dev), torch.from_numpy(my).to(dev), (rows, cols))
    full = ctx.unwrap_median_gray(t_omni, table, k)
    ctx.synchronize()
    f = full.cpu().numpy().reshape(2, nf, rows, cols)
    for i in range(nf):
        want = oracle.median_gray(omni[i], k)
        assert np.array_equal(f[0, i], want) and np.array_equal(f[1, i], want), i
    for rr in ([[0, 1], [rows - 1, rows]], [[k // 2, rows - k // 2], [1, k]], [[5, 6], [0, rows]]):
        out = torch.full_like(full, 77)
        ctx.unwrap_median_gray(t_omni, table, k, gray=out, row_range=torch.tensor(rr, dtype=torch.int32, device=dev))
        ctx.synchronize()
        o = out.cpu().numpy().reshape(2, nf, rows, cols)
        for v in range(2):
            lo, hi = rr[v]
            assert np.array_equal(o[v, :, lo:hi], f[v, :, lo:hi]), (rr, v)
            assert (o[v, :, :lo] == 77).all() and (o[v, :, hi:] == 77).all(), (rr, v)
