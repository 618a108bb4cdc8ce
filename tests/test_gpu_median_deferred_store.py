"""The median kernel stores a row's gray byte one row step late: at the top of the next step, and
the last output row after the loop.  Small shapes at which that can go wrong -- a missing flush, a flush of a row that was
never computed, a store one row off, a flush into the neighbouring image -- bit for bit against the CPU oracle."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

COLS = (1, 53, 54, 55, 109)    # K = 11 (54 output columns per wave): a partial strip, one strip - 1 / exactly / + 1, two + 1
PSHAPE = (40, 60)


def _to(dev, *arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


@pytest.mark.parametrize("k", [3, 5, 11])
def test_plain_every_loop_end(ctx, k):
    """Plain form: the loop walks rows + 2 R source rows in groups of K, so these row counts end it at every position of
    the unrolled group; two images per call (a flush must not land in the neighbour)."""
    rng = np.random.default_rng(100 + k)
    for rows in sorted({1, 2, k - 1, k, k + 1, 2 * k, 2 * k + 1, 23}):
        for cols in COLS:
            imgs = rng.integers(0, 256, (2, rows, cols, 3), dtype=np.uint8)
            (t,) = _to(ctx.device, imgs)
            gray = ctx.median_gray(t, k)
            ctx.synchronize()
            gray = gray.cpu().numpy()
            for i in range(2):
                assert np.array_equal(gray[i], oracle.median_gray(imgs[i], k)), (rows, cols, i)


@pytest.fixture(scope="module")
def fused_case():
    rng = np.random.default_rng(22)
    omni = rng.integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)
    mx = rng.uniform(-2, 55, (2,) + PSHAPE).astype(np.float32)
    my = rng.uniform(-2, 39, (2,) + PSHAPE).astype(np.float32)
    pano = [[oracle.unwrap(omni[f], None, mx[v], my[v]) for f in range(3)] for v in range(2)]
    want = {k: np.stack([np.stack([oracle.median_gray(pano[v][f], k) for f in range(3)]) for v in range(2)]) for k in (3, 5, 11)}
    return omni, mx, my, want


def _ranges():
    out = [[lo, lo + n] for lo in (0, 3) for n in list(range(1, 13)) + [22, 23]]   # every residue of len + 2 R mod K
    return out + [[39, 40], [28, 40], [9, 9], [20, 10]]                           # the last row(s), empty, reversed


@pytest.mark.parametrize("k", [3, 5, 11])
def test_fused_row_ranges(ctx, fused_case, k):
    """Fused form with per-view row ranges: inside a range the oracle chain's bytes, outside the caller's 77s; the two
    views get different ranges in one call; the shared-device hint changes nothing."""
    omni, mx, my, want = fused_case
    t_omni, t_mx, t_my = _to(ctx.device, omni, mx, my)
    table = ctx.unwrap_prepare(None, t_mx, t_my, (37, 53))
    full = ctx.unwrap_median_gray(t_omni, table, k)
    ctx.synchronize()
    assert np.array_equal(full.cpu().numpy().reshape(2, 3, *PSHAPE), want[k])
    ranges = _ranges()
    try:
        for hint in (False, True):
            ctx.set_hint_shared_device(hint)
            for i, r0 in enumerate(ranges):
                pair = [r0, ranges[(i + 5) % len(ranges)]]
                rr = torch.tensor(pair, dtype=torch.int32, device=ctx.device)
                out = torch.full_like(full, 77)
                ctx.unwrap_median_gray(t_omni, table, k, gray=out, row_range=rr)
                ctx.synchronize()
                o = out.cpu().numpy().reshape(2, 3, *PSHAPE)
                for v in range(2):
                    lo = max(0, min(PSHAPE[0], pair[v][0]))
                    hi = max(lo, min(PSHAPE[0], pair[v][1]))
                    assert np.array_equal(o[v, :, lo:hi], want[k][v, :, lo:hi]), (hint, pair, v)
                    assert (o[v, :, :lo] == 77).all() and (o[v, :, hi:] == 77).all(), (hint, pair, v)
    finally:
        ctx.set_hint_shared_device(False)
