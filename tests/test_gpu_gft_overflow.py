"""GPU: sosvo_detect_gft on problems with MORE candidates than the selection sorts (CAND = 4096 for cap <= 1024, 16384
above).  The rule (include/sosvo.h): the kept set is the CAND largest sort keys -- descending response, higher address
first among equal responses -- so kp, n and their order depend on the image, the mask and the parameters only, and the
result is goodFeaturesToTrack on those candidates: a prefix of the unlimited result, and the unlimited result itself when
the budget is reached inside the cut.  Every case compares kp[:n], n and status bit 0 with
oracle.gft_select(..., cand_cap=CAND) bit for bit (the oracle's cut is pinned against a numpy restatement in
test_oracle_gft_candidate_cap.py) and first asserts from the oracle's candidate count that it is in the regime it names."""
import numpy as np
import pytest

import oracle
from test_gpu_detect import _sector_masks
from test_gpu_image import _textured, _to

pytestmark = pytest.mark.gpu

TILE = np.array([[255, 0, 0, 0], [255, 0, 0, 0], [255, 255, 0, 255]], dtype=np.uint8)   # every pixel a 3x3 maximum


def _want(eig, bits, m, quality, min_distance, max_corners, cap):
    """-> (capped oracle result cut to cap, unlimited oracle result cut to cap, number of candidates)."""
    cand = oracle.gft_cand_cap(cap)
    capped, _, count = oracle.gft_select(eig, bits, m, quality, min_distance, max_corners, cand_cap=cand, with_count=True)
    full, _ = oracle.gft_select(eig, bits, m, quality, min_distance, max_corners)
    return capped[:cap], full[:cap], count


def _detect(ctx, img, bits, nimg, nmask, cap, **kw):
    t_img, t_bits = _to(ctx.device, img, bits)
    kp, n, status = ctx.detect_gft(t_img, t_bits, nimg, nmask, cap, **kw)
    ctx.synchronize()
    return kp.cpu().numpy(), n.cpu().numpy(), status.cpu().numpy()


@pytest.fixture(scope="module")
def noise():
    """White noise 200 x 420, seed 77: 5531 candidates at quality 1e-4 -> (image [1, rows, cols], eig, whole-image mask)."""
    img = np.random.default_rng(77).integers(0, 256, (1, 200, 420), dtype=np.uint8)
    return img, oracle.min_eigen(img[0]), np.ones((1, 200, 420), dtype=np.uint32)


def test_budget_reached_inside_the_cut_gives_the_unlimited_result(ctx, noise):
    """5531 candidates, 4096 kept, the capacity of 512 corners reached after ~700 of them."""
    img, eig, bits = noise
    capped, full, count = _want(eig, bits[0], 0, 1e-4, 5.0, 0, 512)
    assert count == 5531 and len(capped) == len(full) == 512
    kp, n, status = _detect(ctx, img, bits, 1, 1, 512, quality=1e-4, min_distance=5.0, max_corners=0)
    assert status[0] == 1 and n[0] == 512
    assert np.array_equal(kp[0, :512], capped) and np.array_equal(kp[0, :512], full)


def test_the_cut_shows_and_gives_a_prefix(ctx, noise):
    """No budget, minDistance 9: the greedy pass runs through all 4096 kept candidates and ends with fewer corners than the
    unlimited pass over 5531 (the counts are the oracle's, taken here)."""
    img, eig, bits = noise
    capped, full, count = _want(eig, bits[0], 0, 1e-4, 9.0, 0, 1024)
    assert count > 4096 and 0 < len(capped) < len(full) < 1024 and np.array_equal(full[: len(capped)], capped)
    kp, n, status = _detect(ctx, img, bits, 1, 1, 1024, quality=1e-4, min_distance=9.0, max_corners=0)
    assert status[0] == 1 and n[0] == len(capped) and n[0] < len(full)
    assert np.array_equal(kp[0, : n[0]], capped)


def _plateau_image():
    """176 x 160, gray 90: noise in rows 0 .. 95, the periodic tile in rows 104 .. 169, columns 8 .. 151."""
    img = np.full((1, 176, 160), 90, dtype=np.uint8)
    img[0, :96] = np.random.default_rng(5).integers(0, 256, (96, 160), dtype=np.uint8)
    img[0, 104:170, 8:152] = np.tile(TILE, (22, 36))
    return img


def test_cut_inside_a_run_of_tied_responses(ctx):
    """Fewer than 4096 candidates are stronger than the plateau of the periodic tile and more than 4096 are at least as
    strong: the 4096th key lies inside the plateau, where the address decides -- the kept plateau pixels are the highest
    addresses (the radix select goes on into the address digits)."""
    img = _plateau_image()
    eig, bits = oracle.min_eigen(img[0]), np.ones(img.shape, dtype=np.uint32)
    plateau = eig[130, 80]
    assert plateau > 0 and (eig[110:164, 14:146] == plateau).all()
    cands, _, count = oracle.gft_select(eig, bits[0], 0, 1e-4, 0.0, 0, with_count=True)       # minDistance 0: all candidates
    v = eig[cands[:, 1].astype(int), cands[:, 0].astype(int)]
    stronger, tied = int((v > plateau).sum()), int((v == plateau).sum())
    assert count == len(cands) and stronger < 4096 < stronger + tied and count > stronger + tied
    capped, full, _ = _want(eig, bits[0], 0, 1e-4, 5.0, 0, 1024)
    assert 0 < len(capped) < len(full) < 1024
    kp, n, status = _detect(ctx, img, bits, 1, 1, 1024, quality=1e-4, min_distance=5.0, max_corners=0)
    assert status[0] == 1 and n[0] == len(capped)
    assert np.array_equal(kp[0, : n[0]], capped)


def test_whole_frame_of_tied_responses(ctx):
    """A frame covered by the periodic tile (image 1 of test_detect_gft_on_a_patch_where_every_pixel_is_a_maximum): all
    candidates but the border's are tied, far more than 4096 of them."""
    rows, cols = 120, 256
    img = np.tile(TILE, (rows // 3 + 1, cols // 4 + 1))[None, :rows, :cols]
    eig, bits = oracle.min_eigen(img[0]), np.ones(img.shape, dtype=np.uint32)
    capped, full, count = _want(eig, bits[0], 0, 0.01, 5.0, 0, 1024)
    assert count > 4 * 4096 and 0 < len(capped) < len(full)
    kp, n, status = _detect(ctx, img, bits, 1, 1, 1024, quality=0.01, min_distance=5.0, max_corners=0)
    assert status[0] == 1 and n[0] == len(capped)
    assert np.array_equal(kp[0, : n[0]], capped)


@pytest.mark.parametrize("min_distance", [5.0, 11.0])
def test_large_variant(ctx, min_distance):
    """cap = 2048 (16384 candidates kept) on white noise 480 x 640, seed 77: 20285 candidates at quality 1e-4.
    minDistance 5: the 2048 corners are reached inside the cut (the capped pass would go on to 6100, the unlimited one to
    6721).  minDistance 11, chosen on the CPU: 1505 corners from the kept 16384 against 1547 from all -- below the capacity,
    so the cut shows."""
    img = np.random.default_rng(77).integers(0, 256, (1, 480, 640), dtype=np.uint8)
    eig, bits = oracle.min_eigen(img[0]), np.ones(img.shape, dtype=np.uint32)
    capped, full, count = _want(eig, bits[0], 0, 1e-4, min_distance, 0, 2048)
    assert count > 16384
    if min_distance == 5.0:
        assert len(capped) == len(full) == 2048 and np.array_equal(capped, full)
    else:
        assert 0 < len(capped) < len(full) < 2048
    kp, n, status = _detect(ctx, img, bits, 1, 1, 2048, quality=1e-4, min_distance=min_distance, max_corners=0)
    assert status[0] == 1 and n[0] == len(capped)
    assert np.array_equal(kp[0, : n[0]], capped)


def test_mixed_launch_through_the_two_pass_scheme(ctx):
    """One call of 4 images x 3 masks, mask 0 the whole image: the noise images' whole-image problems have more than 4096
    candidates (second pass, overflow path), the texture images' between 2048 and 4096 (second pass, no overflow), every
    sector fewer than 2048 (first pass).  Status bit 0 exactly on the problems above 4096."""
    rng = np.random.default_rng(606)
    shape, nmask, cap, q = (200, 420), 3, 1024, 0.003
    imgs = np.stack([rng.integers(0, 256, shape, dtype=np.uint8), oracle.median_gray(_textured(rng, shape + (3,)), 5),
                     rng.integers(0, 256, shape, dtype=np.uint8), oracle.median_gray(_textured(rng, shape + (3,)), 5)])
    bits = (_sector_masks(shape[0], shape[1], nmask, rng) | np.uint32(1))[None]
    want, counts = [], []
    for i in range(4):
        eig = oracle.min_eigen(imgs[i])
        for m in range(nmask):
            capped, _, count = _want(eig, bits[0], m, q, 9.0, 0, cap)
            want.append(capped)
            counts.append(count)
    counts = np.array(counts)
    assert (counts < 2048).any() and ((counts > 2048) & (counts <= 4096)).any() and (counts > 4096).any(), counts
    kp, n, status = _detect(ctx, imgs, bits, 4, nmask, cap, quality=q, min_distance=9.0, max_corners=0)
    assert np.array_equal(status, (counts > 4096).astype(status.dtype)), (status, counts)
    for p in range(4 * nmask):
        assert n[p] == len(want[p]), (p, n[p], len(want[p]), counts[p])
        assert np.array_equal(kp[p, : n[p]], want[p]), p


def test_overflow_in_a_launch_of_more_than_1024_problems(ctx):
    """33 images x 32 masks, every mask the whole image: 1056 problems, the 256-thread instances; one distinct image
    (noise 176 x 420: more than 4096 candidates), so every problem must give the one capped oracle result."""
    nimg, nmask, cap = 33, 32, 1024
    img = np.random.default_rng(33).integers(0, 256, (1, 176, 420), dtype=np.uint8)
    bits = np.full(img.shape, 0xFFFFFFFF, dtype=np.uint32)
    capped, full, count = _want(oracle.min_eigen(img[0]), bits[0], 0, 1e-4, 9.0, 0, cap)
    assert count > 4096 and 0 < len(capped) < len(full) < cap
    kp, n, status = _detect(ctx, np.repeat(img, nimg, axis=0), bits, nimg, nmask, cap, quality=1e-4, min_distance=9.0, max_corners=0)
    assert (status == 1).all() and (n == len(capped)).all()
    assert (kp[:, : len(capped)] == capped[None]).all()


def test_overflowed_call_is_repeatable(ctx, noise):
    """The call of test_the_cut_shows_and_gives_a_prefix five times into fresh outputs, the scratch filled with 0xFF in
    between: kp, n and status byte-identical (which wave reaches the slot counter first must not matter)."""
    img, _, bits = noise
    t_img, t_bits = _to(ctx.device, img, bits)
    outs = []
    for _ in range(5):
        ctx.debug_fill_scratch(0xFF)
        kp, n, status = ctx.detect_gft(t_img, t_bits, 1, 1, 1024, quality=1e-4, min_distance=9.0, max_corners=0)
        ctx.synchronize()
        outs.append((kp.cpu().numpy().tobytes(), n.cpu().numpy().tobytes(), status.cpu().numpy().tobytes()))
    assert status.cpu().numpy()[0] == 1 and n.cpu().numpy()[0] > 0
    for k in range(1, 5):
        assert outs[k] == outs[0], k
