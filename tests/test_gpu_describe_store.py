"""The per-keypoint loop of orb_describe_kernel after DESIGN.md section 31 (origins precomputed in LDS, the descriptor
stored by lane 0 as two 16-byte pieces at a 32-bit offset): ctx.describe_orb against oracle.orb_describe, byte for byte,
with a sentinel in every descriptor byte that must not be written.

One 96 x 160 noise image, with 1 and with 12 masks.  A launch has as many copies of the image as it takes to run the
256-thread instantiation (more than 1024 problems: the staged-region path) or a single copy (the 512-thread instantiation:
per-keypoint patches); the problems take the keypoint lists of SCENARIOS in turn and the oracle runs once per list.  On a
96 x 160 image every bounding box fits the staged region (at most 164 x 96 bytes of the 24 KB), so the repeat "with a
keypoint spread too wide for the region" needs a wider image: it runs on a 96 x 700 noise image, whose lists span 49 KB.
The global-memory fallback runs where edge < R + 1: edge = 19, the smallest the entry accepts, with the pattern scaled by
3/2 (R = 19 .. 23); the lists of that run keep R + 1 pixels from the border themselves."""
import numpy as np
import pytest
import torch

import oracle
from vo_single_camera_sos_amd import orb_pattern

pytestmark = pytest.mark.gpu

ROWS, COLS, WIDE_COLS, CAP, SENT = 96, 160, 700, 72, 0xA5
COUNTS = [0, 1, 3, 4, 5, 8, 9, 64, 65]     # the borders of the wave count (4) and of the old store lanes (4), a wave, a wave + 1


def _radius(pat, ca, sa):
    ca, sa = np.float32(ca), np.float32(sa)
    px, py = pat[:, 0].astype(np.float32), pat[:, 1].astype(np.float32)
    return int(max(np.abs(np.rint(px * ca - py * sa)).max(), np.abs(np.rint(px * sa + py * ca)).max()))


def region_bytes(k, R, rows, cols, edge=31):
    """LDS bytes of the staged region of a keypoint list: the kept keypoints' bounding box grown by R, rows an odd number of
    dwords apart (as the kernel lays it out)."""
    k = k[(k[:, 0] >= edge) & (k[:, 0] < cols - edge) & (k[:, 1] >= edge) & (k[:, 1] < rows - edge)]
    if len(k) == 0:
        return 0
    cx, cy = np.rint(k[:, 0]), np.rint(k[:, 1])
    rw, rh = int(np.ptp(cx)) + 2 * R + 1, int(np.ptp(cy)) + 2 * R + 1
    return 4 * (((rw + 3) >> 2) | 1) * rh


def scenarios(rng, rows, cols, margin):
    """Keypoint lists for an image whose keypoints survive from `margin` px off the border on: x in [margin, cols - margin),
    y in [margin, rows - margin)."""
    x0, x1, y0, y1 = margin, cols - margin - 1, margin, rows - margin - 1          # the extreme integer positions kept

    def rand(k, integer):
        xy = np.stack([rng.uniform(x0, x1, k), rng.uniform(y0, y1, k)], axis=1)
        return (xy.round() if integer else xy).astype(np.float32)
    out = [rand(m, i % 2 == 0) for i, m in enumerate(COUNTS)]
    dup = rand(4, True)
    out.append(dup[[0, 1, 0, 0, 2, 1, 3, 3, 3, 0]])                                    # duplicate keypoints
    corners = np.array([[x0, y0], [x1, y0], [x0, y1], [x1, y1]], np.float32)
    out.append(np.concatenate([corners, rand(3, False), corners[::-1]]))              # the four corners of the bounding box
    out.append(np.array([[x0 + 10.5, y0 + 1.5], [x0 + 11.5, y0 + 2.5], [x0 + 0.49, y0], [x1 + 0.49, y1 + 0.49]], np.float32))  # halves
    removed = rand(20, False)                                                          # the border rule removes every other one
    removed[0::4, 0] = x0 - 0.01
    removed[2::4, 1] = y1 + 1.0
    removed[6, 0] = x1 + 1.0
    out.append(removed)
    out.append(np.array([[x0 - 1.0, y0], [0.0, 0.0]], np.float32))                      # all removed
    return out


def _run(ctx, img, lists, NI, nmask, pat, angle, edge=31, row_range=None):
    """NI copies of img, NI * nmask problems with the lists in turn; row_range (lo, hi) restricts the first half of the images.
    Returns how many problems lost a keypoint."""
    rows, cols = img.shape
    P = NI * nmask
    ca, sa = orb_pattern.angle_cos_sin(angle)
    R = _radius(pat, ca, sa)
    blurred = oracle.gauss7(img)
    want = [oracle.orb_describe(blurred, k, ca, sa, pat, edge=edge) for k in lists]
    kp = np.zeros((P, CAP, 2), np.float32)
    n = np.zeros(P, np.int32)
    for p in range(P):
        k = lists[p % len(lists)]
        kp[p, :len(k)] = k
        n[p] = len(k)
    dev = ctx.device
    t_img = torch.from_numpy(img).to(dev)[None].expand(NI, rows, cols).contiguous()
    t_kp, t_n, t_pat = torch.from_numpy(kp.copy()).to(dev), torch.from_numpy(n.copy()).to(dev), torch.from_numpy(pat).to(dev)
    t_rr = None
    if row_range is not None:
        t_rr = torch.from_numpy(np.array([list(row_range), [0, rows]], np.int32)).to(dev)
    big = torch.full((P + 1, CAP, 32), SENT, dtype=torch.uint8, device=dev)
    ctx.describe_orb(t_img, t_kp, t_n, nmask, t_pat, ca, sa, edge=edge, desc=big[:P], row_range=t_rr)
    ctx.synchronize()
    desc, kp_out, n_out = big.cpu().numpy(), t_kp.cpu().numpy(), t_n.cpu().numpy()
    assert (desc[P] == SENT).all(), "bytes after the last problem were written"
    shorter = 0
    for p in range(P):
        wd, kept = want[p % len(lists)]
        k = lists[p % len(lists)]
        if row_range is not None and p // nmask < NI // 2:
            lo, hi = row_range
            y = np.rint(k[kept, 1]).astype(int)
            ok = (y - R >= (0 if lo <= 0 else lo + 3)) & (y + R <= (rows if hi >= rows else hi - 3) - 1)
            wd, kept = wd[ok], kept[ok]
        m = len(kept)
        shorter += m < len(k)
        assert n_out[p] == m, p
        assert np.array_equal(kp_out[p, :m], k[kept]), p
        assert np.array_equal(desc[p, :m], wd), p
        assert (desc[p, m:] == SENT).all(), "problem %d: a descriptor row at or beyond m = %d was written" % (p, m)
    return shorter


@pytest.fixture(scope="module")
def noise():
    rng = np.random.default_rng(31)
    return rng.integers(0, 256, (ROWS, COLS), dtype=np.uint8), rng.integers(0, 256, (ROWS, WIDE_COLS), dtype=np.uint8)


@pytest.mark.parametrize("nmask", [1, 12])
@pytest.mark.parametrize("angle", [17.0, 233.0])
def test_staged_region(ctx, noise, nmask, angle):
    rng = np.random.default_rng(int(angle) + nmask)
    NI = 1026 if nmask == 1 else 86                                                    # 1026 and 1032 problems: 256 threads
    lists = scenarios(rng, ROWS, COLS, 31)
    R = _radius(orb_pattern.orb_pattern(), *orb_pattern.angle_cos_sin(angle))
    assert max(region_bytes(k, R, ROWS, COLS) for k in lists) <= 24576
    assert _run(ctx, noise[0], lists, NI, nmask, orb_pattern.orb_pattern(), angle) > 0


@pytest.mark.parametrize("nmask", [1, 12])
def test_staged_region_with_a_row_range(ctx, noise, nmask):
    """The first half of the images has blurred rows 20 .. 79 only: keypoints near the range's ends go, after the border rule."""
    rng = np.random.default_rng(50 + nmask)
    NI = 1026 if nmask == 1 else 86
    lists = scenarios(rng, ROWS, COLS, 31)
    plain = _run(ctx, noise[0], lists, NI, nmask, orb_pattern.orb_pattern(), 17.0)
    assert _run(ctx, noise[0], lists, NI, nmask, orb_pattern.orb_pattern(), 17.0, row_range=(20, 80)) > plain


@pytest.mark.parametrize("nmask", [1, 12])
def test_one_image_runs_the_patches_of_the_wider_workgroup(ctx, noise, nmask):
    rng = np.random.default_rng(60 + nmask)
    _run(ctx, noise[0], scenarios(rng, ROWS, COLS, 31), 1, nmask, orb_pattern.orb_pattern(), 17.0)
    _run(ctx, noise[0], scenarios(rng, ROWS, COLS, 31), 2, nmask, orb_pattern.orb_pattern(), 90.0, row_range=(20, 80))


@pytest.mark.parametrize("nmask", [1, 12])
def test_spread_too_wide_for_the_region_runs_the_patches(ctx, noise, nmask):
    rng = np.random.default_rng(70 + nmask)
    NI = 1026 if nmask == 1 else 86
    lists = scenarios(rng, ROWS, WIDE_COLS, 31)
    R = _radius(orb_pattern.orb_pattern(), *orb_pattern.angle_cos_sin(17.0))
    assert sum(region_bytes(k, R, ROWS, WIDE_COLS) > 24576 for k in lists) >= 5    # (the others still fit: both paths in one launch)
    _run(ctx, noise[1], lists, NI, nmask, orb_pattern.orb_pattern(), 17.0)
    _run(ctx, noise[1], lists, NI, nmask, orb_pattern.orb_pattern(), 17.0, row_range=(20, 80))


@pytest.mark.parametrize("NI,nmask", [(86, 12), (1, 12), (1026, 1)])
def test_edge_below_the_pattern_radius_reads_the_image(ctx, noise, NI, nmask):
    rng = np.random.default_rng(80 + NI)
    pat = np.rint(1.5 * orb_pattern.orb_pattern().astype(np.float32)).astype(np.int8)
    ca, sa = orb_pattern.angle_cos_sin(0.0)
    R, edge = _radius(pat, ca, sa), 19
    assert edge < R + 1 <= 24
    lists = scenarios(rng, ROWS, COLS, R + 1)[:-2]            # (every keypoint R + 1 px inside: nothing reads past the image)
    lists[0] = np.concatenate([lists[4], np.array([[3.0, 3.0], [COLS - 2.0, 40.0]], np.float32), lists[3]])   # two go
    assert _run(ctx, noise[0], lists, NI, nmask, pat, 0.0, edge=edge) > 0
