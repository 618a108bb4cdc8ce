"""sosvo_describe_orb with the rotated pattern taken from the per-call table (orb_pattern_table_kernel) instead of being
re-derived by every workgroup: all three workgroup sizes and all three paths of orb_describe_kernel against the oracle,
bit for bit, and the table's lifetime (one call).  Launches of many problems repeat a few distinct (image, keypoints)
pairs; the oracle runs once per distinct pair, every problem of the launch is compared.

(A call captured into a graph and replayed is covered at the pipeline level by tests/test_gpu_graph_replay.py, which
runs this entry point inside capture_graph; a second fixture of that size is not repeated here.)"""
import numpy as np
import pytest
import torch

import oracle
from test_gpu_image import _textured, _to
from vo_single_camera_sos_amd import orb_pattern

pytestmark = pytest.mark.gpu

ANGLES = [0.0, 17.0, 90.0, 233.0]


def _radius(pat, ca, sa):
    ca, sa = np.float32(ca), np.float32(sa)
    px, py = pat[:, 0].astype(np.float32), pat[:, 1].astype(np.float32)
    return int(max(np.abs(np.rint(px * ca - py * sa)).max(), np.abs(np.rint(px * sa + py * ca)).max()))


def _keypoints(rng, D, nmask, cap, n_lo, rows, cols, box=None):
    """D x nmask keypoint lists: integer and fractional coordinates, a few inside the border (they are removed); box(m) ->
    (x0, x1) keeps the keypoints of mask m together (one staged region)."""
    kp = np.zeros((D, nmask, cap, 2), np.float32)
    n = rng.integers(n_lo, cap + 1, (D, nmask)).astype(np.int32)
    n[0, 0] = cap
    if D * nmask > 1:
        n[-1, -1] = 0
    for d in range(D):
        for m in range(nmask):
            x0, x1 = box(m) if box else (31, cols - 31)
            k = n[d, m]
            xy = np.stack([rng.uniform(x0, x1, k), rng.uniform(31, rows - 31.5, k)], axis=1)
            if (d + m) % 2:
                xy = xy.round()
            kp[d, m, :k] = xy
            if k >= 4 and not box:
                kp[d, m, :4] = [[31.0, 31.0], [30.99, 60.0], [cols - 31.0, 60.0], [cols - 31.01, rows - 31.01]]
    return kp, n


def _describe_and_compare(ctx, imgs, kp, n, NI, pat, angle, edge=31, t_pat=None):
    """imgs [D, rows, cols], kp [D, nmask, cap, 2], n [D, nmask]: a launch of NI images x nmask masks (the distinct ones in
    turn) against the oracle.  Returns the number of descriptors compared."""
    D, nmask, cap = kp.shape[:3]
    src = np.arange(NI) % D
    ca, sa = orb_pattern.angle_cos_sin(angle)
    t_img, t_kp, t_n = _to(ctx.device, imgs[src], kp[src].reshape(NI * nmask, cap, 2), n[src].reshape(-1))
    if t_pat is None:
        t_pat, = _to(ctx.device, pat)
    desc = ctx.describe_orb(t_img, t_kp, t_n, nmask, t_pat, ca, sa, edge=edge)
    ctx.synchronize()
    desc, kp_out, n_out = desc.cpu().numpy(), t_kp.cpu().numpy(), t_n.cpu().numpy()
    want = {}
    for d in range(D):
        blurred = oracle.gauss7(imgs[d])
        for m in range(nmask):
            want[d, m] = oracle.orb_describe(blurred, kp[d, m, : n[d, m]], ca, sa, pat, edge=edge)
    total = 0
    for i in range(NI):
        for m in range(nmask):
            (wd, kept), p = want[src[i], m], i * nmask + m
            assert n_out[p] == len(kept), (i, m)
            assert np.array_equal(kp_out[p, : len(kept)], kp[src[i], m, kept]), (i, m)
            assert np.array_equal(desc[p, : len(kept)], wd), (i, m)
            total += len(kept)
    return total


def _images(rng, D, rows, cols):
    return np.stack([oracle.median_gray(_textured(rng, (rows, cols, 3)), 0) for _ in range(D)])


@pytest.mark.parametrize("angle", ANGLES)
def test_staged_region_of_a_many_problem_launch(ctx, angle):
    """1056 problems (256 threads); each mask's keypoints lie in a box of 40 columns: one staged region of < 24 KB."""
    rng = np.random.default_rng(int(angle) + 1)
    rows, cols, nmask, cap = 100, 200, 8, 48
    kp, n = _keypoints(rng, 3, nmask, cap, 8, rows, cols, box=lambda m: (31 + 14 * m, 71 + 14 * m))
    assert _describe_and_compare(ctx, _images(rng, 3, rows, cols), kp, n, 132, orb_pattern.orb_pattern(), angle) > 20000


@pytest.mark.parametrize("angle", ANGLES)
def test_per_keypoint_patches_of_a_many_problem_launch(ctx, angle):
    """1032 problems (256 threads) whose keypoints spread over a whole 146 x 1440 panorama: the region would exceed 24 KB, the
    waves fetch a patch per keypoint."""
    rng = np.random.default_rng(int(angle) + 2)
    rows, cols, nmask, cap = 146, 1440, 8, 24
    kp, n = _keypoints(rng, 2, nmask, cap, 6, rows, cols)
    assert _describe_and_compare(ctx, _images(rng, 2, rows, cols), kp, n, 129, orb_pattern.orb_pattern(), angle) > 8000


@pytest.mark.parametrize("angle", ANGLES)
def test_few_problems_and_large_capacity(ctx, angle):
    """12 problems (512 threads), and a capacity above 1024 (1024 threads)."""
    rng = np.random.default_rng(int(angle) + 3)
    rows, cols = 122, 400
    imgs = _images(rng, 3, rows, cols)
    kp, n = _keypoints(rng, 3, 4, 128, 0, rows, cols)
    assert _describe_and_compare(ctx, imgs, kp, n, 3, orb_pattern.orb_pattern(), angle) > 300
    kp, n = _keypoints(rng, 2, 1, 1100, 1050, rows, cols)       # (the second list is empty: _keypoints' last one)
    assert _describe_and_compare(ctx, imgs[:2], kp, n, 2, orb_pattern.orb_pattern(), angle) > 1000


@pytest.mark.parametrize("NI,nmask", [(132, 8), (3, 4)])
def test_pattern_beyond_the_patch_radius_reads_the_image(ctx, NI, nmask):
    """The pattern scaled by two: R > 23 with edge >= R + 1 -- neither a region nor a patch, the tests read the blurred image."""
    rng = np.random.default_rng(NI)
    rows, cols, cap, edge, angle = 120, 220, 32, 45, 17.0
    pat = (2 * orb_pattern.orb_pattern().astype(np.int16)).astype(np.int8)
    ca, sa = orb_pattern.angle_cos_sin(angle)
    R = _radius(pat, ca, sa)
    assert 23 < R <= edge - 1
    kp, n = _keypoints(rng, 2, nmask, cap, 4, rows, cols)
    kp[:, :, :, 0] = np.clip(kp[:, :, :, 0] + 10, 0, cols - 1)      # some inside the wider border, some not
    assert _describe_and_compare(ctx, _images(rng, 2, rows, cols), kp, n, NI, pat, angle, edge=edge) > 10 * nmask


def test_row_range_removes_a_keypoint(ctx):
    """row_range: a keypoint whose patch leaves the trustworthy blurred rows is removed (the radius comes from the table); the
    others keep the descriptors of the all-rows call."""
    rng = np.random.default_rng(5)
    NI, nmask, cap, rows, cols = 2, 2, 64, 146, 300
    imgs = _images(rng, NI, rows, cols)
    pat = orb_pattern.orb_pattern()
    ca, sa = orb_pattern.angle_cos_sin(233.0)
    R = _radius(pat, ca, sa)
    rr = np.array([[40, 120], [0, rows]], dtype=np.int32)
    kp = np.zeros((NI * nmask, cap, 2), np.float32)
    kp[:, :, 0] = rng.integers(31, cols - 31, (NI * nmask, cap))
    kp[:, :, 1] = rng.integers(31, rows - 31, (NI * nmask, cap))
    kp[0, :4, 1] = [40 + 3 + R, 40 + 3 + R - 1, 120 - 3 - 1 - R, 120 - 3 - R]
    n = np.full(NI * nmask, cap, np.int32)
    t_img, t_pat, t_rr = _to(ctx.device, imgs, pat, rr)
    t_kp_all, t_n_all = _to(ctx.device, kp.copy(), n.copy())
    d_all = ctx.describe_orb(t_img, t_kp_all, t_n_all, nmask, t_pat, ca, sa).cpu().numpy()
    kp_all, n_all = t_kp_all.cpu().numpy(), t_n_all.cpu().numpy()
    ctx.debug_fill_scratch(0xFF)
    t_kp, t_n = _to(ctx.device, kp.copy(), n.copy())
    d = ctx.describe_orb(t_img, t_kp, t_n, nmask, t_pat, ca, sa, row_range=t_rr).cpu().numpy()
    kp_o, n_o = t_kp.cpu().numpy(), t_n.cpu().numpy()
    for p in range(NI * nmask):
        lo, hi = rr[p // nmask]
        y = kp_all[p, : n_all[p], 1].astype(int)
        ok = (y - R >= (0 if lo == 0 else lo + 3)) & (y + R < (rows if hi == rows else hi - 3))
        assert n_o[p] == ok.sum(), p
        assert np.array_equal(kp_o[p, : n_o[p]], kp_all[p, : n_all[p]][ok]) and np.array_equal(d[p, : n_o[p]], d_all[p, : n_all[p]][ok])
    ys = kp_o[0, : n_o[0], 1]
    assert n_o[0] < n_all[0] and (40 + 3 + R) in ys and (40 + 3 + R - 1) not in ys and (120 - 3 - R) not in ys


def test_pattern_rewritten_in_place_between_calls(ctx):
    """Two calls on one context with the pattern rewritten AT THE SAME DEVICE ADDRESS and another angle in between: the second
    result is the second pattern's -- the table belongs to a call, nothing is kept under the pointer."""
    rng = np.random.default_rng(9)
    rows, cols = 100, 200
    imgs = _images(rng, 2, rows, cols)
    kp, n = _keypoints(rng, 2, 4, 64, 16, rows, cols)
    first = orb_pattern.orb_pattern()
    second = np.ascontiguousarray(first[::-1] * np.array([1, -1], np.int8))     # other tests, mirrored
    t_pat, = _to(ctx.device, first.copy())
    address = t_pat.data_ptr()
    assert _describe_and_compare(ctx, imgs, kp, n, 2, first, 17.0, t_pat=t_pat) > 100
    t_pat.copy_(torch.from_numpy(second))
    assert t_pat.data_ptr() == address
    assert _describe_and_compare(ctx, imgs, kp, n, 2, second, 90.0, t_pat=t_pat) > 100
    assert not np.array_equal(first, second)
