"""GPU: the switch points of the Lucas-Kanade window kernels, sosvo_track_lk against tests/reflk.py / reflk_cyclic.py and
sosvo_refine_subpix against tests/refsubpix.py bit for bit, on the cases of tests/lk_lattice_cases.py (whose content
tests/test_lk_lattice_reference.py vouches for on the CPU):

- every window on every depth: half 2 .. 10 x 1 .. 4 levels, counts (24, 1, 5, 0); half 5 and 6 -- the two sides of the switch
  between the 16-lane and the whole-wave mapping -- also with the forward-backward check and the initial-flow flag;
- later rounds of the keypoint loop with a ragged last one: the whole-wave form (half 6, 10) on counts (80, 65, 64, 0), the
  16-lane form (half 2, 5) on (300, 257, 256, 1), each with and without the forward-backward check;
- the grid of 4096 problems (16 rows: two rounds at half 4, five at half 6), eight of them non-empty, two naming an image that
  does not exist;
- tiny images: 5 x 40, 40 x 5, 9 x 12 and the one-row, one-column and 1 x 1 images, half 2, 5, 6, 10 at 1 and 4 levels;
- cyclic columns: half 5 and 6 at the seam, a later-rounds case per mapping with the check, the grid of 4096 problems;
- sosvo_refine_subpix on 4096 problems (16 rows), half 2 and 5.

next / err / back are compared as uint32 bit patterns and the status as bytes over the WHOLE buffers, which start as sentinels
(-123.25, 0xA5): rows at and beyond n[p], and problems that are empty or have no image, must hold them still."""
import numpy as np
import pytest
import torch

import lk_lattice_cases as cases

pytestmark = pytest.mark.gpu


def _dev(ctx, a):
    return torch.from_numpy(np.array(a)).to(ctx.device)       # (a copy: the cases' arrays are read-only)


def _device_track(ctx, case):
    """-> (next, status, err[, back]) as numpy; every output buffer starts as case.sentinels()."""
    pyr = (ctx.gray_pyramid_cyclic if case.cyclic else ctx.gray_pyramid)(_dev(ctx, case.gray), case.levels)
    out = tuple(_dev(ctx, a) for a in case.sentinels())
    res = ctx.track_lk(pyr, _dev(ctx, case.prev_img), _dev(ctx, case.next_img), _dev(ctx, case.pts), _dev(ctx, case.n), half=case.half,
                       max_iter=cases.MAX_ITER, next_pts=out[0] if case.guess is not None else None, fb_max=case.fb_max, out=out)
    ctx.synchronize()
    return tuple(t.cpu().numpy() for t in res)


def _assert_equal(got, want, what):
    """Whole buffers; the first differing (problem, row[, axis]) with (got, want) is what a failure prints."""
    assert len(got) == len(want)
    for g, w, name in zip(got, want, ("next", "status", "err", "back")):
        g, w = (a if a.dtype == np.uint8 else np.ascontiguousarray(a).view(np.uint32) for a in (g, w))
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, name, len(bad), [(tuple(b), g[tuple(b)], w[tuple(b)]) for b in bad[:4]])


def _compare(ctx, case):
    _assert_equal(_device_track(ctx, case), cases.track_reference(case), case)


# ---- every window on every depth ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", cases.LATTICE_LEVELS)
@pytest.mark.parametrize("half", cases.LATTICE_HALVES)
def test_lattice_cell_equals_the_reference(ctx, half, levels):
    _compare(ctx, cases.lattice_case(half, levels))


@pytest.mark.parametrize("variant", ["fb", "guess"])
@pytest.mark.parametrize("levels", cases.LATTICE_LEVELS)
@pytest.mark.parametrize("half", [5, 6])
def test_lattice_cell_at_the_switch_with_the_check_and_the_flag(ctx, half, levels, variant):
    _compare(ctx, cases.lattice_case(half, levels, variant))


# ---- later rounds ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [False, True], ids=["forward", "fb"])
@pytest.mark.parametrize("half,levels", cases.ROUNDS)
def test_later_rounds_equal_the_reference(ctx, half, levels, fb):
    _compare(ctx, cases.rounds_case(half, levels, fb))


# ---- the wide grid -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half,cyclic", [(4, False), (6, False), (6, True)], ids=["half4", "half6", "half6-cyclic"])
def test_wide_grid_equals_the_reference(ctx, half, cyclic):
    case = cases.wide_case(half, cyclic)
    got = _device_track(ctx, case)
    _assert_equal(got, cases.track_reference(case), case)
    rest = np.ones(case.nprob, bool)
    rest[case.live] = False                                  # the empty problems and the two without an image: untouched
    assert rest.sum() == 4088 and (case.n[rest] > 0).sum() == 2
    for g, s in zip(got, case.sentinels()):
        assert np.array_equal(g[rest].view(np.uint8), s[rest].view(np.uint8))


# ---- tiny images ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", cases.TINY_LEVELS)
@pytest.mark.parametrize("half", cases.TINY_HALVES)
@pytest.mark.parametrize("shape", cases.TINY_TEXTURED + cases.TINY_FLAT, ids=lambda s: "%dx%d" % s)
def test_tiny_image_equals_the_reference(ctx, shape, half, levels):
    case = cases.tiny_case(shape, half, levels)
    got = _device_track(ctx, case)
    _assert_equal(got, cases.track_reference(case), case)
    if shape in cases.TINY_FLAT:                             # det == 0 everywhere: status 0, err 0, the position as the rule leaves it
        assert not got[1].any() and not got[2].any()


# ---- cyclic columns ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half,levels", cases.CYCLIC_CELLS)
def test_cyclic_cell_equals_the_reference(ctx, half, levels):
    _compare(ctx, cases.cyclic_case(half, levels))


@pytest.mark.parametrize("half,levels,cap,count", cases.CYCLIC_ROUNDS)
def test_cyclic_later_rounds_equal_the_reference(ctx, half, levels, cap, count):
    _compare(ctx, cases.cyclic_rounds_case(half, levels, cap, count))


# ---- sosvo_refine_subpix on 4096 problems ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", cases.SUBPIX_HALVES)
def test_subpix_wide_grid_equals_the_reference(ctx, half):
    gray, kp, n = cases.subpix_wide_inputs()
    d_kp, d_n = _dev(ctx, kp), _dev(ctx, n)
    ctx.refine_subpix(_dev(ctx, gray), d_kp, d_n, cases.SUBPIX_NMASK, half=half, max_iter=cases.MAX_ITER)
    ctx.synchronize()
    got, want = d_kp.cpu().numpy().view(np.uint32), cases.subpix_wide_reference(half).view(np.uint32)
    assert np.array_equal(d_n.cpu().numpy(), n)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (half, len(bad), [(tuple(b), got[tuple(b)], want[tuple(b)]) for b in bad[:4]])
