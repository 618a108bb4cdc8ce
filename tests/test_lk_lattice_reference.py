"""CPU: the inputs of tests/test_gpu_lk_lattice.py and tests/test_gpu_stereo_lk_lattice.py (tests/lk_lattice_cases.py) through
the references alone, so that the device comparisons there cannot pass on inputs that exercise nothing:

- every cell of the lattice (half 2 .. 10 x 1 .. 4 levels) tracks at least 12 of its 30 points, and the lattice holds a status
  0 from a start off the image;
- every later-rounds case (plain, wide grid, cyclic) has a tracked, a lost and a skipped point at an index that only a later
  round of the keypoint loop reaches, and every forward-backward case clears a status the forward pass had set;
- the tiny textured images (5 x 40, 40 x 5, 9 x 12) track at least 4 of 16 points at every half and depth, the one-row,
  one-column and 1 x 1 images none (err 0, the position as the rule leaves it);
- the wide grid's problems without an image keep their sentinels;
- the stereo scene's cells accept most tracks; the gather case compacts more than 256 and fewer than n_bot rows of its big
  problem, drops a different number of rows in its rounds of 256, and tracks more than 256 (half 4) / 64 (half 6) points;
- the wide-grid sub-pixel case moves, leaves and skips points beyond the first round."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lk_lattice_cases as cases  # noqa: E402


def _kinds(case, ref, rows):
    """How many of the (problem, row) pairs the reference tracked, lost and skipped (a non-finite start)."""
    tracked = lost = skipped = 0
    for p, k in rows:
        if not np.isfinite(case.pts[p, k]).all():
            skipped += 1
            assert ref[1][p, k] == 0 and np.array_equal(ref[0][p, k].view(np.uint32), case.pts[p, k].view(np.uint32))
        elif ref[1][p, k]:
            tracked += 1
        else:
            lost += 1
    return tracked, lost, skipped


def _assert_later_rounds(case):
    ref = cases.track_reference(case)
    rows = cases.later_round_rows(case)
    kinds = _kinds(case, ref, rows)
    assert min(kinds) >= 1, (case, kinds)
    if case.fb_max is not None:
        fwd = cases.forward_status(case)
        assert ((fwd == 1) & (ref[1] == 0)).any(), case
        assert ((ref[1] == fwd) | (ref[1] == 0)).all(), case
        assert any(fwd[p, k] == 1 and ref[1][p, k] == 0 for p, k in rows), case             # ... one of a later round among them


@pytest.mark.parametrize("half", cases.LATTICE_HALVES)
def test_every_lattice_cell_tracks_points(half):
    for levels in cases.LATTICE_LEVELS:
        case = cases.lattice_case(half, levels)
        _, st, _ = cases.track_reference(case)
        assert sum(case.n) == 30
        tracked = sum(int(st[p, :c].sum()) for p, c in enumerate(case.n))
        assert tracked >= 12, (case, tracked)
        assert st[0, 12] == 0 and case.pts[0, 12, 1] < -0.5                  # the start off the image: lost in every cell
        assert (st[3] == cases.ST_SENTINEL).all() and (st[1, 1:] == cases.ST_SENTINEL).all()


@pytest.mark.parametrize("half", (5, 6))
def test_lattice_variants_act(half):
    for levels in cases.LATTICE_LEVELS:
        plain = cases.track_reference(cases.lattice_case(half, levels))
        fb = cases.lattice_case(half, levels, "fb")
        checked = cases.track_reference(fb)
        assert len(checked) == 4 and np.array_equal(cases.forward_status(fb), plain[1])
        assert ((checked[1] == plain[1]) | (checked[1] == 0)).all() and ((plain[1] == 1) & (checked[1] == 0)).any()
        guessed = cases.track_reference(cases.lattice_case(half, levels, "guess"))
        assert not np.array_equal(guessed[0].view(np.uint32), plain[0].view(np.uint32))
        assert guessed[1][0, 9] == 0                                         # the non-finite guess


@pytest.mark.parametrize("half,levels", cases.ROUNDS)
def test_later_rounds_hold_every_kind_of_point(half, levels):
    for fb in (False, True):
        case = cases.rounds_case(half, levels, fb)
        assert case.first_round == (256 if half <= 5 else 64) and max(case.n) > case.first_round
        assert sorted(int(c) - case.first_round for c in case.n if c > case.first_round)[0] == 1      # a ragged last round
        _assert_later_rounds(case)


@pytest.mark.parametrize("half,cyclic", [(4, False), (6, False), (6, True)])
def test_wide_grid_holds_every_kind_of_point(half, cyclic):
    case = cases.wide_case(half, cyclic)
    assert case.nprob == 4096 and case.first_round == (64 if half <= 5 else 16)
    assert case.live[0] == 0 and case.live[-1] == 4095 and len(case.live) == 8
    assert {int(case.n[p]) for p in case.live} == {80, 65, 17, 1}
    assert int((case.n > 0).sum()) == len(case.live) + len(cases.WIDE_NO_IMAGE)
    _assert_later_rounds(case)
    ref = cases.track_reference(case)
    rest = np.ones(case.nprob, bool)
    rest[case.live] = False
    for r, s in zip(ref, case.sentinels()):
        assert np.array_equal(r[rest].view(np.uint8), s[rest].view(np.uint8))


@pytest.mark.parametrize("shape", cases.TINY_TEXTURED + cases.TINY_FLAT, ids=lambda s: "%dx%d" % s)
def test_tiny_images(shape):
    for half in cases.TINY_HALVES:
        for levels in cases.TINY_LEVELS:
            case = cases.tiny_case(shape, half, levels)
            nxt, st, err = cases.track_reference(case)
            if shape in cases.TINY_TEXTURED:
                assert st[0].sum() >= 4, (case, st[0].sum())
            else:
                assert not st[0].any() and not err[0].any(), case
                fin = np.isfinite(case.pts[0]).all(axis=1)
                assert np.array_equal(nxt[0][fin].view(np.uint32), case.pts[0][fin].view(np.uint32)), case
    if shape in cases.TINY_FLAT:
        rows, cols = shape
        at = np.rint(case.pts[0] * 32)
        inside = (at[:, 0] >= 0) & (at[:, 0] <= 32 * (cols - 1)) & (at[:, 1] >= 0) & (at[:, 1] <= 32 * (rows - 1))
        assert inside.sum() >= 3                                              # (lost for want of texture, not for the start)


@pytest.mark.parametrize("half,levels", cases.CYCLIC_CELLS)
def test_cyclic_cells_track_across_the_seam(half, levels):
    case = cases.cyclic_case(half, levels)
    nxt, st, _ = cases.track_reference(case)
    for p in (0, 2):
        assert st[p, :24].sum() >= 20, (case, p)
        crossed = (np.abs(nxt[p, :24, 0] - case.pts[p, :24, 0]) > cases.COLS / 2) & (st[p, :24] == 1)
        assert crossed.sum() >= 3, (case, p)
    assert min(_kinds(case, (nxt, st), [(0, k) for k in range(24, 40)])) >= 1


@pytest.mark.parametrize("half,levels,cap,count", cases.CYCLIC_ROUNDS)
def test_cyclic_later_rounds_hold_every_kind_of_point(half, levels, cap, count):
    case = cases.cyclic_rounds_case(half, levels, cap, count)
    assert case.n[0] == count == case.first_round + 1 and case.cap == cap
    _assert_later_rounds(case)


@pytest.mark.parametrize("half", cases.STEREO_HALVES)
def test_stereo_cells_accept_tracks(half):
    case = cases.stereo_case(half)
    kp, st = cases.stereo_reference(case)
    assert st[0, :16].sum() >= 12 and st[4, :16].sum() >= 12
    moved = (kp.view(np.uint32) != case.kp_bot.view(np.uint32)).any(axis=2)
    assert np.array_equal(moved & (st == 1), moved) and moved.sum() >= 24


@pytest.mark.parametrize("half", cases.GATHER_HALVES)
def test_gather_case_carries_a_count_across_rounds(half):
    case = cases.gather_case(half)
    keep = cases.gathered(case, 0)
    assert len(keep) == 600 and 256 < keep.sum() < 600
    assert keep.sum() > (256 if half <= 5 else 64)                           # later rounds of the tracker behind the gather
    dropped = [int((~keep[q0:q0 + 256]).sum()) for q0 in range(0, 600, 256)]
    assert len(set(dropped[:2])) == 2 and min(dropped) > 0, dropped
    keys = case.keys[0, :600]
    assert (keys == 0xFFFFFFFF).sum() >= 30 and ((keys != 0xFFFFFFFF) & ((keys & 0xFFFFF) >= 40)).sum() >= 30
    kp, st = cases.stereo_reference(case)
    assert not st[0, :600][~keep].any() and not st[0, :600][keep].all()       # (max_shift turns some tracks down)
    assert st[0, :600].sum() > (256 if half <= 5 else 64)
    assert st[0, 256:600].any() and st[0, 512:600].any()
    assert cases.gathered(case, 1).sum() < 257 and cases.gathered(case, 2).sum() < 256 and case.n_bot[3] == 0


@pytest.mark.parametrize("half", cases.SUBPIX_HALVES)
def test_subpix_wide_case_moves_points_beyond_the_first_round(half):
    gray, kp, n = cases.subpix_wide_inputs()
    want = cases.subpix_wide_reference(half)
    assert len(n) == 4096 and [p for p, _ in cases.SUBPIX_LIVE][::7] == [0, 4095]
    assert {c for _, c in cases.SUBPIX_LIVE} == {80, 65, 17, 1} and int((n > 0).sum()) == 8
    moved = left = skipped = 0
    for p, c in cases.SUBPIX_LIVE:
        for k in range(cases.SUBPIX_FIRST_ROUND, c):
            if not np.isfinite(kp[p, k]).all():
                skipped += 1
            elif np.array_equal(want[p, k], kp[p, k]):
                left += 1
            else:
                moved += 1
    assert moved >= 20 and left >= 1 and skipped >= 1, (moved, left, skipped)
    rest = np.ones(4096, bool)
    rest[[p for p, _ in cases.SUBPIX_LIVE]] = False
    assert np.array_equal(want[rest].view(np.uint32), kp[rest].view(np.uint32))
