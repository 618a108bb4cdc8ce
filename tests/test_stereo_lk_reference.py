"""CPU: the rule of sosvo_refine_stereo_lk as tests/refstereolk.py restates it -- what the planted-shift scene gives, the
reverts, and the pre-gate against refining everything."""
import numpy as np
import pytest

import reflk
import refstereolk as ref

_memo = {}


def _planted(k, half):
    """The refined tables of shift k at `half`, memoised."""
    if (k, half) not in _memo:
        t = ref.planted_tables(ref.SHIFTS[k])
        kp, st = ref.refine(t["gray"], 1, t["kp_top"], t["n_top"], t["kp_bot"], t["n_bot"], t["keys"], half=half)
        _memo[(k, half)] = (t, kp, st)
    return _memo[(k, half)]


@pytest.mark.parametrize("k", range(3))
def test_planted_shifts_are_recovered(k):
    """Half 4, the default: every one of the 120 tracks is accepted, none moves further than half from its guess, and the
    largest error stays below TWICE what reflk.track gave on this scene (0.0653 / 0.0716 / 0.0719 px; on the integer grid the
    partners are 0.425 / 0.602 / 0.361 px from the truth on average)."""
    t, kp, st = _planted(k, 4)
    n = len(t["truth"])
    assert n == 120 and st[0, :n].all() and not st[0, n:].any()
    err = ref.errors(kp, t["truth"])
    print("shift %r: mean %.4f max %.4f px (integer grid: mean %.3f)" % (ref.SHIFTS[k], err.mean(), err.max(),
                                                                          ref.errors(t["kp_bot"], t["truth"])[:60].mean()))
    assert np.abs(kp[0, :n] - t["kp_bot"][0, :n]).max() <= 4.0
    assert err.max() < 2.0 * ref.MEASURED_MAX[4][k]
    assert abs(err.max() - ref.MEASURED_MAX[4][k]) < 0.0006          # (the table is this run's, to its last printed digit)
    assert np.array_equal(kp[0, n:], t["kp_bot"][0, n:])              # rows beyond n_bot


def test_reverts_keep_the_bits_and_clear_the_status():
    t = ref.planted_tables(ref.SHIFTS[0])
    args = (t["gray"], 1, t["kp_top"], t["n_top"])
    # a guess 1 px off with max_shift 0.25: rows 60 .. 119 are 1 px off on both axes -- the track converges and is refused
    kp, st = ref.refine(*args, t["kp_bot"], t["n_bot"], t["keys"], max_shift=0.25)
    assert not st[0, 60:120].any() and np.array_equal(kp[0, 60:120].view(np.uint32), t["kp_bot"][0, 60:120].view(np.uint32))
    assert not st[0, :60].any()                     # (the rounded partners are 0.37 px off in x: refused as well)
    kp, st = ref.refine(*args, t["kp_bot"], t["n_bot"], t["keys"], max_shift=0.5)
    assert st[0, :60].all() and not st[0, 60:120].any() and np.abs(kp[0, :60] - t["kp_bot"][0, :60]).max() <= 0.5
    # a flat bottom image: J is the same everywhere, so every iteration takes the same step -- the point walks out of the bound
    # (or of the image).  A flat TOP image has no texture at all (min_eig): lost.
    for view in (1, 0):
        flat = t["gray"].copy()
        flat[view] = 128
        kp, st = ref.refine(flat, 1, t["kp_top"], t["n_top"], t["kp_bot"], t["n_bot"], t["keys"])
        assert not st.any() and np.array_equal(kp.view(np.uint32), t["kp_bot"].view(np.uint32)), view
    # SOSVO_KEY_NONE, a train index at n_top, non-finite keypoints
    keys, kb, kt = t["keys"].copy(), t["kp_bot"].copy(), t["kp_top"].copy()
    keys[0, 3] = ref.KEY_NONE
    keys[0, 5] = np.uint32(60 | (9 << 20))                                # n_top is 60
    kb[0, 7, 0] = np.nan
    kb[0, 8, 1] = np.inf
    kt[0, 9, 0] = -np.inf                                                  # the partner of rows 9 and 69
    kt[0, 10, 1] = np.nan
    kp, st = ref.refine(t["gray"], 1, kt, t["n_top"], kb, t["n_bot"], keys)
    for q in (3, 5, 7, 8, 9, 10, 69, 70):
        assert st[0, q] == 0 and np.array_equal(kp[0, q].view(np.uint32), kb[0, q].view(np.uint32)), q
    assert st[0, :120].sum() == 120 - 8
    # a status buffer keeps what it held beyond n_bot
    kp, st = ref.refine(*args, t["kp_bot"], t["n_bot"], t["keys"], status=np.full((1, 128), 7, np.uint8))
    assert (st[0, 120:] == 7).all() and (st[0, :120] == 1).all()


@pytest.mark.parametrize("k", range(3))
def test_pre_gate_never_changes_what_passes_the_assemble_gates(k):
    """stereo_max_hdiff 2.5, stereo_min_disp 1, half 4: partners displaced to both sides of each loosened bound (|du| = 6.5,
    dv = -3) and of each gate itself.  The refined kp_bot restricted to the pairs that pass the assemble gates afterwards is
    identical with and without the pre-gate, and the pre-gate does skip something."""
    H, D, half = 2.5, 1.0, 4
    gray, pts, true = ref.planted(ref.SHIFTS[k])
    pts = pts[::3]                                                          # 20 points
    n = len(pts)
    du = (-6.75, -6.5, -6.25, -2.75, -2.25, 0.0, 2.25, 2.75, 6.25, 6.5, 6.75)   # u_top - u_bot
    dv = (-3.25, -3.0, -2.75, 0.75, 1.25)                                       # v_top - v_bot
    rows = [(a, 5.0) for a in du] + [(0.0, b) for b in dv] + [(6.25, -2.75), (-6.75, -3.25)]
    cap = n * (len(rows) + 1)
    kp_top = np.zeros((1, cap, 2), np.float32)
    kp_top[0, :n] = pts
    kp_bot = np.zeros((1, cap, 2), np.float32)
    kp_bot[0, :n] = np.rint(true[::3])                                      # the matcher's partner, as in the planted scene
    for i, (a, b) in enumerate(rows):
        kp_bot[0, n * (i + 1):n * (i + 2)] = pts - np.array([a, b], np.float32)
    keys = (np.tile(np.arange(n), len(rows) + 1).astype(np.uint32) | np.uint32(3 << 20))[None]
    n_top, n_bot = np.array([n], np.int32), np.array([cap], np.int32)
    kw = dict(half=half, min_disp=D, max_hdiff=H)
    with_gate, st_with = ref.refine(gray, 1, kp_top, n_top, kp_bot, n_bot, keys, pre_gate=True, **kw)
    without, st_without = ref.refine(gray, 1, kp_top, n_top, kp_bot, n_bot, keys, pre_gate=False, **kw)
    t_of = keys[0] & ref.KEY_IDX_MASK
    passing = np.array([ref.passes_gates(*kp_top[0, t_of[q]], *without[0, q], D, H) for q in range(cap)])
    passing_with = np.array([ref.passes_gates(*kp_top[0, t_of[q]], *with_gate[0, q], D, H) for q in range(cap)])
    assert np.array_equal(passing, passing_with)
    assert passing.sum() >= n                                               # the planted partners pass
    assert np.array_equal(with_gate[0][passing].view(np.uint32), without[0][passing].view(np.uint32))
    assert np.array_equal(st_with[0][passing], st_without[0][passing])
    skipped = np.array([ref.pre_gate_skips(*kp_top[0, t_of[q]], *kp_bot[0, q], 4.0, D, H) for q in range(cap)])
    assert skipped[n * 1:n * 2].all() and not skipped[n * 2:n * 3].any()     # |du| 6.75 is skipped, 6.5 (the bound) is not
    assert skipped[n * 12:n * 13].all() and not skipped[n * 13:n * 14].any()   # dv -3.25 is skipped, -3 is not
    assert not st_with[0][skipped].any()
    assert not (skipped & passing).any()
    # each side is disabled exactly when the assemble stage's is
    assert not ref.pre_gate_skips(0.0, 0.0, 100.0, 0.0, 4.0, D, 0.0) and ref.pre_gate_skips(0.0, 0.0, 100.0, 0.0, 4.0, D, 1e-9)
    assert not ref.pre_gate_skips(0.0, 0.0, 0.0, 100.0, 4.0, -1e-9, H) and ref.pre_gate_skips(0.0, 0.0, 0.0, 100.0, 4.0, 0.0, H)


def test_measured_figures_of_the_other_window_sizes():
    """Half 2 and 10 on the first shift: the table's figures (0.182 and 0.0306 px), with the same margin."""
    for half in (2, 10):
        t, kp, st = _planted(0, half)
        err = ref.errors(kp, t["truth"])
        print("half %d: mean %.4f max %.4f px" % (half, err.mean(), err.max()))
        assert st[0, :120].all()
        assert np.abs(kp[0, :120] - t["kp_bot"][0, :120]).max() <= half
        assert err.max() < 2.0 * ref.MEASURED_MAX[half][0]


def test_the_planted_scene():
    gray, pts, true = ref.planted(ref.SHIFTS[1])
    assert gray.shape == (2, 96, 128) and pts.shape == (60, 2) and np.array_equal(gray[0], reflk.texture(7, 96, 128))
    assert np.allclose(true - pts, ref.SHIFTS[1])
