"""GPU: cyclic panorama columns at the stage level -- sosvo_gray_pyramid_cyclic and sosvo_track_lk with
SOSVO_LK_CYCLIC_COLUMNS against tests/reflk_cyclic.py bit for bit (windows on a 16-lane group and on a whole wave, 1 and 3
levels, starts in the twelve columns on either side of the seam, both shift signs, the initial-flow flag, the forward-backward
check, a row range), the plain call's bits away from the seam, the refusals, and the cyclic |du| gate of the two assembles and
of the gated matcher against numpy restatements on hand-made problems."""
import ctypes

import numpy as np
import pytest
import torch

import matching_scenes as scenes
import reflk_cyclic as rc
from refmatch import IDX, NONE, capped, two_smallest_keys
from vo_single_camera_sos_amd import _lib
from vo_single_camera_sos_amd.device import make_rig
from vo_single_camera_sos_amd.omnistereo import common_cv

pytestmark = pytest.mark.gpu

ROWS, W, CAP, MAX_ITER = 96, 128, 80, 10
SHIFTS = ((5.3, -3.6), (-5.3, 3.6))
PREV_IMG, NEXT_IMG = (0, 2, 0, 2), (1, 3, 1, 3)     # view-major: pair A = images (0, 1) of view 0, pair B = (2, 3) of view 1
COUNTS = (72, 1, 64, 0)
FEW = (30, 1, 24, 0)                                  # what the whole-wave window (half 10) is compared on
SENTINEL = np.float32(-123.25)
ROW_RANGE = np.array([[21, 70], [9, 96]], np.int32)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _starts(rng, count):
    """count starts: the columns 0 .. 11 and W - 12 .. W - 1 first (integer and fractional rows), then anywhere on the circle
    and a little beyond it, a NaN, a start just below column W and one above the first row."""
    kp = np.full((CAP, 2), SENTINEL, np.float32)
    seam = list(range(12)) + list(range(W - 12, W))
    for k in range(count):
        if k < 24:
            kp[k] = seam[k], (30 + 2 * k if k % 2 else rng.uniform(26, 66))
        elif k % 3 == 0:
            kp[k] = rng.uniform(-3, W + 3), rng.uniform(24, 70)
        else:
            kp[k] = rng.uniform(0, W), rng.uniform(24, 70)
    if count >= 30:
        kp[24] = np.nan, 30
        kp[25] = W - 1 / 64, 40                            # rounds to column W = column 0
        kp[26] = 3.5, -0.6                                 # the rows keep their edge: lost
        kp[27] = W - 0.25, 44.5
    return kp


@pytest.fixture(scope="module")
def scene():
    """Two shifted pairs of the periodic texture (one per shift sign), the starts, the reference pyramids per (levels, row
    range): host arrays, built once and never written."""
    rng = np.random.default_rng(31)
    gray = np.stack([rc.texture(7, ROWS, W), rc.texture(7, ROWS, W, SHIFTS[0]), rc.texture(8, ROWS, W), rc.texture(8, ROWS, W, SHIFTS[1])])
    pts = np.stack([_starts(rng, c) for c in COUNTS])
    s = dict(gray=gray, pts=pts, n=np.array(COUNTS, np.int32), few=np.array(FEW, np.int32), pyrs={})

    def pyrs(levels, row_range=None):
        key = (levels, None if row_range is None else row_range.tobytes())
        if key not in s["pyrs"]:
            s["pyrs"][key] = rc.pyramid_set(gray, levels, row_range)
        return s["pyrs"][key]
    s["ref_pyrs"] = pyrs
    return s


def _device_track(ctx, gray, levels, pts, n, half, guess=None, fb_max=None, row_range=None, prev_img=PREV_IMG, next_img=NEXT_IMG,
                  cyclic=True):
    """-> (next, status, err[, back]) as numpy; every output buffer starts as the sentinel (0xA5 for the status)."""
    rr = None if row_range is None else _dev(ctx, row_range)
    pyr = (ctx.gray_pyramid_cyclic if cyclic else ctx.gray_pyramid)(_dev(ctx, gray), levels, row_range=rr)
    P = len(prev_img)
    nxt = torch.full((P, CAP, 2), float(SENTINEL), dtype=torch.float32, device=ctx.device)
    out = (nxt, torch.full((P, CAP), 0xA5, dtype=torch.uint8, device=ctx.device),
           torch.full((P, CAP), float(SENTINEL), dtype=torch.float32, device=ctx.device),
           torch.full((P, CAP, 2), float(SENTINEL), dtype=torch.float32, device=ctx.device))
    if guess is not None:
        nxt.copy_(_dev(ctx, guess))
    res = ctx.track_lk(pyr, _dev(ctx, np.array(prev_img, np.int32)), _dev(ctx, np.array(next_img, np.int32)), _dev(ctx, pts),
                       _dev(ctx, n), half=half, max_iter=MAX_ITER, next_pts=nxt if guess is not None else None, fb_max=fb_max,
                       out=out)
    ctx.synchronize()
    return tuple(t.cpu().numpy() for t in res)


def _sentinels(guess=None):
    P = len(PREV_IMG)
    return (np.full((P, CAP, 2), SENTINEL, np.float32) if guess is None else guess.copy(), np.full((P, CAP), 0xA5, np.uint8),
            np.full((P, CAP), SENTINEL, np.float32), np.full((P, CAP, 2), SENTINEL, np.float32))


def _assert_equal(got, want, n, what):
    """next / err / back as uint32 bit patterns, status as bytes; the rows at and beyond n[p] hold what they held."""
    assert len(got) == len(want)
    for g, w, name in zip(got, want, ("next", "status", "err", "back")):
        g, w = (a if a.dtype == np.uint8 else _u32(a) for a in (g, w))
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, name, bad[:4], [(g[tuple(b)], w[tuple(b)]) for b in bad[:4]])
    assert sum(int(c) for c in n) > 0


def _reference(s, levels, n, half, row_range=None, guess=None, fb_max=None):
    return rc.track_problems(s["ref_pyrs"](levels, row_range), PREV_IMG, NEXT_IMG, s["pts"], n, half, MAX_ITER, next_pts=guess,
                             fb_max=fb_max, out=_sentinels(guess))


# ---- the pyramid -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,levels,row_range", [(12, 16, 3, None), (ROWS, W, 4, None),
                                                        (95, 24, 2, np.array([[94, 95], [-3, 40]], np.int32)),
                                                        (33, 200, 4, np.array([[5, 30], [0, 33]], np.int32))])
def test_pyramid_equals_the_reference_byte_for_byte(ctx, rows, cols, levels, row_range):
    """The device buffer starts as 0xAB, so the rows outside a range are seen to stay.  (12, 16): a top level of 4 columns, a
    tile far wider than the level; 200 columns: more than one tile, the wrap in the last one."""
    rng = np.random.default_rng(rows + cols)
    gray = rng.integers(0, 256, (4, rows, cols), dtype=np.uint8)
    sizes = rc.level_sizes(rows, cols, levels)
    assert _lib.gray_pyramid_bytes(4, rows, cols, levels) == 4 * sum(r * c for r, c in sizes[1:])
    d_gray = _dev(ctx, gray)
    rr = None if row_range is None else _dev(ctx, row_range)
    pyr = ctx.gray_pyramid_cyclic(d_gray, levels, row_range=rr)
    pyr.upper.fill_(0xAB)
    pyr = ctx.gray_pyramid_cyclic(d_gray, levels, row_range=rr, out=pyr)
    assert pyr.cyclic
    plain = ctx.gray_pyramid(d_gray, levels, row_range=rr)
    ctx.synchronize()
    differs = False
    for i in range(4):
        fill = [np.full(sz, 0xAB, np.uint8) for sz in sizes[1:]]
        want, _ = rc.pyramid(gray[i], levels, None if row_range is None else row_range[i // 2], fill=fill)
        for l in range(1, levels):
            got = pyr.level(l)[i].cpu().numpy()
            assert np.array_equal(got, want[l]), (i, l)
            differs |= not np.array_equal(got, plain.level(l)[i].cpu().numpy())
    assert differs                                            # (the wrap did act: the clamped pyramid is another one)
    assert np.array_equal(d_gray.cpu().numpy(), gray)


# ---- the tracker against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("half", [2, 4, 10])
def test_track_equals_the_reference_bit_for_bit(ctx, scene, half, levels):
    s = scene
    n = s["few"] if half == 10 else s["n"]
    got = _device_track(ctx, s["gray"], levels, s["pts"], n, half)
    _assert_equal(got, _reference(s, levels, n, half), n, (half, levels))
    nxt, st, _ = got
    for p in (0, 2):                                          # both shift signs
        k = int(n[p])
        assert st[p, :24].sum() >= 23                         # the 24 starts at the seam (half 2 on one level loses one: no texture)
        assert ((nxt[p, :k, 0] >= 0) & (nxt[p, :k, 0] < W))[st[p, :k] == 1].all()
        crossed = (np.abs(nxt[p, :k, 0] - s["pts"][p, :k, 0]) > W / 2) & (st[p, :k] == 1)
        assert crossed.sum() >= 5, (p, crossed.sum())         # (columns 0 .. 5 / W - 6 .. W - 1 move across)
    assert st[0, 24] == 0 and np.array_equal(_u32(nxt[0, 24]), _u32(s["pts"][0, 24]))        # the non-finite start: next = prev
    assert st[0, 26] == 0                                                                    # off the rows
    assert st[0, 25] == 1 and 0.0 <= nxt[0, 25, 0] < W


def test_track_with_the_initial_flow_flag(ctx, scene):
    s = scene
    rng = np.random.default_rng(5)
    guess = (s["pts"] + np.float32(1.0) + rng.uniform(-1, 1, s["pts"].shape)).astype(np.float32)
    guess[:, :12, 0] -= np.float32(4.0)                          # guesses on the far side of the seam
    guess[2, 7] = np.nan, 3.0
    guess[:, CAP - 3:] = SENTINEL
    for half, levels in ((4, 3), (2, 1)):
        got = _device_track(ctx, s["gray"], levels, s["pts"], s["n"], half, guess=guess)
        _assert_equal(got, _reference(s, levels, s["n"], half, guess=guess), s["n"], (half, levels))
        assert got[1][2, 7] == 0 and np.array_equal(_u32(got[0][2, 7]), _u32(s["pts"][2, 7]))
    plain = _device_track(ctx, s["gray"], 1, s["pts"], s["n"], 2)
    assert not np.array_equal(_u32(plain[0]), _u32(got[0]))      # (the guesses did act)


@pytest.mark.parametrize("half,levels", [(4, 3), (2, 1), (10, 3)])
def test_track_with_the_forward_backward_check(ctx, scene, half, levels):
    s = scene
    n = s["few"] if half == 10 else s["n"]
    got = _device_track(ctx, s["gray"], levels, s["pts"], n, half, fb_max=0.25)
    _assert_equal(got, _reference(s, levels, n, half, fb_max=0.25), n, (half, levels))
    fwd = _device_track(ctx, s["gray"], levels, s["pts"], n, half)
    assert np.array_equal(_u32(fwd[0]), _u32(got[0])) and np.array_equal(_u32(fwd[2]), _u32(got[2]))
    assert ((got[1] == 0) | (fwd[1] == got[1])).all()            # the check only clears
    if levels == 3:                                              # points that crossed the seam come back and are kept
        crossed = (np.abs(got[0][0, 12:24, 0] - s["pts"][0, 12:24, 0]) > W / 2) & (got[1][0, 12:24] == 1)
        assert crossed.any()


def test_track_under_a_row_range_ignores_the_rows_outside(ctx, scene):
    s = scene
    outs = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        gray = s["gray"].copy()
        for i in range(4):
            r0, r1 = ROW_RANGE[i // 2]
            gray[i, :r0] = rng.integers(0, 256, (r0, W))
            gray[i, r1:] = rng.integers(0, 256, (ROWS - r1, W))
        outs.append(_device_track(ctx, gray, 3, s["pts"], s["n"], 4, row_range=ROW_RANGE))
    want = _reference(s, 3, s["n"], 4, row_range=ROW_RANGE)
    _assert_equal(outs[0], want, s["n"], "noise 1")
    _assert_equal(outs[1], want, s["n"], "noise 2")


def test_rows_at_and_beyond_the_count_are_untouched(ctx, scene):
    s = scene
    got = _device_track(ctx, s["gray"], 3, s["pts"], s["n"], 4, fb_max=0.25)
    for p, c in enumerate(COUNTS):
        assert (_u32(got[0][p, c:]) == _u32(SENTINEL)).all() and (got[1][p, c:] == 0xA5).all()
        assert (_u32(got[2][p, c:]) == _u32(SENTINEL)).all() and (_u32(got[3][p, c:]) == _u32(SENTINEL)).all()


def test_away_from_the_seam_the_flag_changes_no_bit(ctx, scene):
    """Starts in x = 40 .. 88 of 128 columns, half 4, 3 levels, shifts of a few pixels: no window touches a border on any level,
    so the cyclic pyramid's columns that are read and every tap are the plain call's."""
    s = scene
    rng = np.random.default_rng(9)
    pts = np.full((4, CAP, 2), SENTINEL, np.float32)
    n = np.array([60, 1, 40, 0], np.int32)
    for p in range(4):
        pts[p, :n[p]] = np.stack([rng.uniform(40, 88, n[p]), rng.uniform(30, 62, n[p])], -1)
    for fb in (None, 0.25):
        a = _device_track(ctx, s["gray"], 3, pts, n, 4, fb_max=fb, cyclic=True)
        b = _device_track(ctx, s["gray"], 3, pts, n, 4, fb_max=fb, cyclic=False)
        _assert_equal(a, b, n, "interior")
        assert a[1][0, :60].sum() > 50
    seam = _device_track(ctx, s["gray"], 3, s["pts"], s["n"], 4, cyclic=False)
    assert not np.array_equal(seam[1], _device_track(ctx, s["gray"], 3, s["pts"], s["n"], 4)[1])    # (at the seam it does)


def test_host_mirror_takes_the_option(ctx, scene):
    s = scene
    pts = s["pts"][0, :COUNTS[0]]
    nxt, st, err = common_cv.calc_optical_flow_pyr_lk(s["gray"][0], s["gray"][1], pts.reshape(-1, 1, 2), win_half=4, max_level=2,
                                                      max_iter=MAX_ITER, ctx=ctx, cyclic=True)
    want = _device_track(ctx, s["gray"][:2], 3, s["pts"][:1], s["n"][:1], 4, prev_img=[0], next_img=[1])
    assert np.array_equal(_u32(nxt[:, 0]), _u32(want[0][0, :COUNTS[0]])) and np.array_equal(st[:, 0], want[1][0, :COUNTS[0]])
    assert np.array_equal(_u32(err[:, 0]), _u32(want[2][0, :COUNTS[0]]))
    with pytest.raises(ValueError, match="127"):
        common_cv.calc_optical_flow_pyr_lk(s["gray"][0][:, :127], s["gray"][1][:, :127], pts, win_half=4, max_level=2, ctx=ctx, cyclic=True)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_the_stages_refuse_bad_arguments(ctx):
    lib = _lib.load()
    gray = torch.zeros((2, 16, 32), dtype=torch.uint8, device=ctx.device)
    upper = torch.zeros((_lib.gray_pyramid_bytes(2, 16, 32, 4),), dtype=torch.uint8, device=ctx.device)
    pts = torch.zeros((1, 4, 2), dtype=torch.float32, device=ctx.device)
    st = torch.zeros((1, 4), dtype=torch.uint8, device=ctx.device)
    err = torch.zeros((1, 4), dtype=torch.float32, device=ctx.device)
    i32 = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def pyramid(cols=32, levels=3, fn=lib.sosvo_gray_pyramid_cyclic):
        return fn(ctx._h, p(gray), 2, 16, cols, levels, None, p(upper))

    def track(cols=32, levels=2, half=4, flags=_lib.LK_CYCLIC_COLUMNS):
        return lib.sosvo_track_lk(ctx._h, p(gray), p(upper), 2, 16, cols, levels, None, p(i32), p(i32), 1, 4, p(pts), p(i32), half, 10,
                                  0.01, 1e-4, flags, p(pts), p(st), p(err), None, 0.0)
    assert pyramid() == 0 and track() == 0 and track(flags=_lib.LK_CYCLIC_COLUMNS | _lib.LK_INITIAL_FLOW) == 0
    assert pyramid(cols=20, levels=3) == 0                    # 20 = 4 * 5: three levels are whole periods
    for bad in (dict(cols=31, levels=2), dict(cols=30, levels=3), dict(cols=20, levels=4), dict(levels=5)):
        assert pyramid(**bad) == -1, bad
        assert "sosvo_gray_pyramid_cyclic" in lib.sosvo_last_error(ctx._h).decode()
    assert pyramid(cols=31, levels=2, fn=lib.sosvo_gray_pyramid) == 0     # (the plain call takes any width)
    # flags = 8 and flags = 2 are no flags; 20 columns with 3 levels leave 5 on the top level, fewer than any template;
    # half 4 at 2 levels of 20 columns: 10 < 11; an odd width
    for bad in (dict(flags=8), dict(flags=2), dict(flags=_lib.LK_CYCLIC_COLUMNS | 8), dict(cols=20, levels=3, half=2),
                dict(cols=20, levels=3), dict(cols=20, levels=2), dict(cols=31, levels=2), dict(cols=30, levels=3)):
        assert track(**bad) == -1, bad
        assert "sosvo_track_lk" in lib.sosvo_last_error(ctx._h).decode()
    assert track(cols=20, levels=3, flags=0) == 0             # (without the flag the sizes are fine)
    assert track(cols=20, levels=1) == 0 and track(cols=22, levels=2) == 0
    with pytest.raises(_lib.SosvoError):
        ctx.gray_pyramid_cyclic(gray[:, :, :31].contiguous(), 2)
    ctx.synchronize()


# ---- the assembles -------------------------------------------------------------------------------------------------------------
PERIOD_CASES = [1440.5, 0.0, -1440.0, float("nan"), 16385.0]


def _frames(rng, F, Fc, cols, rows, M):
    m = [np.stack([rng.uniform(0, cols, (F, Fc)), rng.uniform(8, rows - 8, (F, Fc))], -1).astype(np.float32) for _ in range(2)]
    return m, rng.uniform(-3000, 3000, (F, Fc, 3)), [rng.normal(size=(F, Fc, 3)) for _ in range(2)], np.array(M, np.int32)


def test_tracked_assemble_with_the_cyclic_gate_equals_a_numpy_restatement(ctx):
    """4 pairs over 4 frames, frame_cap 8, corr_cap 9; the reference frames hold 8, 0, 1 and 8 points.  Pair 0: tracks on both
    sides of the seam, one at each boundary of the gate (d = 90, W - d = 90) and one float32 step beyond each, a lost point."""
    rng = np.random.default_rng(43)
    _, rig_kw = scenes.rig()
    cols, rows = rig_kw["pano_top"][0], rig_kw["pano_top"][1]
    assert cols == int(cols) and rig_kw["pano_bot"][0] == cols
    F, Fc, Cc, NP, g = 4, 8, 9, 4, 90.0
    m, X, _, M = _frames(rng, F, Fc, cols, rows, [8, 0, 1, 8])
    ref = np.array([0, 1, 2, 3], np.int32)
    trk = [(m[v][ref] + rng.uniform(-6, 6, (NP, Fc, 2))).astype(np.float32) for v in range(2)]
    st = [np.ones((NP, Fc), np.uint8) for _ in range(2)]
    up = np.float32(1.0) * np.float32(cols)
    m[0][0, :6, 0] = [3.0, cols - 2.5, 100.0, 100.0, 40.0, 40.0]
    trk[0][0, :6, 0] = [cols - 10.0, 7.25, 190.0, np.nextafter(np.float32(190.0), up), cols - 50.0, np.nextafter(np.float32(cols - 50.0), np.float32(0))]
    m[1][0, :3, 0] = [cols - 1.0, 5.0, 700.0]
    trk[1][0, :3, 0] = [0.0, cols - 80.0, 700.0 + cols / 2]
    st[0][0, 7], st[1][0, 6] = 0, 0
    m[0][2, 0, 0], trk[0][2, 0, 0] = 1.0, cols - 1.0             # the frame with one point: across the seam
    frames = dict(m_top=_dev(ctx, m[0]), m_bot=_dev(ctx, m[1]), X=_dev(ctx, X), M=_dev(ctx, M))
    sentinel = lambda: dict(f=torch.full((NP, Cc, 3), -7.0, dtype=torch.float64, device=ctx.device),  # noqa: E731
                            p=torch.full((NP, Cc, 3), -7.0, dtype=torch.float64, device=ctx.device),
                            cam=torch.full((NP, Cc), -7, dtype=torch.int32, device=ctx.device),
                            q=torch.full((NP, Cc), -7, dtype=torch.int32, device=ctx.device),
                            t=torch.full((NP, Cc), -7, dtype=torch.int32, device=ctx.device),
                            n=torch.full((NP,), -7, dtype=torch.int32, device=ctx.device),
                            n_top=torch.full((NP,), -7, dtype=torch.int32, device=ctx.device))
    seen = {}
    for hdiff in (g, -1.0, 0.0):
        rig = make_rig(**dict(rig_kw, f2f_max_hdiff=hdiff))
        for cyclic in (True, False):
            out = ctx.f2f_assemble_tracked(rig, frames, _dev(ctx, ref), _dev(ctx, trk[0]), _dev(ctx, trk[1]), _dev(ctx, st[0]),
                                           _dev(ctx, st[1]), Cc, out=sentinel(), cyclic=cyclic)
            ctx.synchronize()
            got = {k: v.cpu().numpy() for k, v in out.items()}
            for pr in range(NP):
                rows_, nt = [], min(int(M[ref[pr]]), Fc)
                for v in range(2):
                    a, b = m[v][ref[pr], :nt, 0], trk[v][pr, :nt, 0]
                    ok = rc.du_gate(a, b, hdiff, cols) if cyclic else rc.du_gate_plain(a, b, hdiff)
                    rows_ += [(v, k) for k in range(nt) if st[v][pr, k] and ok[k]]
                    if v == 0:
                        n_top = min(len(rows_), Cc)
                rows_ = rows_[:Cc]
                assert got["n"][pr] == len(rows_) and got["n_top"][pr] == n_top, (pr, hdiff, cyclic)
                assert [(int(c), int(t)) for c, t in zip(got["cam"][pr, :len(rows_)], got["t"][pr, :len(rows_)])] == rows_
                assert (got["q"][pr, :len(rows_)] == -1).all()
                for i, (v, k) in enumerate(rows_):
                    assert np.array_equal(got["p"][pr, i], X[ref[pr], k])
                    pano = rig_kw["pano_top" if v == 0 else "pano_bot"]
                    bb = ctx.pano_to_bearing(_dev(ctx, trk[v][pr, k].astype(np.float64).reshape(1, 2)), *pano)[2]
                    assert np.array_equal(got["f"][pr, i], bb.cpu().numpy()[0])
                # rows at and beyond the count are untouched
                assert (got["cam"][pr, len(rows_):] == -7).all() and (got["f"][pr, len(rows_):] == -7.0).all()
                assert (got["t"][pr, len(rows_):] == -7).all() and (got["p"][pr, len(rows_):] == -7.0).all()
            seen[(hdiff, cyclic)] = got
    on, off = seen[(g, True)], seen[(g, False)]
    assert [int(t) for t in on["t"][0, :on["n_top"][0]]] == [0, 1, 2, 4, 6]      # 3: d one step beyond 90; 5: W - d beyond; 7: lost
    assert [int(t) for t in off["t"][0, :off["n_top"][0]]] == [2, 6]
    assert on["n"][1] == 0 and on["n"][2] == 2 and off["n"][2] == 1 and on["n"][3] == Cc
    for k in ("n", "n_top", "cam", "t"):                        # the disabled gate: both forms keep the same rows
        assert np.array_equal(seen[(-1.0, True)][k], seen[(-1.0, False)][k]) and np.array_equal(seen[(0.0, True)][k], seen[(0.0, False)][k])
    # a period that is no positive integer
    lib = _lib.load()
    for bad in PERIOD_CASES:
        for name in ("pano_top", "pano_bot"):
            rig = make_rig(**dict(rig_kw, f2f_max_hdiff=g, **{name: (bad,) + tuple(rig_kw[name][1:])}))
            with pytest.raises(_lib.SosvoError, match="sosvo_f2f_assemble_tracked_cyclic"):
                ctx.f2f_assemble_tracked(rig, frames, _dev(ctx, ref), _dev(ctx, trk[0]), _dev(ctx, trk[1]), _dev(ctx, st[0]),
                                         _dev(ctx, st[1]), Cc, cyclic=True)
    assert "sosvo_f2f_assemble_tracked_cyclic" in lib.sosvo_last_error(ctx._h).decode()


def test_matched_assemble_with_the_cyclic_gate_equals_a_numpy_restatement(ctx):
    """3 pairs over 4 frames holding 8, 0, 1 and 8 points; hand-made keys (a NONE among them) in a shuffled rank order."""
    rng = np.random.default_rng(47)
    _, rig_kw = scenes.rig()
    cols, rows = rig_kw["pano_top"][0], rig_kw["pano_top"][1]
    F, Fc, Cc, g = 4, 8, 6, 90.0
    m, X, b, M = _frames(rng, F, Fc, cols, rows, [8, 0, 1, 8])
    ref, cur = np.array([0, 3, 2], np.int32), np.array([3, 1, 0], np.int32)    # (8 x 8, an empty current frame, 8 queries x 1 train)
    NP = len(ref)
    keys = [np.full((NP, Fc, 1), NONE, np.uint32) for _ in range(2)]
    order = [np.stack([rng.permutation(Fc) for _ in range(NP)]).astype(np.int32) for _ in range(2)]
    for v in range(2):
        keys[v][0, :, 0] = (rng.integers(0, 60, Fc).astype(np.uint32) << 20) | rng.permutation(Fc).astype(np.uint32)
        keys[v][0, 5, 0] = NONE
        keys[v][2, :, 0] = rng.integers(0, 60, Fc).astype(np.uint32) << 20           # every query of pair 2 chose train 0
    t_of = lambda v, q: int(keys[v][0, q, 0] & IDX)  # noqa: E731
    # pair 0, top view: query q of frame 3 against its train of frame 0
    for q, (u_t, u_q) in enumerate([(2.0, cols - 3.0), (cols - 0.5, 60.0), (500.0, 590.0), (500.0, np.nextafter(np.float32(590.0), np.float32(600))),
                                    (30.0, cols - 60.0), (0.0, 0.0), (30.0, np.nextafter(np.float32(cols - 60.0), np.float32(0))), (700.0, 20.0)]):
        if q != 5:                                               # (query 5 has no match)
            m[0][3, q, 0], m[0][0, t_of(0, q), 0] = u_q, u_t
    m[0][2, 0, 0], m[1][2, 0, 0] = cols - 20.0, 15.0             # pair 2's one train per view, and its bottom queries
    m[1][0, :, 0] = [cols - 5.0, 3.0, 20.0, cols - 70.0, 104.0, 500.0, 900.0, 106.0]
    frames = dict(m_top=_dev(ctx, m[0]), m_bot=_dev(ctx, m[1]), X=_dev(ctx, X), b_top=_dev(ctx, b[0]), b_bot=_dev(ctx, b[1]),
                  M=_dev(ctx, M))
    seen = {}
    for hdiff in (g, -1.0):
        rig = make_rig(**dict(rig_kw, f2f_max_hdiff=hdiff))
        for cyclic in (True, False):
            out = dict(f=torch.full((NP, Cc, 3), -7.0, dtype=torch.float64, device=ctx.device),
                       p=torch.full((NP, Cc, 3), -7.0, dtype=torch.float64, device=ctx.device),
                       cam=torch.full((NP, Cc), -7, dtype=torch.int32, device=ctx.device),
                       q=torch.full((NP, Cc), -7, dtype=torch.int32, device=ctx.device),
                       t=torch.full((NP, Cc), -7, dtype=torch.int32, device=ctx.device),
                       n=torch.full((NP,), -7, dtype=torch.int32, device=ctx.device),
                       n_top=torch.full((NP,), -7, dtype=torch.int32, device=ctx.device))
            ctx.f2f_assemble(rig, frames, _dev(ctx, ref), _dev(ctx, cur), _dev(ctx, keys[0]), _dev(ctx, order[0]), _dev(ctx, keys[1]),
                             _dev(ctx, order[1]), Cc, out=out, cyclic=cyclic)
            ctx.synchronize()
            got = {k: v.cpu().numpy() for k, v in out.items()}
            for pr in range(NP):
                nq, nt = min(int(M[cur[pr]]), Fc), min(int(M[ref[pr]]), Fc)
                rows_ = []
                for v in range(2):
                    for r in range(nq if nt else 0):
                        q = int(order[v][pr, r])
                        key = int(keys[v][pr, q, 0])
                        if key == NONE:
                            continue
                        t = key & IDX
                        a, c = m[v][ref[pr], t, 0], m[v][cur[pr], q, 0]
                        if (rc.du_gate([a], [c], hdiff, cols) if cyclic else rc.du_gate_plain([a], [c], hdiff))[0]:
                            rows_.append((v, q, t))
                    if v == 0:
                        n_top = min(len(rows_), Cc)
                rows_ = rows_[:Cc]
                assert got["n"][pr] == len(rows_) and got["n_top"][pr] == n_top, (pr, hdiff, cyclic, got["n"][pr], len(rows_))
                assert [(int(c), int(q), int(t)) for c, q, t in zip(got["cam"][pr], got["q"][pr], got["t"][pr])][:len(rows_)] == rows_
                for i, (v, q, t) in enumerate(rows_):
                    assert np.array_equal(got["f"][pr, i], b[v][cur[pr], q]) and np.array_equal(got["p"][pr, i], X[ref[pr], t])
                assert (got["cam"][pr, len(rows_):] == -7).all() and (got["f"][pr, len(rows_):] == -7.0).all()
            seen[(hdiff, cyclic)] = got
    on, off = seen[(g, True)], seen[(g, False)]
    top_q = lambda s: sorted(int(q) for q in s["q"][0, :s["n_top"][0]])  # noqa: E731
    assert top_q(on) == [0, 1, 2, 4] and top_q(off) == [2]       # 3, 6: one step beyond a boundary; 5: no match; 7: far
    assert on["n"][1] == 0 and on["n"][2] == Cc                  # pair 2: 8 queries on one train, both views across the seam
    assert off["n"][2] < on["n"][2]
    with pytest.raises(_lib.SosvoError, match="sosvo_f2f_assemble_cyclic"):
        rig = make_rig(**dict(rig_kw, f2f_max_hdiff=g, pano_bot=(cols + 0.5,) + tuple(rig_kw["pano_bot"][1:])))
        ctx.f2f_assemble(rig, frames, _dev(ctx, ref), _dev(ctx, cur), _dev(ctx, keys[0]), _dev(ctx, order[0]), _dev(ctx, keys[1]),
                         _dev(ctx, order[1]), Cc, cyclic=True)


# ---- the gated matcher -----------------------------------------------------------------------------------------------------------
def _cyclic_gate_matrix(q_pos, t_pos, max_du, period):
    """gate(i, j) of sosvo_match_hamming_gated_cyclic: d <= max_du or d >= period - max_du, the right side formed once."""
    d = np.abs(t_pos[None, :, 0].astype(np.float64) - q_pos[:, None, 0].astype(np.float64))
    if not max_du > 0:
        return np.ones(d.shape, bool)
    return (d <= max_du) | (d >= float(period) - max_du)


def test_gated_matcher_with_the_cyclic_gate_equals_a_numpy_restatement(ctx):
    """Stride 160 (two train tiles, the range split over workgroups); problems with 0, 1 and 160 queries / trains, positions all
    around a circle of 1440 columns, every second train a re-observation of a query a few columns away -- across the seam for
    the queries near it.  Constructed rows of problem 0 sit at both gate boundaries and one float32 step beyond them."""
    rng = np.random.default_rng(53)
    S, P, period, g = 160, 4, 1440, 90.0
    nq, nt = np.array([160, 1, 0, 97]), np.array([160, 160, 31, 1])
    qd = rng.integers(0, 256, (P, S, 32), dtype=np.uint8)
    td = rng.integers(0, 256, (P, S, 32), dtype=np.uint8)
    qp = np.stack([rng.uniform(0, period, (P, S)), rng.uniform(0, 300, (P, S))], -1).astype(np.float32)
    tp = np.stack([rng.uniform(0, period, (P, S)), rng.uniform(0, 300, (P, S))], -1).astype(np.float32)
    qp[0, :40, 0] = rng.uniform(0, 30, 40)                           # queries at the seam, their partners on the other side
    for p_ in range(P):
        for j in range(0, int(nt[p_]), 2):
            i = int(rng.integers(0, max(1, nq[p_])))
            td[p_, j] = qd[p_, i]
            td[p_, j, rng.integers(0, 32)] ^= np.uint8(1 << rng.integers(0, 8))
            tp[p_, j, 0] = np.float32((float(qp[p_, i, 0]) + rng.uniform(-100, 100)) % period)
    # constructed: query 150 .. 155 each with ONE exact copy, placed by hand (the other trains' copies lose to distance 0)
    hand = [(150, 10.0, 100.0, True), (151, 10.0, np.nextafter(np.float32(100.0), np.float32(200)), False),
            (152, 10.0, 1360.0, True), (153, 10.0, np.nextafter(np.float32(1360.0), np.float32(0)), False),
            (154, 1439.5, 3.25, True), (155, 700.0, 1420.0, False)]
    for i, u_q, u_t, _ in hand:
        td[0, i] = qd[0, i]
        qp[0, i, 0], tp[0, i, 0] = u_q, u_t
    d = [_dev(ctx, a) for a in (qd, td, qp, tp)]
    d_nq, d_nt = _dev(ctx, nq.astype(np.int32)), _dev(ctx, nt.astype(np.int32))
    for max_du, cap in ((g, None), (g, 40), (37.5, None), (-1.0, None), (0.0, 256)):
        keys = ctx.match_hamming_gated_cyclic(d[0], d[1], d[2], d[3], d_nq, d_nt, max_du, period, max_distance=cap)
        plain = ctx.match_hamming_gated(d[0], d[1], d[2], d[3], d_nq, d_nt, -1.0, max_du, max_distance=cap)
        ctx.synchronize()
        keys, plain = keys.cpu().numpy()[:, :, 0], plain.cpu().numpy()[:, :, 0]
        for p_ in range(P):
            n, k = int(nq[p_]), int(nt[p_])
            adm = _cyclic_gate_matrix(qp[p_, :n], tp[p_, :k], max_du, period)
            want = capped(two_smallest_keys(qd[p_, :n], td[p_, :k], adm)[0], cap)
            assert np.array_equal(keys[p_, :n], want), (p_, max_du, cap)
            if not max_du > 0:
                assert np.array_equal(keys[p_, :n], plain[p_, :n])
            else:                                                      # the cyclic gate only admits more: a key never gets worse
                assert (keys[p_, :n] <= plain[p_, :n]).all()
        if max_du == g and cap is None:
            for i, _, _, passes in hand:
                assert (keys[0, i] == i) == passes, i                  # distance 0, train i -- or another train / NONE
            assert (keys[0, :40] != plain[0, :40]).any()               # partners found across the seam
    # reversed problems and slots: the u side is symmetric, so the role-swapped twin of problem 0 through slot tables
    # equals the forward search with the blocks swapped
    both_d = torch.cat([d[0][:1], d[1][:1]]), torch.cat([d[2][:1], d[3][:1]])
    cnt = _dev(ctx, np.array([160, 160], np.int32))
    qs, ts = _dev(ctx, np.array([0, 1], np.int32)), _dev(ctx, np.array([1, 0], np.int32))
    tw = ctx.match_hamming_gated_cyclic(both_d[0], both_d[0], both_d[1], both_d[1], cnt, cnt, g, period, q_slot=qs, t_slot=ts, n_forward=1)
    fw = ctx.match_hamming_gated_cyclic(d[1][:1], d[0][:1], d[3][:1], d[2][:1], cnt[:1], cnt[:1], g, period)
    ctx.synchronize()
    assert np.array_equal(tw.cpu().numpy()[1], fw.cpu().numpy()[0])
    lib = _lib.load()
    for bad in PERIOD_CASES:
        with pytest.raises(_lib.SosvoError, match="sosvo_match_hamming_gated_cyclic"):
            ctx.match_hamming_gated_cyclic(d[0], d[1], d[2], d[3], d_nq, d_nt, g, bad)
    assert "sosvo_match_hamming_gated_cyclic" in lib.sosvo_last_error(ctx._h).decode()
